// process_baseband's ring endpoints: dump files and sink files (--replay, --out-sink / --co-sink), and psrdada rings
// through the flat C shim of include/pb_dada.h, bound at run time (dlopen of $PB_DADA_LIB or libpb_dada.so beside the
// program), so the program builds and runs replays where psrdada is absent.
#ifndef PB_HOST_RINGS_H
#define PB_HOST_RINGS_H

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "pb_dada.h"

namespace host {

struct ReadRing {
    virtual ~ReadRing() {}
    virtual int64_t next_header(char *dst) = 0;           // DADA_HDR bytes; 0 = no more observations; < 0 error
    virtual int64_t read(void *buf, size_t n) = 0;        // up to n bytes, fewer only at end of data
    virtual void finish_observation() {}
};
struct WriteRing {
    virtual ~WriteRing() {}
    virtual bool write_header(const std::string &hdr) = 0;
    virtual bool write(const void *buf, size_t n) = 0;
    virtual void end_of_data() = 0;
};

// Replay of dump files: each file = 4096-byte ASCII header + VDIF frame stream.  A single thread copies
// ~9 GB/s out of the page cache (28 ms per second of data); large reads of regular files go over 8 threads.
struct FileRing : ReadRing {
    std::vector<std::string> paths;
    int i = -1, fd = -1;
    bool regular = false;
    explicit FileRing(const std::vector<std::string> &p) : paths(p) {}
    ~FileRing();
    int64_t next_header(char *dst) override;
    int64_t read(void *buf, size_t n) override;
};

struct FileSink : WriteRing {
    FILE *fp;
    explicit FileSink(const std::string &path) : fp(fopen(path.c_str(), "wb")) {}
    ~FileSink();
    bool write_header(const std::string &hdr) override;
    bool write(const void *buf, size_t n) override;
    void end_of_data() override;
};

struct DadaRing : ReadRing, WriteRing {
    pb_dada *d = nullptr;
    bool header_posted = false;
    int threads;                                          // see read()
    static DadaRing *connect(unsigned key, int mode, std::string &why);
    DadaRing();
    ~DadaRing();
    int64_t next_header(char *dst) override;
    int64_t read(void *buf, size_t n) override;
    void finish_observation() override;
    bool write_header(const std::string &hdr) override;
    bool write(const void *buf, size_t n) override;
    void end_of_data() override;
};

}   // namespace host

#endif
