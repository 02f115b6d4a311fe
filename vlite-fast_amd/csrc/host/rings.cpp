#include "rings.h"

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <thread>

#include "formats.h"

namespace host {

FileRing::~FileRing()
{
    if (fd >= 0) close(fd);
}
int64_t FileRing::next_header(char *dst)
{
    if (fd >= 0) close(fd);
    fd = -1;
    if (++i >= (int)paths.size()) return 0;
    fd = open(paths[i].c_str(), O_RDONLY);
    if (fd < 0) return -1;
    struct stat st;
    regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
    return read(dst, DADA_HDR) == (int64_t)DADA_HDR ? (int64_t)DADA_HDR : -1;
}
int64_t FileRing::read(void *buf, size_t n)
{
    const size_t CH = 8u << 20;
    if (regular && n >= 2 * CH) {
        const off_t pos = lseek(fd, 0, SEEK_CUR);
        struct stat st;
        fstat(fd, &st);
        const size_t want = std::min<size_t>(n, st.st_size > pos ? (size_t)(st.st_size - pos) : 0);
        if (want >= 2 * CH) {
            const int nth = (int)std::min<size_t>(8, std::max(1u, std::thread::hardware_concurrency()));
            std::vector<std::thread> th;
            std::vector<size_t> got(nth, 0), span(nth, 0);
            const size_t per = ((want / nth) + 4095) & ~(size_t)4095;
            for (int t = 0; t < nth; ++t)
                th.emplace_back([&, t]() {
                    size_t a = std::min(want, (size_t)t * per), b = std::min(want, a + per);
                    span[t] = b - a;
                    while (a < b) {
                        ssize_t r = pread(fd, (char *)buf + a, b - a, pos + (off_t)a);
                        if (r < 0 && errno == EINTR) continue;
                        if (r <= 0) break;
                        a += (size_t)r;
                        got[t] += (size_t)r;
                    }
                });
            for (int t = 0; t < nth; ++t) th[t].join();
            // only the CONTIGUOUS prefix counts: a piece that came up short (file truncated under us, I/O
            // error) ends the read there, so that the frame stream is never assembled around a hole
            size_t total = 0;
            for (int t = 0; t < nth; ++t) {
                total += got[t];
                if (got[t] < span[t]) break;
            }
            lseek(fd, pos + (off_t)total, SEEK_SET);
            return (int64_t)total;
        }
    }
    size_t got = 0;
    while (got < n) {
        ssize_t r = ::read(fd, (char *)buf + got, n - got);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) break;
        got += (size_t)r;
    }
    return (int64_t)got;
}

FileSink::~FileSink()
{
    if (fp) fclose(fp);
}
bool FileSink::write_header(const std::string &hdr) { return fp && fwrite(hdr.data(), 1, hdr.size(), fp) == hdr.size(); }
bool FileSink::write(const void *buf, size_t n) { return fp && fwrite(buf, 1, n, fp) == n; }
void FileSink::end_of_data()
{
    if (fp) fflush(fp);
}

// psrdada rings through the flat C shim of include/pb_dada.h, bound at run time
static struct DadaApi {
    void *lib = nullptr;
    decltype(&pb_dada_open) open = nullptr;
    decltype(&pb_dada_next_header) next_header = nullptr;
    decltype(&pb_dada_read) read = nullptr;
    decltype(&pb_dada_read_mt) read_mt = nullptr;
    decltype(&pb_dada_end_read) end_read = nullptr;
    decltype(&pb_dada_write_header) write_header = nullptr;
    decltype(&pb_dada_write) write = nullptr;
    decltype(&pb_dada_end_write) end_write = nullptr;
    decltype(&pb_dada_close) close = nullptr;
    bool load(std::string &why)
    {
        if (lib) return true;
        std::vector<std::string> cand;
        if (const char *e = getenv("PB_DADA_LIB")) cand.push_back(e);
        char self[4096];
        ssize_t n = readlink("/proc/self/exe", self, sizeof self - 1);
        if (n > 0) {
            self[n] = 0;
            std::string d(self);
            cand.push_back(d.substr(0, d.rfind('/')) + "/libpb_dada.so");
        }
        cand.push_back("libpb_dada.so");
        for (auto &c : cand)
            if ((lib = dlopen(c.c_str(), RTLD_NOW))) break;
        if (!lib) {
            const char *e = dlerror();   // (a second call returns NULL)
            why = "psrdada rings need the shim library (make -C vlite-fast_amd/csrc dada PSRDADA=<prefix>; or "
                  "PB_DADA_LIB=<path to libpb_dada.so>): " + std::string(e ? e : "not found");
            return false;
        }
#define PB_SYM(name) name = (decltype(name))dlsym(lib, "pb_dada_" #name)
        PB_SYM(open); PB_SYM(next_header); PB_SYM(read); PB_SYM(read_mt); PB_SYM(end_read);
        PB_SYM(write_header); PB_SYM(write); PB_SYM(end_write); PB_SYM(close);
#undef PB_SYM
        if (!open || !next_header || !read || !read_mt || !end_read || !write_header || !write || !end_write || !close) {
            why = "the shim library lacks symbols of include/pb_dada.h";
            return false;
        }
        return true;
    }
} g_dada;

DadaRing *DadaRing::connect(unsigned key, int mode, std::string &why)
{
    if (!g_dada.load(why)) return nullptr;
    char err[512] = "";
    pb_dada *d = g_dada.open(key, mode, err, sizeof err);
    if (!d) {
        why = err;
        return nullptr;
    }
    DadaRing *r = new DadaRing;
    r->d = d;
    return r;
}
// Data reads: block level by default (the ring's filled buffers copied out by PB_DADA_THREADS threads, 8 unless
// set; one ipcio_read memcpy thread moves ~9 GB/s = 28 ms per second of data), the reference's ipcio_read for
// every read with PB_DADA_THREADS=1.  Decided once: psrdada does not let the two alternate on a ring.
DadaRing::DadaRing() : threads(getenv("PB_DADA_THREADS") ? std::max(1, atoi(getenv("PB_DADA_THREADS"))) : 8) {}
DadaRing::~DadaRing()
{
    if (d) g_dada.close(d);
}
int64_t DadaRing::next_header(char *dst) { return g_dada.next_header(d, dst); }
int64_t DadaRing::read(void *buf, size_t n)
{
    size_t got = 0;
    while (got < n) {
        int64_t r = threads > 1 ? g_dada.read_mt(d, (char *)buf + got, n - got, threads)
                                : g_dada.read(d, (char *)buf + got, n - got);
        if (r <= 0) break;
        got += (size_t)r;
    }
    return (int64_t)got;
}
void DadaRing::finish_observation() { g_dada.end_read(d); }
bool DadaRing::write_header(const std::string &hdr)
{
    header_posted = true;
    return g_dada.write_header(d, hdr.data()) == 0;
}
bool DadaRing::write(const void *buf, size_t n) { return g_dada.write(d, buf, n) == (int64_t)n; }
void DadaRing::end_of_data()
{
    if (header_posted) g_dada.end_write(d);
    header_posted = false;
}

}   // namespace host
