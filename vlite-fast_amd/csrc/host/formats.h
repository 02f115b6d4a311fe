// What process_baseband reads and writes besides samples, as pure functions: VDIF frame headers and their times, the
// ASCII ring headers, the SIGPROC header, the file names (--dump-headers needs nothing else of the program).
#ifndef PB_HOST_FORMATS_H
#define PB_HOST_FORMATS_H

#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "pb_hip.h"

namespace host {

constexpr size_t VD_FRM = PB_VDIF_FRAME, VD_DAT = PB_VDIF_DATA;
constexpr size_t DADA_HDR = 4096;

// ---- VDIF header (32 bytes, little-endian words; same decoding as the reference's VDIFHeader,
// analysis/baseband.py:19-28) ----
struct VH {
    int64_t second;
    int epoch, frame, threadid, thread, station;
    bool invalid;
};
VH unpack_header(const uint8_t *p);
int64_t vdif_to_unixepoch(const VH &h);                 // src/utils.c:498-514
int64_t frame_mjd(const VH &h);
int64_t frame_mjd_sec(const VH &h);
double frame_dmjd(const VH &h, double framepersec);     // getVDIFFrameDMJD (src/process_baseband.cu:241)

// ---- ASCII ring headers: "KEY value" lines; the first token after each key, like ascii_header_get ----
typedef std::vector<std::pair<std::string, std::string>> KV;
std::map<std::string, std::string> ascii_header_parse(const char *raw, size_t n);
std::string ascii_header_format(const KV &kv);
std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
std::string get(const std::map<std::string, std::string> &m, const char *k, const char *dflt = "");

// ---- SIGPROC header (src/util.c:51-82 send_string / send_int / send_double; keys and values
// src/process_baseband.cu:226-270) ----
std::string sigproc_header(int station, double ra, double dec, const std::string &name, double dmjd, int npol, int nbit);
// get_fbfile / get_cofbfile (:272-304): CHANMIN < 2411 gives the `_muos` infix, the coadd variant is station 99
void fb_names(int64_t unix_s, int station, const std::string &datadir, std::string &fb, std::string &fb_kur,
              std::string &co, std::string &co_kur);
// write_psrdada_header (:136-201), in its order
KV psrdada_out_header(const std::map<std::string, std::string> &in, int npol, int nbit, const std::string &fb_file,
                      int64_t unix_s, int64_t mjd, int64_t mjd_sec);

}   // namespace host

#endif
