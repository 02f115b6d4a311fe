#include "formats.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>

namespace host {

VH unpack_header(const uint8_t *p)
{
    uint32_t w[4];
    memcpy(w, p, 16);
    VH h;
    h.second = w[0] & 0x3FFFFFFF;
    h.invalid = (w[0] >> 31) != 0;
    h.epoch = (int)((w[1] >> 24) & 0x3F);
    h.frame = (int)(w[1] & 0xFFFFFF);
    h.station = (int)(w[3] & 0xFFFF);
    h.threadid = (int)((w[3] >> 16) & 0x3FF);
    h.thread = h.threadid != 0;
    return h;
}
// Unix time of the start of a VDIF reference epoch (half-years since 2000-01-01)
static int64_t epoch_unix(int epoch)
{
    tm g;
    memset(&g, 0, sizeof g);
    g.tm_year = 100 + epoch / 2;
    g.tm_mon = 6 * (epoch % 2);
    g.tm_mday = 1;
    return (int64_t)timegm(&g);
}
int64_t vdif_to_unixepoch(const VH &h) { return epoch_unix(h.epoch) + h.second; }
int64_t frame_mjd(const VH &h) { return 40587 + (epoch_unix(h.epoch) + h.second) / 86400; }
int64_t frame_mjd_sec(const VH &h) { return (epoch_unix(h.epoch) + h.second) % 86400; }
double frame_dmjd(const VH &h, double framepersec)
{
    return (double)frame_mjd(h) + ((double)frame_mjd_sec(h) + (double)h.frame / framepersec) / 86400.0;
}

std::map<std::string, std::string> ascii_header_parse(const char *raw, size_t n)
{
    std::map<std::string, std::string> out;
    std::string txt(raw, strnlen(raw, n));
    size_t pos = 0;
    while (pos < txt.size()) {
        size_t e = txt.find('\n', pos);
        if (e == std::string::npos) e = txt.size();
        std::string line = txt.substr(pos, e - pos);
        pos = e + 1;
        char k[256], v[1024];
        if (sscanf(line.c_str(), "%255s %1023s", k, v) == 2 && !out.count(k)) out[k] = v;
    }
    return out;
}
std::string ascii_header_format(const KV &kv)
{
    std::string txt;
    char line[2048];
    for (auto &p : kv) {
        snprintf(line, sizeof line, "%-19s %s\n", p.first.c_str(), p.second.c_str());
        txt += line;
    }
    txt.resize(DADA_HDR, '\0');
    return txt;
}
std::string fmt(const char *f, ...)
{
    char b[1024];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof b, f, ap);
    va_end(ap);
    return b;
}
std::string get(const std::map<std::string, std::string> &m, const char *k, const char *dflt)
{
    auto it = m.find(k);
    return it == m.end() ? dflt : it->second;
}

static void send_string(std::string &o, const std::string &s)
{
    int32_t n = (int32_t)s.size();
    o.append((const char *)&n, 4);
    o += s;
}
static void send_int(std::string &o, const char *name, int32_t v)
{
    send_string(o, name);
    o.append((const char *)&v, 4);
}
static void send_double(std::string &o, const char *name, double v)
{
    send_string(o, name);
    o.append((const char *)&v, 8);
}
// all intermediates are C floats, as the reference writes them (:249-259)
static float sigproc_angle(double x)
{
    float hh = (float)x;
    float mm = (hh - (int)hh) * 60;
    float ss = (mm - (int)mm) * 60;
    float out = (int)hh * 1e4 + (int)mm * 1e2 + ss;
    return out;
}
std::string sigproc_header(int station, double ra, double dec, const std::string &name, double dmjd, int npol, int nbit)
{
    const double chbw = -64. / PB_NCHAN;
    const double tsamp = (double)PB_NFFT / 128000000 * PB_NSCRUNCH;
    std::string o;
    send_string(o, "HEADER_START");
    send_string(o, "source_name");
    send_string(o, name);
    send_int(o, "barycentric", 0);
    send_int(o, "telescope_id", station);
    send_double(o, "src_raj", (double)sigproc_angle((180 / M_PI) * (24. / 360) * ra));
    send_double(o, "src_dej", (double)sigproc_angle((180 / M_PI) * fabs(dec)));   // sign dropped (:258)
    send_int(o, "data_type", 1);
    send_double(o, "fch1", 384 + (PB_CHANMIN - 0.5) * chbw);
    send_double(o, "foff", chbw);
    send_int(o, "nchans", PB_CHANMAX - PB_CHANMIN + 1);
    send_int(o, "nbits", nbit);
    send_double(o, "tstart", dmjd);
    send_double(o, "tsamp", tsamp);
    send_int(o, "nifs", npol);
    send_string(o, "HEADER_END");
    return o;
}
static std::string change_extension(const std::string &name, const char *oldext, const char *newext)
{
    size_t i = name.find(oldext);
    return i == std::string::npos ? name + newext : name.substr(0, i) + newext;
}
void fb_names(int64_t unix_s, int station, const std::string &datadir, std::string &fb, std::string &fb_kur,
              std::string &co, std::string &co_kur)
{
    char stamp[32];
    time_t t = (time_t)unix_s;
    tm g;
    gmtime_r(&t, &g);
    strftime(stamp, sizeof stamp, "%Y%m%d_%H%M%S", &g);
    const char *infix = PB_CHANMIN < 2411 ? "_muos" : "";
    fb = fmt("%s/%s%s_ea%02d.fil", datadir.c_str(), stamp, infix, station);
    co = fmt("%s/%s%s_ea%02d.fil", datadir.c_str(), stamp, infix, 99);
    fb_kur = change_extension(fb, ".fil", "_kur.fil");
    co_kur = change_extension(co, ".fil", "_kur.fil");
}
KV psrdada_out_header(const std::map<std::string, std::string> &in, int npol, int nbit, const std::string &fb_file,
                      int64_t unix_s, int64_t mjd, int64_t mjd_sec)
{
    const double chbw = -64. / PB_NCHAN;
    const double tsamp = (double)PB_NFFT / 128000000 * PB_NSCRUNCH * 1e6;
    const int nchan = PB_CHANMAX - PB_CHANMIN + 1;
    const int station = atoi(get(in, "STATIONID", "0").c_str());
    char utc[64];
    time_t t = (time_t)unix_s;
    tm g;
    gmtime_r(&t, &g);
    strftime(utc, sizeof utc, "%Y-%m-%d-%H:%M:%S", &g);
    KV h;
    h.emplace_back("STATIONID", fmt("%d", station));
    h.emplace_back("BEAM", fmt("%d", station));
    h.emplace_back("RA", fmt("%f", atof(get(in, "RA", "0").c_str())));
    h.emplace_back("DEC", fmt("%f", atof(get(in, "DEC", "0").c_str())));
    h.emplace_back("NAME", get(in, "NAME"));
    h.emplace_back("SCANSTART", fmt("%f", atof(get(in, "SCANSTART", "0").c_str())));
    h.emplace_back("NCHAN", fmt("%d", nchan));
    h.emplace_back("BANDWIDTH", fmt("%f", nchan * chbw));
    h.emplace_back("CFREQ", fmt("%f", 384. + 0.5 * (PB_CHANMIN + PB_CHANMAX - 1) * chbw));
    h.emplace_back("NPOL", fmt("%d", npol));
    h.emplace_back("NBIT", fmt("%d", nbit));
    h.emplace_back("TSAMP", fmt("%f", tsamp));
    h.emplace_back("UTC_START", utc);
    h.emplace_back("UNIXEPOCH", fmt("%f", (double)unix_s));
    h.emplace_back("VDIF_MJD", fmt("%lld", (long long)mjd));
    h.emplace_back("VDIF_SEC", fmt("%lld", (long long)mjd_sec));
    if (!fb_file.empty()) h.emplace_back("SIGPROC_FILE", fb_file);
    return h;
}

}   // namespace host
