// process_baseband: the reference's executable as a native host program above the C ABI of include/pb_hip.h
// (no HIP headers here: device work, streams and page-locked memory all sit behind libpb_hip.so).
//
// Drop-in under scripts/start_process:50 of the reference:
//     process_baseband -k <bb_key> -K <fb_key> -w <0|1|2> -b <2|4|8> -g <gpu> -o -C <coadd_key>
// (+ -P 1|2  -r 0|1|2  -i  -s  -t; the legacy `-p N` of scripts/baseband_test:26 is accepted and ignored, as
// the reference's getopt string silently does).  Mirrors /root/reference/src/process_baseband.cu main():
//   :358-470   option parsing (keys are hexadecimal: `-k 40` means 0x40)
//   :784-1000  per-observation set-up: ring header, first frame, file names, SIGPROC / psrdada headers
//   :1015-1496 per-second loop: frames are placed by their own headers, a second is dispatched only once a
//              frame of the NEXT second has been seen, so the last second of an observation is dropped
//   :1108-1458 ten 100-ms segments per second -> ONE pb_submit_vdif_at + pb_process call
//   :1416-1441 coadd ring (one write per segment), .fil / _kur.fil;  :1482-1494 output ring (10 s, then 1 s)
//   :1538-1556 the PROFILE lines (-t)
// Same behaviour, log lines and bytes as vlite-fast_amd/process_baseband.py (tests compare the two: on the GPU
// tests/test_native_exe.py; without one tests/test_native_host_cpu.py, which links these sources against a stand-in
// for the library and runs the loop under sanitizers).
// What lives where (host/ beside this file; the Makefile's HOST_SRCS is the list):
//   host/formats.{h,cpp}        VDIF headers and times, ASCII ring headers, SIGPROC header, file names: pure functions
//   host/rings.{h,cpp}          dump files, sink files, psrdada rings through the shim
//   host/log.h                  the log
//   host/second_reader.{h,cpp}  SecondReader: fill / seal / advance, as the Python host's class of that name
//   this file                   options, the -w 1 source list, the control socket, and run(): process set-up
//                               (Host), then per observation begin_observation, ObsOutput (files, rings' streams,
//                               the 10-s buffer; collect) and observe (the per-second loop)
// Extensions: --replay FILE.. (dump files instead of ring -k), --out-sink / --co-sink FILE (instead of rings
// -K / -C), --datadir, --logdir, --no-control, --fft-backend lds|hipfft, --taps 1|4, --rows-per-seg N,
// --dump-headers (print the two headers of the first observation as hex and exit; no GPU needed),
// --control-port N (test hook: commands on UDP 127.0.0.1:N instead of the multicast group).
// Rings: the psrdada shim of include/pb_dada.h is loaded at run time (dlopen of $PB_DADA_LIB or
// libpb_dada.so beside this program), so the program builds and runs replays where psrdada is absent.
#include <arpa/inet.h>
#include <fcntl.h>
#include <getopt.h>
#include <netinet/in.h>
#include <sys/socket.h>
#include <sys/time.h>
#include <unistd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "host/formats.h"
#include "host/log.h"
#include "host/rings.h"
#include "host/second_reader.h"
#include "pb_dada.h"
#include "pb_hip.h"

namespace {

using namespace host;

constexpr int SEG_PER_SEC = 10;
constexpr int nsets = 2;                // buffer sets of the handle: second k is queued while second k-1 is collected
const char *MC_GROUP = "224.3.29.71";   // src/multicast.h:14
constexpr int MC_READER_PORT = 20000;   // src/multicast.h:16
constexpr char CMD_QUIT = 'Q';          // src/def.h:6
const char *DEF_LOGDIR = "/home/vlite-master/mtk/logs";   // src/def.h:26
const char *DEF_DATADIR = "/mnt/ssd/fildata";             // src/def.h:28
// `-w 1` writes only for the sources a site file lists (site policy, src/util.c:91-152 of the reference; out of the
// hot path's scope, so it is data, not code): $PB_WRITE_ALLOW, else <dir of this program>/../site/write_allow.txt,
// lines `name <substring of NAME>` / `dataid <substring of DATAID>`; no file: -w 1 writes nothing
struct WriteAllow {
    std::vector<std::string> names, ids;
    std::vector<std::pair<double, double>> coords;     // `coords <ra> <dec>` [rad], check_coords (src/util.c:136-152)
    std::string path;
    bool loaded = false, ok = false;
    void load()
    {
        if (loaded) return;
        loaded = true;
        if (const char *e = getenv("PB_WRITE_ALLOW")) path = e;
        else {
            char self[4096];
            ssize_t n = readlink("/proc/self/exe", self, sizeof self - 1);
            if (n <= 0) return;
            self[n] = 0;
            std::string d(self);
            path = d.substr(0, d.rfind('/')) + "/../site/write_allow.txt";
        }
        FILE *f = fopen(path.c_str(), "r");
        if (!f) return;
        ok = true;
        char line[512];
        while (fgets(line, sizeof line, f)) {
            if (char *h = strchr(line, '#')) *h = 0;
            char key[32], val[256];
            double ra, de;
            if (sscanf(line, "%31s %lf %lf", key, &ra, &de) == 3 && !strcmp(key, "coords")) { coords.push_back({ra, de}); continue; }
            if (sscanf(line, "%31s %255s", key, val) != 2) continue;
            if (!strcmp(key, "name")) names.push_back(val);
            else if (!strcmp(key, "dataid")) ids.push_back(val);
        }
        fclose(f);
    }
} g_allow;

double now()
{
    timeval tv;
    gettimeofday(&tv, nullptr);
    return tv.tv_sec + 1e-6 * tv.tv_usec;
}

struct Args {
    unsigned key_in = 0x40, key_out = 0, key_co = 0;
    bool stdout_output = false, inject_frb = false, single_pass = false, profile_pass = false, no_control = false;
    bool dump_headers = false;
    bool coherence = false;   // --coherence (with -P 2): AA, BB, CR, CI
    int write_fb = 2, nbit = 2, npol = 1, rfi_mode = 2, gpu_id = 0, taps = 1, rows_per_seg = 1024;
    int fft_backend = PB_FFT_LDS, control_port = MC_READER_PORT;
    std::vector<std::string> replay;
    std::string datadir = DEF_DATADIR, logdir = DEF_LOGDIR, out_sink, co_sink;
};

// ---- control socket: non-blocking membership of 224.3.29.71:20000 (src/utils.c:619, process_baseband.cu:764) ----
// port != MC_READER_PORT (test hook --control-port): a plain UDP socket on 127.0.0.1, no multicast group
int open_control_socket(int port)
{
    int s = socket(AF_INET, SOCK_DGRAM, IPPROTO_UDP);
    if (s < 0) return -1;
    int one = 1;
    setsockopt(s, SOL_SOCKET, SO_REUSEADDR, &one, sizeof one);
    sockaddr_in a;
    memset(&a, 0, sizeof a);
    a.sin_family = AF_INET;
    a.sin_port = htons((uint16_t)port);
    a.sin_addr.s_addr = htonl(port == MC_READER_PORT ? INADDR_ANY : INADDR_LOOPBACK);
    ip_mreq m;
    m.imr_multiaddr.s_addr = inet_addr(MC_GROUP);
    m.imr_interface.s_addr = htonl(INADDR_ANY);
    if (bind(s, (sockaddr *)&a, sizeof a) < 0 ||
        (port == MC_READER_PORT && setsockopt(s, IPPROTO_IP, IP_ADD_MEMBERSHIP, &m, sizeof m) < 0)) {
        close(s);
        return -1;
    }
    fcntl(s, F_SETFL, fcntl(s, F_GETFL, 0) | O_NONBLOCK);
    return s;
}
// src/utils.c:174-186: one non-blocking read of up to 32 bytes, any byte equal to cmd
bool test_for_cmd(int sock, char cmd)
{
    if (sock < 0) return false;
    char buf[32];
    ssize_t n = recv(sock, buf, sizeof buf, 0);
    for (ssize_t i = 0; i < n; ++i)
        if (buf[i] == cmd) return true;
    return false;
}

// src/process_baseband.cu:893-913: position, then NAME, then DATAID (check_coords / check_name / check_id)
bool source_allowed(const std::map<std::string, std::string> &hdr)
{
    const std::string name = get(hdr, "NAME"), id = get(hdr, "DATAID");
    g_allow.load();
    const double ra = atof(get(hdr, "RA").c_str()), dec = atof(get(hdr, "DEC").c_str());
    for (const auto &c : g_allow.coords) {
        const double dde = dec - c.second, dra = (ra - c.first) * cos(c.second);      // coord_dist, src/util.c:127-134
        if (sqrt(dde * dde + dra * dra) < 0.01) return true;
    }
    for (const std::string &n : g_allow.names)
        if (name.find(n) != std::string::npos) return true;
    for (const std::string &n : g_allow.ids)
        if (id.find(n) != std::string::npos) return true;
    return false;
}

void usage()
{
    puts("usage: process_baseband -k <key_in hex> -K <key_out hex> -C <key_co hex> -w <0|1|2> -b <2|4|8> -P <1|2>\n"
         "       -r <0|1|2> -g <gpu> [-o] [-i] [-s] [-t] [-m] [-p N]\n"
         "       [--replay FILE...] [--out-sink FILE] [--co-sink FILE] [--datadir DIR] [--logdir DIR] [--no-control]\n"
         "       [--fft-backend lds|hipfft] [--taps 1|4] [--rows-per-seg N] [--dump-headers] [--coherence]\n"
         "       process_baseband --check-source NAME DATAID RA DEC");
}

bool parse(int argc, char **argv, Args &a)
{
    enum { O_REPLAY = 1000, O_DATADIR, O_LOGDIR, O_OUTSINK, O_COSINK, O_NOCTL, O_FFT, O_TAPS, O_ROWS, O_DUMP, O_CTLPORT, O_COH };
    static option lo[] = {{"replay", required_argument, nullptr, O_REPLAY}, {"datadir", required_argument, nullptr, O_DATADIR},
                          {"logdir", required_argument, nullptr, O_LOGDIR},  {"out-sink", required_argument, nullptr, O_OUTSINK},
                          {"co-sink", required_argument, nullptr, O_COSINK}, {"no-control", no_argument, nullptr, O_NOCTL},
                          {"fft-backend", required_argument, nullptr, O_FFT}, {"taps", required_argument, nullptr, O_TAPS},
                          {"rows-per-seg", required_argument, nullptr, O_ROWS}, {"dump-headers", no_argument, nullptr, O_DUMP},
                          {"control-port", required_argument, nullptr, O_CTLPORT}, {"coherence", no_argument, nullptr, O_COH},
                          {nullptr, 0, nullptr, 0}};
    int c;
    while ((c = getopt_long(argc, argv, "hk:K:C:omiw:b:P:r:stg:p:", lo, nullptr)) != -1) {
        switch (c) {
        case 'h': usage(); exit(0);
        case 'k': a.key_in = (unsigned)strtoul(optarg, nullptr, 16); break;     // sscanf "%x" (:367-383)
        case 'K': a.key_out = (unsigned)strtoul(optarg, nullptr, 16); break;
        case 'C': a.key_co = (unsigned)strtoul(optarg, nullptr, 16); break;
        case 'o': a.stdout_output = true; break;
        case 'm': break;                                                         // accepted, no effect (:403-407)
        case 'i': a.inject_frb = true; break;
        case 'w': a.write_fb = atoi(optarg); break;
        case 'b': a.nbit = atoi(optarg); break;
        case 'P': a.npol = atoi(optarg); break;
        case 'r': a.rfi_mode = atoi(optarg); break;
        case 's': a.single_pass = true; break;
        case 't': a.profile_pass = true; break;
        case 'g': a.gpu_id = atoi(optarg); break;
        case 'p': break;                                                         // legacy, ignored
        case O_REPLAY:
            a.replay.push_back(optarg);
            while (optind < argc && argv[optind][0] != '-') a.replay.push_back(argv[optind++]);
            break;
        case O_DATADIR: a.datadir = optarg; break;
        case O_LOGDIR: a.logdir = optarg; break;
        case O_OUTSINK: a.out_sink = optarg; break;
        case O_COSINK: a.co_sink = optarg; break;
        case O_NOCTL: a.no_control = true; break;
        case O_FFT:
            if (!strcmp(optarg, "lds")) a.fft_backend = PB_FFT_LDS;
            else if (!strcmp(optarg, "hipfft")) a.fft_backend = PB_FFT_HIPFFT;
            else return false;
            break;
        case O_TAPS: a.taps = atoi(optarg); break;
        case O_ROWS: a.rows_per_seg = atoi(optarg); break;
        case O_DUMP: a.dump_headers = true; break;
        case O_CTLPORT: a.control_port = atoi(optarg); break;
        case O_COH: a.coherence = true; break;
        default: return false;
        }
    }
    if (a.nbit != 2 && a.nbit != 4 && a.nbit != 8) { fputs("Unsupported NBIT!\n", stderr); return false; }
    if (a.rfi_mode < 0 || a.rfi_mode > 2) { fputs("Unsupported RFI mode!\n", stderr); return false; }
    if (a.npol != 1 && a.npol != 2) { fputs("Unsupported npol!\n", stderr); return false; }
    if (a.coherence && a.npol != 2) { fputs("--coherence needs -P 2\n", stderr); return false; }
    if (a.rows_per_seg == 1024 && (a.gpu_id < 0 || a.gpu_id > 7)) { fputs("Unsupported GPU id!\n", stderr); return false; }
    return true;
}

void hex(const char *what, const std::string &s)
{
    printf("%s %zu ", what, s.size());
    for (unsigned char ch : s) printf("%02x", ch);
    putchar('\n');
}

// a failed pb_* call: the call as it is written, then the library's message (so the names at the call sites -- h,
// queued, k, nsets, block, current_sec ... -- are part of that log line); the caller leaves with status 1.
// PB_FAILED takes `log` and `h` from the scope it is used in.
bool pb_failed(Log &log, pb_handle *h, int rc, const char *call)
{
    if (rc == PB_OK) return false;
    log.line(true, "%s: %s", call, pb_last_error(h));
    return true;
}
#define PB_FAILED(call) pb_failed(log, h, (call), #call)

// What set-up makes and every observation uses.  The rings and the handle are plain owning pointers that only close(),
// on the normal path, releases: after a fatal error the program leaves with everything as it is, like the reference's
// exit(EXIT_FAILURE) -- unlocking a write ring would signal end of data to its reader, and pb_destroy after a HIP error
// would synchronise streams of a device that may be stuck.
struct Host {
    const Args &args;
    Log log;
    const size_t frames_per_sec;          // per thread; 25600 at R = 1024
    const size_t sec_bytes;               // 257 638 400 at R = 1024
    ReadRing *in_ring = nullptr;
    WriteRing *out_ring = nullptr, *co_ring = nullptr;
    pb_handle *h = nullptr;
    size_t trim = 0;
    int ctl = -1;
    std::vector<uint8_t *> blocks;        // page-locked staging for one second of frames
    explicit Host(const Args &a)
        : args(a), frames_per_sec((size_t)a.rows_per_seg * SEG_PER_SEC * 12500 / VD_DAT), sec_bytes(2 * frames_per_sec * VD_FRM)
    {
    }
    bool set_up();
    void close();
};

bool Host::set_up()
{
    log.open(args.logdir, args.stdout_output);
    std::string why;
    if (!args.replay.empty()) in_ring = new FileRing(args.replay);
    else if (!(in_ring = DadaRing::connect(args.key_in, PB_DADA_READ, why))) {
        log.line(true, "could not connect to input ring %x: %s", args.key_in, why.c_str());
        return false;
    }
    if (!args.dump_headers) {
        if (!args.out_sink.empty()) out_ring = new FileSink(args.out_sink);
        else if (args.key_out && !(out_ring = DadaRing::connect(args.key_out, PB_DADA_WRITE, why))) {
            log.line(true, "could not connect to output ring %x: %s", args.key_out, why.c_str());
            return false;
        }
        if (!args.co_sink.empty()) co_ring = new FileSink(args.co_sink);
        else if (args.key_co && !(co_ring = DadaRing::connect(args.key_co, PB_DADA_WRITE, why))) {
            log.line(true, "could not connect to coadd ring %x: %s", args.key_co, why.c_str());
            return false;
        }
    }
    pb_sizes sz;
    memset(&sz, 0, sizeof sz);
    if (!args.dump_headers) {
        pb_config cfg;
        pb_config_default(&cfg);
        cfg.device = args.gpu_id;
        cfg.nant = 1;
        cfg.nbit = args.nbit;
        cfg.npol = args.npol;
        cfg.rfi_mode = args.rfi_mode;
        cfg.taps = args.taps;
        cfg.fft_backend = args.fft_backend;
        cfg.rows_per_seg = args.rows_per_seg;
        cfg.max_seg = SEG_PER_SEC;
        cfg.inject_frb = args.inject_frb;
        cfg.nsets = nsets;
        cfg.coherence = args.coherence ? 1 : 0;
        if (pb_create(&cfg, &h) != PB_OK) {
            log.line(true, "pb_create: %s", pb_last_error(nullptr));
            return false;
        }
        pb_query(h, &sz);
    }
    trim = sz.code_bytes_per_seg;
    ctl = args.no_control ? -1 : open_control_socket(args.control_port);
    // One second of frames is assembled in page-locked memory (nsets + 1 buffers in turn: the H2D of second k is
    // known to be complete once its filterbank bytes have been fetched, which happens before buffer
    // k mod (nsets + 1) comes round again), read straight into place -- one copy from the ring.  Allocated at
    // start-up, as the reference allocates its host buffer (cudaMallocHost, :579): pinning 0.77 GB takes 0.15 s.
    if (h)
        for (int i = 0; i < nsets + 1; ++i) {
            uint8_t *b = (uint8_t *)pb_host_alloc(sec_bytes);
            if (!b) {
                log.line(true, "pb_host_alloc(%zu) failed", sec_bytes);
                return false;
            }
            blocks.push_back(b);
        }
    return true;
}

void Host::close()
{
    if (h) {
        pb_sync(h);
        for (uint8_t *b : blocks) pb_host_free(b);
        pb_destroy(h);
    }
    delete in_ring;
    delete out_ring;
    delete co_ring;
}

// what the ring header and the first frame say about an observation: names and headers of everything it will write
struct ObsStart {
    double t_obs;
    std::map<std::string, std::string> hdr;
    uint8_t first[VD_FRM];
    VH vh;
    std::string fb, fb_kur, cofb, cofb_kur, sp_hdr, out_hdr, co_hdr;
};

// -> 1: `obs` describes the next observation; 0: the input ring is closed; -1: fatal
int begin_observation(Host &host, ObsStart &obs)
{
    const Args &args = host.args;
    Log &log = host.log;
    pb_handle *h = host.h;
    log.line(false, "Waiting for DADA header.");
    std::vector<char> raw_hdr(DADA_HDR);
    const int64_t hn = host.in_ring->next_header(raw_hdr.data());
    if (hn <= 0) {
        log.line(false, "Input ring closed.  Exiting.");
        return 0;
    }
    obs.t_obs = now();
    obs.hdr = ascii_header_parse(raw_hdr.data(), DADA_HDR);
    const auto &hdr = obs.hdr;
    log.line(false, "Beginning new observation.");
    if (h && PB_FAILED(pb_reset_history(h, 0))) return -1;   // taps=4: the FIR window does not span observations
    if (host.in_ring->read(obs.first, VD_FRM) != (int64_t)VD_FRM) {
        log.line(true, "Problem reading first bloody frame!  Bailing.");
        return -1;
    }
    const VH vh = obs.vh = unpack_header(obs.first);
    if (vh.frame != 0 && vh.thread != 0) {          // sic: `&&` in the reference (:845)
        log.line(true, "Incoming data were not aligned!");
        return -1;
    }
    const int station = atoi(get(hdr, "STATIONID", "0").c_str());
    const int64_t t_unix = vdif_to_unixepoch(vh);
    fb_names(t_unix, station, args.datadir, obs.fb, obs.fb_kur, obs.cofb, obs.cofb_kur);
    const std::string heimdall_file = args.rfi_mode ? obs.fb_kur : obs.fb, coheimdall_file = args.rfi_mode ? obs.cofb_kur : obs.cofb;
    const int64_t mjd = frame_mjd(vh), mjd_sec = frame_mjd_sec(vh);
    const int out_npol = args.coherence ? 4 : args.npol;   // nifs / NPOL: AA, BB, CR, CI with --coherence
    obs.sp_hdr = sigproc_header(station, atof(get(hdr, "RA", "0").c_str()), atof(get(hdr, "DEC", "0").c_str()),
                                get(hdr, "NAME"), frame_dmjd(vh, (double)host.frames_per_sec), out_npol, args.nbit);
    obs.out_hdr = ascii_header_format(psrdada_out_header(hdr, out_npol, args.nbit, heimdall_file, t_unix, mjd, mjd_sec));
    obs.co_hdr = ascii_header_format(psrdada_out_header(hdr, out_npol, args.nbit, coheimdall_file, t_unix, mjd, mjd_sec));
    return 1;
}

void dump_headers(const ObsStart &obs)
{
    hex("sigproc", obs.sp_hdr);
    hex("out", obs.out_hdr);
    hex("co", obs.co_hdr);
    printf("files %s %s %s %s\n", obs.fb.c_str(), obs.fb_kur.c_str(), obs.cofb.c_str(), obs.cofb_kur.c_str());
}

// What one observation writes to -- its files and the rings -- with the 10-s buffer of the stream heimdall gets
// (:691-697) and the count of the seconds written.
struct ObsOutput {
    const Args &args;
    Log &log;
    pb_handle *h;
    WriteRing *out_ring, *co_ring;
    const size_t trim;
    std::string fb, fb_kur;               // the files' names after the -w decision
    FILE *fb_fp = nullptr, *fb_kur_fp = nullptr;
    long integrated_sec = 0;
    size_t fb_bytes = 0;
    double t_rt = 0, prof_write = 0;
    std::vector<std::vector<uint8_t>> out_buf;
    explicit ObsOutput(Host &host)
        : args(host.args), log(host.log), h(host.h), out_ring(host.out_ring), co_ring(host.co_ring), trim(host.trim)
    {
    }
    bool open(const ObsStart &obs);
    int ring_write(WriteRing *r, const void *buf, size_t n);
    int collect(long k);
};

// the -w decision, the files, and the headers of files and rings; false: fatal
bool ObsOutput::open(const ObsStart &obs)
{
    const auto &hdr = obs.hdr;
    fb = obs.fb;
    fb_kur = obs.fb_kur;
    bool write_to_null = args.write_fb == 0;
    if (args.write_fb == 1) {
        g_allow.load();
        if (g_allow.ok)
            log.line(false, "Source list for -w 1: %s (%zu names, %zu dataids, %zu positions).", g_allow.path.c_str(),
                     g_allow.names.size(), g_allow.ids.size(), g_allow.coords.size());
        else
            log.line(true, "Source list for -w 1 not usable (%s): no source will be recorded.", g_allow.path.c_str());
        if (source_allowed(hdr))
            log.line(false, "Source %s matches target list, recording filterbank data.", get(hdr, "NAME").c_str());
        else {
            write_to_null = true;
            log.line(false, "Source %s not on target list, disabling filterbank data.", get(hdr, "NAME").c_str());
        }
    }
    if (write_to_null) {
        log.line(false, "Filterbank output disabled.  Would have written to %s.", fb.c_str());
        fb = fb_kur = "/dev/null";
    }
    if (args.rfi_mode == 0 || args.rfi_mode == 2) {
        fb_fp = fopen(fb.c_str(), "wb");
        log.line(false, "Writing no-RFI-excision filterbanks to %s.", fb.c_str());
    } else {
        fb_fp = fopen(fb_kur.c_str(), "wb");
        log.line(false, "Writing RFI-excision filterbanks to %s.", fb_kur.c_str());
    }
    if (args.rfi_mode == 2) {
        fb_kur_fp = fopen(fb_kur.c_str(), "wb");
        log.line(false, "Writing RFI-excision filterbanks to %s.", fb_kur.c_str());
    }
    if (!fb_fp || (args.rfi_mode == 2 && !fb_kur_fp)) {
        log.line(true, "could not open the filterbank files in %s", args.datadir.c_str());
        return false;
    }
    if ((out_ring && !out_ring->write_header(obs.out_hdr)) || (co_ring && !co_ring->write_header(obs.co_hdr))) {
        log.line(true, "Could not write the psrdada output header.");
        return false;
    }
    fwrite(obs.sp_hdr.data(), 1, obs.sp_hdr.size(), fb_fp);
    if (fb_kur_fp) fwrite(obs.sp_hdr.data(), 1, obs.sp_hdr.size(), fb_kur_fp);
    return true;
}

// a failed ring write is fail-stop, like check_ipcio_write (src/process_baseband.cu:322-332)
int ObsOutput::ring_write(WriteRing *r, const void *buf, size_t n)
{
    if (r->write(buf, n)) return 0;
    fprintf(stderr, "failed ipcio write\n");
    log.line(true, "Tried to write %lu bytes to psrdada buffer but the write came up short.", (unsigned long)n);
    return 1;
}

// filterbank bytes of queued second k -> files and rings (:1364-1441, :1482-1494)
int ObsOutput::collect(long k)
{
    const double t0 = now();
    if (PB_FAILED(pb_select_set(h, (int)(k % nsets)))) return 1;
    const uint8_t *raw = nullptr, *kur = nullptr;
    if (args.rfi_mode != 1 && PB_FAILED(pb_fetch_ptr(h, 0, 0, &raw))) return 1;
    if (args.rfi_mode != 0 && PB_FAILED(pb_fetch_ptr(h, 0, 1, &kur))) return 1;
    const uint8_t *main_codes = args.rfi_mode != 1 ? raw : kur, *heim_codes = args.rfi_mode != 0 ? kur : raw;
    for (int iseg = 0; iseg < SEG_PER_SEC; ++iseg) {
        if (co_ring && ring_write(co_ring, heim_codes + iseg * trim, trim)) return 1;
        fwrite(main_codes + iseg * trim, 1, trim, fb_fp);
        if (fb_kur_fp) fwrite(kur + iseg * trim, 1, trim, fb_kur_fp);
        fb_bytes += trim;
    }
    out_buf.emplace_back(heim_codes, heim_codes + SEG_PER_SEC * trim);
    ++integrated_sec;
    if (integrated_sec % 10 == 0) {
        const double lag = (now() - t_rt) - 10.0 * (args.rows_per_seg / 1024.0);
        if (lag > 0.5) log.line(true, "Measured time exceeding integrated time: lag %.2f s", lag);
        t_rt = now();
    }
    if (integrated_sec >= 10 && out_ring) {
        if (integrated_sec == 10) {                                        // the full 10-s buffer, one write
            std::vector<uint8_t> all;
            for (auto &b : out_buf) all.insert(all.end(), b.begin(), b.end());
            if (ring_write(out_ring, all.data(), all.size())) return 1;
        } else if (ring_write(out_ring, out_buf.back().data(), out_buf.back().size()))  // then 1 s at a time
            return 1;
    }
    if (out_buf.size() > 10) out_buf.erase(out_buf.begin());
    prof_write += now() - t0;
    return 0;
}

// the normal end of an observation: end of data on the rings, files closed, the closing log lines
void finish_observation(Host &host, const ObsStart &obs, ObsOutput &out, double prof_read, double prof_todev)
{
    const Args &args = host.args;
    Log &log = host.log;
    pb_handle *h = host.h;
    if (out.out_ring) out.out_ring->end_of_data();
    if (out.co_ring) out.co_ring->end_of_data();
    host.in_ring->finish_observation();
    fclose(out.fb_fp);
    if (out.fb_kur_fp) fclose(out.fb_kur_fp);
    const double tsamp = 12500.0 / 128e6 * 8;
    const size_t nsamp = out.fb_bytes * (8 / args.nbit) / 4096;
    log.line(false, "Wrote %.2f MB (%.2f s) to %s", out.fb_bytes * 1e-6, nsamp * tsamp, out.fb.c_str());
    log.line(false, "Proc Time...%.3f", now() - obs.t_obs);
    if (args.profile_pass) {
        // the reference's PROFILE block (:1538-1556).  Its kernels are fused here: "Convert" lives in the
        // kurtosis and channeliser kernels, "FFT" is the channeliser (unpack + FFT + detect), and normalise /
        // pscrunch / tscrunch / digitise are one kernel, reported under "Normalize".
        pb_profile(h, 0);
        pb_timers tm;
        pb_get_timers(h, &tm, 1);
        log.line(false, "Read Time...%.3f", prof_read);
        log.line(false, "Copy To Dev.%.3f", prof_todev);
        log.line(false, "Kurtosis....%.3f", tm.ms[PB_ST_KURTOSIS] * 1e-3);
        log.line(false, "FFT.........%.3f", (tm.ms[PB_ST_CHANNELIZE] + tm.ms[PB_ST_FFT] + tm.ms[PB_ST_INJECT]) * 1e-3);
        log.line(false, "Normalize...%.3f", tm.ms[PB_ST_DETECT] * 1e-3);
        log.line(false, "Write.......%.3f", out.prof_write);
    }
}

// One observation.  Its seconds are assembled by a SecondReader (host/second_reader.h) and pipelined over the handle's
// buffer sets: second k is queued (H2D + kernels) before the output of second k-1 is collected.  A major skip and
// CMD_QUIT end it, and the run, in order (`quit`, `exit_status`); false: fatal, nothing has been closed.
bool observe(Host &host, const ObsStart &obs, bool &quit, int &exit_status)
{
    const Args &args = host.args;
    Log &log = host.log;
    pb_handle *h = host.h;
    const size_t sec_bytes = host.sec_bytes;
    ObsOutput out(host);
    if (!out.open(obs)) return false;
    SecondReader reader(host.in_ring, obs.first, sec_bytes, log);
    log.line(false, "Starting sec=%lld, thread=%d", (long long)reader.current_sec, obs.vh.thread);
    long queued = 0;
    out.t_rt = now();
    double prof_read = 0, prof_todev = 0;
    if (args.profile_pass) {
        pb_timers tm;
        pb_get_timers(h, &tm, 1);
        pb_profile(h, 1);
    }
    while (true) {
        double t0 = now();
        uint8_t *block = host.blocks[queued % host.blocks.size()];
        size_t have;
        VH nh;
        const bool more = reader.fill(block, have, nh);
        const int64_t current_sec = reader.current_sec;
        prof_read += now() - t0;
        if (!more) break;              // end of data: the last (partial or whole) second is dropped
        if (nh.second - current_sec > 1) {
            log.line(true, "Major data skip!  (%lld vs. %lld; thread = %d) Aborting this observation.",
                     (long long)nh.second, (long long)current_sec, nh.thread);
            exit_status = 1;
            quit = true;
            break;
        }
        if (test_for_cmd(host.ctl, CMD_QUIT)) {
            log.line(false, "Received CMD_QUIT, indicating data taking is ceasing.  Exiting.");
            quit = true;
            break;
        }
        reader.seal(block, have);
        const int inject_now = (args.inject_frb && current_sec % 60 == 0) ? 1 : 0;
        if (inject_now) log.line(false, "Injecting an FRB with integrated = %.2f!!!.", (double)queued);
        t0 = now();
        if (PB_FAILED(pb_select_set(h, (int)(queued % nsets)))) return false;
        if (PB_FAILED(pb_submit_vdif_at(h, 0, 0, block, sec_bytes, current_sec, 0))) return false;
        if (PB_FAILED(pb_process(h, SEG_PER_SEC, inject_now))) return false;
        prof_todev += now() - t0;
        ++queued;
        if (queued - out.integrated_sec >= nsets)
            if (out.collect(out.integrated_sec)) return false;   // the oldest queued second, while the newest computes
        reader.advance();
    }
    while (out.integrated_sec < queued)
        if (out.collect(out.integrated_sec)) return false;
    finish_observation(host, obs, out, prof_read, prof_todev);
    return true;
}

int run(const Args &args)
{
    Host host(args);
    if (!host.set_up()) return 1;
    int exit_status = 0;
    bool quit = false;
    while (!quit) {
        if (test_for_cmd(host.ctl, CMD_QUIT)) break;
        ObsStart obs;
        const int began = begin_observation(host, obs);
        if (began < 0) return 1;
        if (began == 0) break;
        if (args.dump_headers) {
            dump_headers(obs);
            return 0;
        }
        if (!observe(host, obs, quit, exit_status)) return 1;
        if (args.profile_pass || args.single_pass) break;
    }
    host.close();
    return exit_status;
}

}   // namespace

int main(int argc, char **argv)
{
    // --check-source NAME DATAID RA DEC: the -w 1 decision for one header (prints 1 or 0; no GPU, no rings) -- what
    // the reference's check_coords / check_name / check_id answer (tests/test_ref_util.py compares)
    if (argc == 6 && !strcmp(argv[1], "--check-source")) {
        std::map<std::string, std::string> hdr{{"NAME", argv[2]}, {"DATAID", argv[3]}, {"RA", argv[4]}, {"DEC", argv[5]}};
        printf("%d\n", source_allowed(hdr) ? 1 : 0);
        return 0;
    }
    Args args;
    if (!parse(argc, argv, args)) {
        usage();
        return 1;
    }
    return run(args);
}
