// Internal declarations shared by the HIP translation units of libpb_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "pb_hip.h"
#include "pb_own.h"      // PB_LOCAL; DevBuf, PinBuf, Event, Stream, EventPool: what owns the handle's resources

// D'Agostino constants (src/pb_kernels.cu:3-12 of the reference), evaluated on the host
// with the reference's float/double mix and handed to the kernel by value.
struct DagConsts {
    double one_m_2_over_A;  // (1 - 2./A)
    double mu1;
    double Z1, Z2, Z3;
    // Where the score crosses DAG_THRESH, in terms of t = (1 - 2/A) / (1 + (kur - 3 - mu1) Z3) (the argument of the
    // cube root): the block is flagged for 0 < t <= t_lo_sure and for t >= t_hi_sure, not flagged for
    // t_lo_clear <= t <= t_hi_clear; in the (few floats wide, normally empty) bands between them the score itself is
    // evaluated.  Found on the device at pb_create by evaluating the score on every float around the crossings
    // (pb_tables.hip: find_dag_bands), so that a flag never needs the cube root and its eight Newton steps.
    float t_lo_sure, t_lo_clear, t_hi_clear, t_hi_sure;
};

struct FrbParams {
    const float *delays;  // [6251] or nullptr
    int since;            // nfft_since_frb for the first row of the launch
    float width;
    float amp;
};

// twiddle tables of the LDS FFT (all float2, built on the host in double); the radix-5/25/10 twiddles
// are compile-time literals (fft_consts.h)
struct PB_LOCAL FftTables {
    DevBuf<float2> tw2;    // [12 pairs (r, r+1)][25 k][2]   pass-2 twiddles exp(-2 pi i r k / 625), r = 1..24 (fft_lds.h: load_t2)
    DevBuf<float2> tw3;    // [625 j][10]    pass-3 twiddles exp(-2 pi i r j / 6250), r = 1..9, one pad
    DevBuf<float2> post;   // [6251]
    DevBuf<float2> postc;  // [4096] = post[2155..6250], its own 16-byte aligned allocation
    DevBuf<float> taps;    // [4][12500] FIR taps of the 4-tap window (always built)
    DevBuf<float2> taps_n; // the same interleaved for the PFB channeliser: [6250 n][4 taps] pairs (samples 2n, 2n+1)
};

// Scheduling choices read from the environment ONCE PER HANDLE, at pb_create (INTEGRATION.md lists them).  None of
// them changes a result: tests/test_gpu_schedules.py runs one full-size second through their combinations and
// requires identical bytes.  (Per handle, not per process: a test -- or a host -- can hold handles of several modes.)
struct PbSched {
    int overlap_detect;   // PB_OVERLAP_DETECT (1): detect + copy-out on streams of their own beside the next batch
    int kur_early;        // PB_KUR_EARLY (1): >= 3 sets: the kurtosis pass does not wait for the previous channeliser
    int detect_depth;     // PB_DETECT_DEPTH (0 = by configuration): 2 / 3 chunks in flight in detect's ring
    // read from the environment by the experiments build only (`make exp`); the shipped library uses the defaults
    int copy_dma;         // PB_COPY_DMA (0): 1 = hipMemcpyAsync instead of the copy-out kernel
    int copy_wgs;         // PB_COPY_WGS (8): workgroups of the copy-out kernel
    int det_cus;          // PB_DET_CUS (0): CU mask of the detect stream
    int det_prio;         // PB_DET_PRIO (1): detect's stream at the highest priority
};
PbSched pb_read_sched();

// Everything the handle takes from the HIP runtime is a member that owns it (pb_own.h), so `delete h` releases it all and
// pb_destroy keeps no list.  THE ORDER OF THE MEMBERS MATTERS in one respect: members are destroyed last to first, and
// the streams are declared before every buffer and event so that they outlive them.  (PB_LOCAL: neither the struct's
// own functions nor the templates over it become symbols of the library.)
struct PB_LOCAL pb_handle {
    pb_config cfg = {};
    PbSched sched = {};
    int R = 0;                 // rows per segment
    int S = 0;                 // max segments
    int A = 0;                 // antennas
    size_t seg_samples = 0;    // R * 12500
    size_t nblk_seg = 0;       // R * 25 (per pol)
    size_t trim = 0;           // code bytes per segment
    size_t ave_per_seg = 0;    // compact floats per segment
    size_t device_bytes = 0;
    std::string err;

    // --- streams: before the buffers and events (see above)
    Stream s_main;                   // the main stream while it is the handle's own (empty: pb_set_stream gave a caller's)
    hipStream_t stream = nullptr;    // the main stream -- s_main.s or the caller's -- or, inside a StreamScope, where launchers enqueue
    Stream s_det;                    // detect of the previous batch (pipelined mode); copy-out in the single-set mode
    Stream s_copy;                   // copy-out of the filterbank bytes in pipelined mode, so that it does not hold up the next detect
    Stream s_kur;                    // kurtosis of the next batch, beside detect of the previous one
    hipStream_t s_coadd = nullptr;   // stream of pb_coadd_local / pb_coadd_finish (nullptr: the main stream).  THE CALLER'S
                                     // (pb_set_coadd_stream): never destroyed here, nor waited for at pb_destroy
    Event ev_fftdone, ev_kur, ev_alldone;
    Event ev_hist;                   // taps = 4: the batch's last rows and flags have been kept for the next one

    DevBuf<uint8_t> d_vdif;          // staging for one raw 1-s block; grows with the block (its .cap is in bytes)
    DevBuf<int32_t> d_frame_idx;     // [2][frames] frame -> slot in block, -1 = missing (not counted in device_bytes)
    DevBuf<float> d_bp;              // [A][2 streams][2 pols][4096]
    DevBuf<float> d_frb_delays;      // [6251]
    DevBuf<uint8_t> d_hist_in;       // taps=4: [2 slots][A][2][3][PFB_HIST_STRIDE] last three rows of the previous batch
    int hist_rd = 0;                 // the slot the current batch reads (its history kernel fills the other)
    DevBuf<uint8_t> d_hist_flags;    // taps=4: [2][A][3][25] their kurtosis flags (1 = flagged / no data)
    DevBuf<uint8_t> d_hist_valid;    // taps=4: [2][A][3] slot holds data
    DevBuf<float> d_tapE;            // taps=4: [4][25] window energy per (tap, block) + total at [100]
    float frb_width = 0.f, frb_amp = 1.f;   // inject_frb parameters (rows, amplitude factor)
    // --- pipeline slots: these buffers and events exist once per set (cfg.nsets); everything reads the SELECTED
    // set through set() (pb_select_set)
    struct PB_LOCAL BufSet {
        DevBuf<uint8_t> d_in;            // [A][S][2][seg_samples]
        DevBuf<uint8_t> d_flags;         // [A][S*R*25]
        DevBuf<float> d_wrow;            // [A][S*R] row weights, then [A][S*R] uint32 row flag masks (pb_rowmask)
        DevBuf<float> d_stats;           // debug: [A][3][2][S*R*25] pow,kur,dag
        DevBuf<float> d_fraw, d_fkur;    // hipFFT path: f32 voltages, same indexing as d_in
        DevBuf<float2> d_Xraw, d_Xkur;   // hipFFT path: [A][S][2][R][6251]
        DevBuf<float> d_Praw, d_Pkur;    // LDS path: power [A][S][2][R][4096]; coherence: complex, float2 [A][S][2][R][4096]
        DevBuf<uint8_t> d_codes;         // [A][2 streams][S][trim]
        PinBuf<uint8_t> h_codes;         // pinned mirror of d_codes, filled asynchronously after detect
        DevBuf<float> d_ave;             // [A][2 streams][S][ave_per_seg]
        float *d_coadd_target = nullptr; // nant = 1: the coadd stream's plane of antenna 0 goes here instead (pb_set_coadd_target).
                                         // THE CALLER'S memory: never freed here
        PinBuf<int32_t> h_frame_idx;     // page-locked VDIF frame index of this set (the H2D copy of it is asynchronous)
        Event ev_idx;                    // that copy has completed: the host may rewrite the index
        Event ev_chan;                   // kernels of this set done (its D2H may start)
        Event ev_det;                    // D2H of this set done (set may be refilled / fetched)
        Event ev_cl;                     // pb_coadd_local has read this set's fp32 planes (next detect may overwrite)
        int processed = 0;               // segments of the last pb_process on this set
    };
    int fuse = 0;                                      // PB_FUSE_KURTOSIS at pb_create (pb_fused_kurtosis)
    std::vector<BufSet> sets;
    int cur_set = 0;
    BufSet &set() { return sets[cur_set]; }
    const BufSet &set() const { return sets[cur_set]; }
    int last_set = -1;               // buffer set of the previous pb_process (-1: none)
    bool staged = false;             // input has been queued on s_kur since the last pb_process
    DevBuf<uint8_t> d_coadd_codes;   // [2][S*trim] coadded bytes, made by the first pb_coadd_finish / pb_coadd_publish
    PinBuf<uint8_t> h_coadd_codes;   // their pinned mirror, likewise
    Event ev_coadd[2];
    int coadd_slot = 0, coadd_last = 0;
    struct pb_corr_state *corr = nullptr;   // the correlator's job (pb_job.h; pb_correlate.hip), from its first call on
    struct pb_track_state *track = nullptr; // pb_correlate_tracked's (pb_correlate_track.hip), likewise
    struct pb_beam_state *beam = nullptr, *beamproj = nullptr;   // pb_beamform's and pb_beamform_proj's (pb_beamform.hip), likewise
    struct pb_plane_state *plane = nullptr;                      // pb_beam_planes' own buffers (pb_beam_plane.hip), likewise
    FftTables ft;
    DagConsts dag = {}, dag_fb = {};   // D'Agostino constants for N = 500 (blocks) and N = 12500 (FFT rows, K4)
    int dag_bands = 0;               // 1: crossings located (flags decided without the cube root); -1: PB_DAG_BANDS=0; -2: search failed, fallback
    DevBuf<DagConsts> d_dag;         // dag in device memory (not counted in device_bytes)
    std::map<long, hipfftHandle> plans;

    bool profile = false;
    pb_timers timers = {};
    struct Pending { int stage; hipEvent_t a, b; };
    std::vector<Pending> pending;        // recorded, not yet read back: events out of ev_pool, which they return to
    EventPool ev_pool;
};

// Launchers enqueue on h->stream: this sends them to another stream for one scope and puts the handle back on its own
// stream on every way out of it.
struct StreamScope {
    pb_handle *h;
    hipStream_t saved;
    StreamScope(pb_handle *h_, hipStream_t s) : h(h_), saved(h_->stream) { h->stream = s; }
    ~StreamScope() { h->stream = saved; }
};

// ---- what the library's files share (each defined in the file named beside it unless inline here); on top of it,
// pb_job.h: the host side of the calls that run beside the pipeline on a stream of their own (correlator, beamformer,
// imager) ----
#define HIPCHK(h, call)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                 \
            return PB_EHIP;                                                               \
        }                                                                                 \
    } while (0)

PB_LOCAL int fail(pb_handle *h, int code, const std::string &msg);   // pb_handle.hip; h = nullptr: the error pb_create reports
PB_LOCAL hipError_t sync_all(pb_handle *h);                          // pb_handle.hip
PB_LOCAL int pb_skip_mask();                                         // pb_handle.hip: PB_SKIP of the experiments build, else 0
PB_LOCAL int pb_lean_lds(int dflt);                                  // pb_handle.hip, FFT_LEAN variant builds only
PB_LOCAL void pb_correlate_free(pb_handle *h);                       // pb_correlate.hip: what pb_destroy releases
PB_LOCAL void pb_correlate_track_free(pb_handle *h);                 // pb_correlate_track.hip: likewise
PB_LOCAL void pb_beamform_free(pb_handle *h);                        // pb_beamform.hip: likewise, both calls' states
PB_LOCAL void pb_beam_plane_free(pb_handle *h);                      // pb_beam_plane.hip: likewise
// pb_tables.hip: what pb_create builds (twiddles and FIR taps; taps = 4: history slots and window energies; D'Agostino constants)
PB_LOCAL int build_fft_tables(pb_handle *h);
PB_LOCAL int build_pfb_history(pb_handle *h);
PB_LOCAL int build_dag(pb_handle *h, bool search_bands);
PB_LOCAL int set_frb(pb_handle *h, float dm, float width_rows, float amp);

static inline int check_ant(pb_handle *h, int ant)
{
    if (ant < 0 || ant >= h->A) return fail(h, PB_EINVAL, "antenna index out of range");
    return PB_OK;
}

// a row of the PFB history (d_hist_in): 12500 samples and the overhang of the channeliser's 16-byte row loads
#define PFB_HIST_STRIDE 12512

// device_bytes follows every buffer that grows through here
template <class T>
hipError_t DevBuf<T>::grow(pb_handle *h, size_t n)
{
    if (n <= cap) return hipSuccess;
    h->device_bytes -= cap * sizeof(T);
    hipError_t e = alloc(n);
    if (e == hipSuccess) h->device_bytes += n * sizeof(T);
    return e;
}

// Per-stage device time without disturbing the stream: each stage records a pair of events
// from a pool; pb_get_timers synchronises once and reads them all back.
PB_LOCAL hipEvent_t take_event(pb_handle *h);
PB_LOCAL void retire_done(pb_handle *h);
PB_LOCAL void drain_timers(pb_handle *h);
struct StageTimer {
    pb_handle *h;
    int stage;
    hipEvent_t a, b;
    StageTimer(pb_handle *h_, int s) : h(h_), stage(s), a(nullptr), b(nullptr)
    {
        if (h->profile) {
            if (h->ev_pool.free.size() < 2) retire_done(h);
            a = take_event(h);
            b = take_event(h);
            (void)hipEventRecord(a, h->stream);
        }
    }
    void stop()
    {
        if (!h->profile) return;
        (void)hipEventRecord(b, h->stream);
        h->pending.push_back({stage, a, b});
    }
};

// The channeliser computes the kurtosis flags of its own rows (k_channelize_kur) instead of a kurtosis pass in
// front of it: in-library FFT, rectangular window, an RFI mode that flags, no statistics kept.  PB_FUSE_KURTOSIS=0
// keeps the two kernels (timing experiments).
bool pb_fused_kurtosis(const pb_handle *h);
// PB_EXPERIMENTS: the experiments build (libpb_hip_exp.so, `make exp`) also reads PB_SKIP, which leaves kernels out
// (results invalid; energy and upper-bound measurements).  Never in the shipped library.
#ifndef PB_EXPERIMENTS
#define PB_EXPERIMENTS 0
#endif
// row flag masks (bit r = kurtosis block r of the row is flagged), written by k_kurtosis_row behind the weights.
// taps = 4 adds bit 31 (k_pfb_weights): the row's window is complete and has no flag, so its excised power IS its raw
// power -- k_channelize_pfb then writes it to the raw plane only and detect's excised stream takes it from there.  (The
// weight cannot say so: flagging the faintest block of the window alone, E / total = 2e-9, still rounds to 1.0f.)
#define PB_ROWMASK_FLAGS 0x1ffffffu
#define PB_ROWMASK_KUR_IN_RAW 0x80000000u
static inline uint32_t *pb_rowmask(pb_handle *h) { return (uint32_t *)(h->set().d_wrow.p + (size_t)h->A * h->S * h->R); }

// ---- launchers (each enqueues on h->stream and returns a hipError_t) ----
hipError_t launch_kurtosis_flag(pb_handle *h, int nseg, bool write_f32);
hipError_t launch_deframe(pb_handle *h, int ant, int seg0, size_t nframes_per_thread);
hipError_t launch_dag_scan(pb_handle *h, const DagConsts &c, uint32_t bits0, int n, uint8_t *d_out);
hipError_t launch_dag_check(pb_handle *h, uint32_t bits_lo, uint64_t n, unsigned long long *d_mismatches);
hipError_t launch_inject_c64(pb_handle *h, int nseg, int inject_now);
hipError_t launch_detect(pb_handle *h, int nseg, int inject_now);
hipError_t launch_detect_pow(pb_handle *h, int nseg);
hipError_t launch_detect_coh(pb_handle *h, int nseg);   // coherence = 1 (k_detect_coh.hip)
// device -> pinned host copy done by a kernel (see k_detect.hip: hipMemcpyAsync blocks the host now and then)
hipError_t launch_copy_out(const PbSched &sched, uint8_t *host_pinned, const uint8_t *dev, size_t nbytes, hipStream_t st);
hipError_t launch_channelize(pb_handle *h, int nseg, int inject_now);
hipError_t launch_channelize_pfb(pb_handle *h, int nseg, int inject_now);
hipError_t launch_pfb_weights(pb_handle *h, int nseg);
hipError_t launch_pfb_history(pb_handle *h, int nseg);   // taps = 4: the batch's last three rows and flags into the history slot the NEXT batch reads
hipError_t launch_channelize_f32(pb_handle *h, const float *d_x, int nrows, int taps, float2 *d_out);
hipError_t launch_coadd_local(pb_handle *h, int nseg, float *d_sum, int accumulate, hipStream_t st);
hipError_t launch_coadd_local_codes(pb_handle *h, int nseg, float *d_sum, int accumulate, hipStream_t st);   // coadd_codes.hip
hipError_t launch_coadd_digitise_flat(pb_handle *h, const float *d_sum, size_t nfloat, float scale, uint8_t *d_codes,
                                      hipStream_t st);
hipError_t launch_coadd_tree(const float *const *leaves, int n, float *d_dst, size_t nfloat, hipStream_t st);
hipError_t launch_coadd_digitise(pb_handle *h, int nseg, const float *d_sum, float scale,
                                 uint8_t *d_codes, hipStream_t st);
