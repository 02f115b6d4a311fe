// What the search's translation units share on the host side: the handle, the dispersion delay, the error and timer
// helpers, and each stage's free function.  search_run.hip holds the core (create .. fetch_clean) and the RFI cleaning, search_rfichan.hip the cleaning's channel stage;
// search_cutout.hip, search_refine.hip, search_giants.hip, search_stream.hip, search_pol.hip, search_subband.hip and search_periodic.hip one optional stage each, kernels and host side together (a
// kernel lives in the file that launches it); search_plane.hip the streaming stage's entry for fp32 planes.  Device-only helpers: search_dev.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "pb_hip.h"

#define SEARCH_LOCAL __attribute__((visibility("hidden")))      // shared between the search's files, not exported

// Every member has a default initialiser: new pb_search() is a valid handle with every stage off, and a stage's free
// function ends with `s->stage = {}`.
struct pb_search {
    int device = 0, nchan = 0, max_samples = 0, ndm = 0, nbox = 0;
    float fch1 = 0.f, foff = 0.f, tsamp = 0.f;
    double dm_last = 0, ftop = 0;          // the grid's last trial DM; the delays' reference frequency (top of the band, MHz)
    int max_delay = 0;
    uint8_t *d_codes = nullptr, *d_xt = nullptr;       // raw block; channel-major [nchan][tpitch]
    int32_t *d_delay = nullptr;            // [ndm][nact] delays of the channels that are not zapped
    int32_t *d_chans = nullptr;            // [nact] their indices
    int nact = 0;
    uint32_t *d_D = nullptr;               // [ndm][max_samples]
    float *d_stats = nullptr;              // [ndm][2] mean, rms
    float *d_snr = nullptr;                // [ndm][max_samples]
    uint8_t *d_wid = nullptr;              // [ndm][max_samples] log2 width
    uint64_t *d_P = nullptr;               // [ndm][ppitch()] prefix sums of D (P[0] = 0)
    int32_t *d_peaks = nullptr;            // [1 + 4 * max_peaks]: count, then (dm index, sample, S/N bits, log2 width)
    int max_peaks = 1 << 20;
    int baseline = 0;                      // running-baseline window in samples (0: one clipped mean per DM series)
    int last_tout = 0, last_nsamp = 0;     // last run: output samples, block length
    int plane_tout = 0;                    // tout of the planes in d_snr / d_wid (the last run's, or pb_search_set_planes')
    float ms[6] = {};                      // last run: H2D, transpose, dedisperse, prefix + statistics, boxcar, D2H
    hipEvent_t ev[7] = {};
    size_t tpitch = 0;
    hipStream_t stream = nullptr;
    std::string err;
    size_t ppitch() const { return tpitch + 8; }       // pitch of a row of prefix sums

    // RFI cleaning (pb_search_set_rfi); the buffers exist once it has been switched on
    struct {
        int narrow = 0, broad = 0, nbox = 5;
        float tol = 5.0f;
        int ran = 0;                       // whether the last run was cleaned
        int32_t *d_zdelay = nullptr;       // [nact] zeros: k_dedisperse at DM 0 gives the zero-DM series
        uint8_t *d_med = nullptr;          // [nact] median code of each unzapped channel
        uint32_t *d_z = nullptr;           // [tpitch] zero-DM series
        uint64_t *d_zP = nullptr;          // [ppitch()] its prefix sums
        float *d_zstats = nullptr, *d_zsnr = nullptr;  // [2], [tpitch]
        uint8_t *d_zwid = nullptr;         // [tpitch]
        int32_t *d_tlist = nullptr;        // [tpitch] flagged samples of the broad pass
        unsigned long long *d_rcnt = nullptr;          // [2]: narrow flags, broad samples
        hipEvent_t ev[1] = {};             // end of cleaning (it starts at the core's ev[2])
        uint64_t n_narrow = 0;
        int n_broad = 0;
        float ms = 0.f;
    } rfi;
    // the cleaning's channel stage (pb_search_set_rfi_chan); the buffers exist while it is switched on (tol > 0)
    struct {
        int radius = 0, nlag = 0, npad = 0;
        float tol = 0.f;
        int ran = 0;                       // whether the last block went through the stage
        int have = 0;                      // the buffers hold the results of the block in d_xt (a gulp cleaned in place keeps them)
        int launched = 0;                  // the last search_block launched the stage itself
        int32_t *d_lags = nullptr;         // [nlag] signed lags
        int64_t *d_mom = nullptr;          // [2][nact] sum, S of each unzapped channel
        uint8_t *d_fill = nullptr, *d_mask = nullptr;  // [nact] rounded mean; flag
        uint8_t *d_tab = nullptr;          // [nlag][nact] outlier of the lag
        int32_t *d_cnt = nullptr;          // [2][nact] recv, cast; then nflag
        hipEvent_t ev[3] = {};             // start, end of the stage; end of the cleaning window where narrow and broad are off
    } chan;
    // cutouts (pb_search_set_cutouts); the buffers exist while it is switched on (max > 0)
    struct {
        int nsub = 0, nt = 0, ndmrow = 0, max = 0;
        int32_t *d_req = nullptr;          // [max][3] requests: DM index, peak sample, time-scrunch factor
        int32_t *d_sub = nullptr;          // [nsub][2] each subband's run [first, last) of chans[]
        uint32_t *d_out = nullptr;         // one call's outputs (cut_layout)
        uint32_t *h_out = nullptr;         // page-locked: the same, then the requests
        hipEvent_t ev[3] = {};             // start, kernels done, copy done
        float ms[2] = {};                  // last call: kernels, kernels + D2H copy
    } cut;
    // refinement (pb_search_set_refine); the buffers exist while it is switched on (max > 0)
    struct {
        int nstep = 0, H = 0, wmax = 0, max = 0;
        double *d_g = nullptr;             // [nact] f^-2 - ftop^-2 of each unzapped channel (delay_chan_term)
        int32_t *d_reqi = nullptr;         // [max][4] requests: peak sample, odd width, status, 0
        float *d_reqf = nullptr;           // [max][2] dm_lo, dm_step
        int32_t *d_out = nullptr;          // one call's outputs (refine_layout)
        int32_t *h_out = nullptr;          // page-locked: the same, then the requests
        hipEvent_t ev[3] = {};             // start, kernels done, copy done
        float ms[2] = {};                  // last call: kernels, kernels + D2H copy
    } rf;
    // giants and clusters (pb_search_set_giants); the buffers exist while the stage is switched on (max > 0)
    struct {
        int sep_time = 0, sep_dm = 0, sep_filter = 0, max = 0;
        int last = 0;                      // giants of the last pb_search_giants that are in d_giants (0 after an overflow)
        int sweeps = 0;                    // hook / jump sweeps of the last call
        int32_t *d_cnt = nullptr, *d_row = nullptr;    // [ndm] giants per series; [ndm + 1] their exclusive sums = each row's first giant
        int32_t *d_giants = nullptr;       // [max][8] the giants, ascending (dmi, begin)
        int32_t *d_lab = nullptr;          // [max] labels
        unsigned long long *d_best = nullptr;          // [max] per label: the largest (S/N key, ~member index)
        int32_t *d_acc = nullptr;          // [max][4] per label: members, points, INT_MAX - smallest begin, largest end
        int32_t *d_tile = nullptr;         // [ntile] roots per 256 giants, then [ntile + 1] their exclusive sums
        int32_t *d_out = nullptr;          // [16] control words (G, overflow, candidates, changed), then [max][8] the candidates
        int32_t *h_out = nullptr;          // page-locked: the same
        hipEvent_t ev[4] = {};             // start, giants written, candidates made, copy done
        float ms[3] = {};                  // last call: giant pass, labelling + merge, everything with the copy
    } gi;
    // streaming (pb_search_set_gulp): d_xt is filled piece by piece; the side buffer exists while it is switched on (keep_max > 0)
    struct {
        int keep_max = 0;
        int fill = 0;                      // samples per channel accumulated in d_xt
        int cleaned = 0;                   // d_xt[.][0, fill) was cleaned in place by a gulp call since the last push / advance
        int tail_n = 0;                    // d_tail row c holds the raw samples [fill - tail_n, fill) of channel c
        uint8_t *d_tail = nullptr;         // [nchan][kpitch]
        size_t kpitch = 0;
        hipEvent_t ev[5] = {};             // push: start, bytes on the device, appended; advance: start, end
        float ms[3] = {};                  // last push: copy, append; last advance
    } gp;
    // polarisation (pb_search_set_pol): the blocks are [nsamp][4][nchan]; the buffers exist while it is switched on (max > 0)
    struct {
        int off_len = 0, guard = 0, nrm = 0, max = 0;
        double rm_lo = 0, rm_step = 0;
        int have = 0;                      // the planes hold the last block searched
        uint8_t *d_codes = nullptr;        // [max_samples][4][nchan] staging of a host block
        uint8_t *d_plane[4] = {};          // AA, BB, CR, CI: channel-major [nchan][tpitch] + the gather's pad, as d_xt
        int32_t *d_req = nullptr;          // [max][3] requests: DM index, peak sample, on-window length
        double *d_st = nullptr;            // [max][3][nact] q, u, lambda^2 - lambda0^2 of each unzapped channel
        uint8_t *d_out = nullptr;          // one call's outputs (pol_layout)
        uint8_t *h_out = nullptr;          // page-locked: the same, then the requests
        uint32_t *d_cut = nullptr, *h_cut = nullptr;   // pb_search_pol_cutouts: pft [n][4][nsub][nt], pft_hits [n][nsub][nt]
        int cut_sig[4] = {};               // (nsub, nt, cutouts' max_cands, max) that d_cut / h_cut were made for
        hipEvent_t ev[3] = {};             // start, kernels done, copy done
        float ms[2] = {};                  // last pb_search_pol: kernels, kernels + D2H copy
    } pol;
    // sub-band search (pb_search_set_subbands); the buffers exist while it is switched on (nbands > 0)
    struct {
        int nsb = 0, nbands = 0, max = 0;
        int chunk = 0;                     // trial DMs per pass of the stage's kernels
        int32_t *d_run = nullptr;          // [nsb][2] each base sub-band's run [first, last) of chans[]
        int32_t *d_bands = nullptr;        // [nbands][2] first base sub-band, how many
        uint32_t *d_S = nullptr;           // [nsb][rows][tpitch] sub-band series of a pass's rows
        uint32_t *d_B = nullptr;           // [nbands][rows][tpitch] band series; the next four are laid out the same
        uint64_t *d_P = nullptr;           // prefix sums, pitch ppitch()
        float *d_stats = nullptr, *d_snr = nullptr;
        uint8_t *d_wid = nullptr;
        int32_t *d_pts = nullptr;          // [1 + PB_SUBPOINT_WORDS * max]: count, then the points
        float *d_best = nullptr;           // [tpitch] pb_search_subband_dm: best S/N
        uint8_t *d_bestw = nullptr;        // [2][tpitch] its log2 width, its band
        std::vector<hipEvent_t> ev;        // per pass: start, dedispersed, statistics; then kernels done, copy done
        float ms[4] = {};                  // last pb_search_subbands: dedispersion, sums + statistics, boxcars + best, all with the copy
    } sub;
    // periodicity search (pb_search_set_periodic); the buffers exist while it is switched on (bins > 0)
    struct {
        int bins = 0, k_lo = 0, k_hi = 0, Q = 0;           // base periods bins .. 2 bins - 1, octaves, widths 2^0 .. 2^Q = bins / 2
        int chunk = 0;                     // trial DMs per pass of the stage's kernels
        size_t spitch = 0;                 // words of a scratch row: one trial DM, one octave, every base period's M rows
        uint32_t *d_buf[2] = {};           // [chunk][spitch] the folding stages, written in turn
        int32_t *d_tab = nullptr;          // [nk][bins][4] per octave and base period: offset in the scratch row, m, L, M
        std::vector<int32_t> h_tab;        // the same on the host
        int tab_tout = 0;                  // tout that the tables were made for
        int32_t *d_best = nullptr;         // [ndm][nk][bins][4] S/N bits, i, q, j
        uint32_t *d_fprof = nullptr;       // pb_search_periodic_fold: [M][p] profiles
        float *d_fsnr = nullptr;           // [M][Q + 1] S/N
        int32_t *d_fj = nullptr;           // [M][Q + 1] first bin of the best window
        std::vector<hipEvent_t> ev;        // per pass and octave: start, folded; then kernels done, copy done
        float ms[3] = {};                  // last pb_search_periodic: folding, evaluation, everything with the copy
    } per;
};

// The dispersion delay of one channel in samples, in double: 4.148808e3 MHz^2 s (src/candidate.py:33) x DM x
// (f^-2 - ftop^-2) / tsamp, rounded half up.  The ONE place it is written: the trial DMs' table (search_create, host) and
// the fine trials of the refinement (k_refine_series, device) both come from here; IEEE double, no contraction.
static __host__ __device__ inline double delay_chan_term(double f, double ftop) { return 1.0 / (f * f) - 1.0 / (ftop * ftop); }
static __host__ __device__ inline int32_t delay_samples(double dm, double chan_term, double tsamp)
{
    const double d = 4.148808e3 * dm * chan_term / tsamp;
    return (int32_t)floor(d + 0.5);
}

extern SEARCH_LOCAL std::string g_search_err;      // the error of a call that has no handle to keep it in

// "<fn>: <what>" becomes the handle's last error (the global one without a handle); returns PB_EINVAL
static inline int search_fail(pb_search *s, const char *fn, const std::string &what)
{
    (s ? s->err : g_search_err) = std::string(fn) + ": " + what;
    return PB_EINVAL;
}

#define SCHK(s, call)                                                         \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) {                                               \
            (s)->err = std::string(#call) + ": " + hipGetErrorString(e_);     \
            return PB_EHIP;                                                   \
        }                                                                     \
    } while (0)

// The opening checks of a stage's entry point: a handle, the stage switched on, something to work on.  `on` and `ready`
// are written `s && ...` by the caller.  PB_OK, or the error recorded by search_fail.
static inline int search_enter(pb_search *s, const char *fn, bool on, const char *off_msg, bool ready, const char *idle_msg)
{
    if (!s) return search_fail(nullptr, fn, "no search handle");
    if (!on) return search_fail(s, fn, off_msg);
    if (!ready) return search_fail(s, fn, idle_msg);
    return PB_OK;
}

// device ms from event a to event b, 0 if either was not recorded
static inline float search_ms(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}

// the body of every *_timers getter
static inline int search_get_ms(const pb_search *s, const float *ms, int n, float *out)
{
    if (!s || !out) return PB_EINVAL;
    for (int i = 0; i < n; ++i) out[i] = ms[i];
    return PB_OK;
}

// what a stage's free function does before it assigns `s->stage = {}`: nullptr entries are skipped
static inline void search_release(std::initializer_list<void *> dev, void *host, hipEvent_t *ev, int nev)
{
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (host) (void)hipHostFree(host);
    for (int i = 0; i < nev; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
}

SEARCH_LOCAL void search_rfi_free(pb_search *s);
SEARCH_LOCAL void search_rfichan_free(pb_search *s);
SEARCH_LOCAL void search_cutouts_free(pb_search *s);
SEARCH_LOCAL void search_refine_free(pb_search *s);
SEARCH_LOCAL void search_giants_free(pb_search *s);
SEARCH_LOCAL void search_gulp_free(pb_search *s);
SEARCH_LOCAL void search_pol_free(pb_search *s);
SEARCH_LOCAL void search_subbands_free(pb_search *s);
SEARCH_LOCAL void search_periodic_free(pb_search *s);

// search_rfichan.hip, for search_run.hip: the channel stage on the nsamp samples of d_xt, in place
SEARCH_LOCAL int search_rfichan_launch(pb_search *s, int nsamp);
// search_pol.hip, for search_run.hip: the transposition of a [nsamp][4][nchan] block into the four product planes and the
// search plane d_xt (between ev[1] and ev[2]); codes: device bytes
SEARCH_LOCAL int search_pol_transpose(pb_search *s, const uint8_t *codes, int nsamp);
// search_cutout.hip, for search_pol.hip: k_cutout_ft over the requests in cut.d_req on a channel-major plane laid out as d_xt
SEARCH_LOCAL void search_cutout_ft_launch(pb_search *s, const uint8_t *plane, int n, uint32_t *ft, uint32_t *fth);
// search_cutout.hip, for search_subband.hip too: run = [nsub][2], each subband's run [first, last) of chans[] (zapped
// channels are left out of chans[], so the unzapped channels of [b nchan/nsub, (b+1) nchan/nsub) are one run of it)
SEARCH_LOCAL int search_sub_runs(pb_search *s, int nsub, std::vector<int32_t> &run);
// search_run.hip, for search_subband.hip: k_prefix and k_series_stats, then k_boxcar (no peak list), on nrow series laid
// out like d_D / d_P / d_stats / d_snr / d_wid, with the handle's baseline window and boxcars
SEARCH_LOCAL void search_series_launch(pb_search *s, const uint32_t *D, uint64_t *P, float *stats, int nrow, int tout);
SEARCH_LOCAL void search_boxcar_launch(pb_search *s, const uint64_t *P, const float *stats, float *snr, uint8_t *wid, int nrow, int tout);

// search_run.hip, for search_stream.hip: the search from the cleaning on over the nsamp samples that d_xt holds (after
// ev[2]; `cleaned`: leave the cleaning out, the block is cleaned already), and the copies to the host that end
// pb_search_run / pb_search_peaks
SEARCH_LOCAL int search_block(pb_search *s, int nsamp, float thresh, bool want_peaks, bool cleaned);
SEARCH_LOCAL int search_run_out(pb_search *s, float *snr, uint8_t *width_log2, uint32_t *series, float *stats, int *tout_out);
SEARCH_LOCAL int search_peaks_out(pb_search *s, int32_t *peaks, int max_out, int *npeaks, int *tout_out);
