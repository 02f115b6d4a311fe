// On-GPU incoherent dedispersion + boxcar matched filter over a (coadded) filterbank block:
// the stage downstream of process_baseband in the reference's production chain
// (external `heimdall_stream -dm 2 1000 -boxcar_max 64 -nsamps_gulp 30720 -zap_chans 0 190
//  -zap_chans 3900 4096`, /root/reference/scripts/start_heimdall_single_antenna:21).
// heimdall and its dedisp library are third-party and absent, so parity with heimdall's candidate
// list is UNPINNED; what is pinned is the arithmetic below against a NumPy restatement (tests) and
// the recovered S/N against the reference's own estimator (analysis/loc_step0.py:optimize_pulse).
//
//   1. transpose the time-major codes [T][nchan] (SIGPROC order, 8/4/2-bit) to channel-major u8
//   2. brute-force dedispersion: D[dm][t] = sum over unzapped channels of x[c][t + delay(dm, c)],
//      delay = round(4.148808e3 * dm * (f_c^-2 - f_top^-2) / tsamp)  (MHz; src/candidate.py:33)
//   3. per-DM mean / rms with one 3-sigma clip, boxcars 2^0..2^k (k = log2 boxcar_max):
//      S/N(t, w) = (sum_{i<w} D[t+i] - w mean) / (rms sqrt(w)); keep the best width per (dm, t)
// All integer up to the normalisation, so 1-2 are bit-exact vs the NumPy restatement.
// Optional between 1 and 2: RFI cleaning of the channel-major block in place (pb_search_set_rfi; off by default, and
// then nothing of it is launched).  The definition is include/pb_hip.h's; the kernels are k_rfi_narrow (per-channel
// histogram, median, MAD, outliers -> median), then the zero-DM series through k_dedisperse / k_prefix /
// k_series_stats / k_boxcar, k_rfi_broad_list (the flagged samples) and k_rfi_broad_mask (those samples -> median).
// Optional after a run: per-candidate cutouts of the block and of the dedispersed series that are still on the device
// (pb_search_set_cutouts / pb_search_cutouts; definition in include/pb_hip.h): k_cutout_ft, k_cutout_dt.
// Optional after a run: a candidate's DM, width and S/N refined on a fine DM grid with the reference's estimator
// (analysis/loc_step0.py: refine_dm, optimize_pulse), from the block that is still on the device (pb_search_set_refine /
// pb_search_refine; definition in include/pb_hip.h): k_refine_series, k_refine_dm, k_refine_width.
// Optional after a run: the S/N planes that are still on the device turned into giants and clusters of giants, one
// candidate per cluster (pb_search_set_giants / pb_search_giants; definition in include/pb_hip.h): k_giant_count,
// k_giant_scan, k_giant_write, then k_giant_hook / k_giant_jump until no label changes, k_giant_reduce, k_giant_cands.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pb_hip.h"

struct pb_search {
    int device, nchan, max_samples, ndm, nbox;
    float fch1, foff, tsamp, dm_min, dm_step;
    int max_delay;
    uint8_t *d_codes, *d_xt;       // raw block; channel-major [nchan][tpitch]
    int32_t *d_delay;              // [ndm][nact] delays of the channels that are not zapped
    int32_t *d_chans;              // [nact] their indices
    int nact;
    uint32_t *d_D;                 // [ndm][max_samples]
    float *d_stats;                // [ndm][2] mean, rms
    float *d_snr;                  // [ndm][max_samples]
    uint8_t *d_wid;                // [ndm][max_samples] log2 width
    uint64_t *d_P;                 // [ndm][tpitch + 1] prefix sums of D (P[0] = 0)
    int32_t *d_peaks;              // [1 + 4 * max_peaks]: count, then (dm index, sample, S/N bits, log2 width)
    int max_peaks;
    int baseline;                  // running-baseline window in samples (0: one clipped mean per DM series)
    int last_tout;
    float ms[6];                   // last run: H2D, transpose, dedisperse, prefix + statistics, boxcar, D2H
    hipEvent_t ev[7];
    size_t tpitch;
    hipStream_t stream;
    std::string err;
    // RFI cleaning (pb_search_set_rfi); the buffers exist once it has been switched on
    int rfi_narrow, rfi_broad, rfi_nbox;
    float rfi_tol;
    int last_nsamp, rfi_ran;       // last run: block length, whether it was cleaned
    int32_t *d_zdelay;             // [nact] zeros: k_dedisperse at DM 0 gives the zero-DM series
    uint8_t *d_med;                // [nact] median code of each unzapped channel
    uint32_t *d_z;                 // [tpitch] zero-DM series
    uint64_t *d_zP;                // [tpitch + 8] its prefix sums
    float *d_zstats, *d_zsnr;      // [2], [tpitch]
    uint8_t *d_zwid;               // [tpitch]
    int32_t *d_tlist;              // [tpitch] flagged samples of the broad pass
    unsigned long long *d_rcnt;    // [2]: narrow flags, broad samples
    hipEvent_t ev_rfi;             // end of cleaning (it starts at ev[2])
    uint64_t n_narrow;
    int n_broad;
    float rfi_ms;
    // cutouts (pb_search_set_cutouts); the buffers exist while it is switched on (cut_max > 0)
    int cut_nsub, cut_nt, cut_ndmrow, cut_max;
    int32_t *d_cut_req;            // [cut_max][3] requests: DM index, peak sample, time-scrunch factor
    int32_t *d_cut_sub;            // [cut_nsub][2] each subband's run [first, last) of chans[]
    uint32_t *d_cut;               // one call's ft, ft_hits [n][nsub][nt] and dt, dt_hits [n][ndmrow][nt], back to back
    uint32_t *h_cut;               // page-locked: the same, then the requests
    hipEvent_t ev_cut[3];          // start, kernels done, copy done
    float cut_ms[2];               // last call: kernels, kernels + D2H copy
    // refinement (pb_search_set_refine); the buffers exist while it is switched on (rf_max > 0)
    double dm_last, ftop;          // the grid's last trial DM; the delays' reference frequency (top of the band, MHz)
    int rf_nstep, rf_H, rf_wmax, rf_max;
    double *d_rf_g;                // [nact] f^-2 - ftop^-2 of each unzapped channel (delay_chan_term)
    int32_t *d_rf_reqi;            // [rf_max][4] requests: peak sample, odd width, status, 0
    float *d_rf_reqf;              // [rf_max][2] dm_lo, dm_step
    double *d_rf_out;              // one call's sn_dm [n][nstep], opt_sn [n][nw] (double), kbest [n], opt_loc [n][nw] (i32),
                                   // then the fine series about each peak [n][nstep][2 (H + M)] (u32)
    double *h_rf;                  // page-locked: the same, then the series, then the requests
    hipEvent_t ev_rf[3];           // start, kernels done, copy done
    float rf_ms[2];                // last call: kernels, kernels + D2H copy
    // giants and clusters (pb_search_set_giants); the buffers exist while the stage is switched on (gi_max > 0)
    int gi_tout;                   // tout of the planes in d_snr / d_wid (the last run's, or pb_search_set_planes')
    int gi_sep_time, gi_sep_dm, gi_sep_filter, gi_max;
    int gi_last;                   // giants of the last pb_search_giants that are in d_gi (0 after an overflow)
    int gi_sweeps;                 // hook / jump sweeps of the last call
    int32_t *d_gi_cnt, *d_gi_row;  // [ndm] giants per series; [ndm + 1] their exclusive sums = each row's first giant
    int32_t *d_gi;                 // [gi_max][8] the giants, ascending (dmi, begin)
    int32_t *d_gi_lab;             // [gi_max] labels
    unsigned long long *d_gi_best; // [gi_max] per label: the largest (S/N key, ~member index)
    int32_t *d_gi_acc;             // [gi_max][4] per label: members, points, INT_MAX - smallest begin, largest end
    int32_t *d_gi_tile;            // [ntile] roots per 256 giants, then [ntile + 1] their exclusive sums
    int32_t *d_gi_out;             // [16] control words (G, overflow, candidates, changed), then [gi_max][8] the candidates
    int32_t *h_gi;                 // page-locked: the same
    hipEvent_t ev_gi[4];           // start, giants written, candidates made, copy done
    float gi_ms[3];                // last call: giant pass, labelling + merge, everything with the copy
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

static std::string g_search_err;

#define SCHK(s, call)                                                         \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) {                                               \
            (s)->err = std::string(#call) + ": " + hipGetErrorString(e_);     \
            return PB_EHIP;                                                   \
        }                                                                     \
    } while (0)

// codes: [T][nchan] samples of nbit bits, low bits first within a byte -> xt[c][t] u8
__global__ __launch_bounds__(256) void k_transpose_codes(const uint8_t *__restrict__ codes, uint8_t *__restrict__ xt,
                                                         int T, int nchan, int nbit, size_t tpitch)
{
    __shared__ uint8_t tile[64][65];
    const int t0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int per = 8 / nbit, maskv = (1 << nbit) - 1;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int tt = i / 64, cc = i % 64;
        const int t = t0 + tt, c = c0 + cc;
        uint8_t v = 0;
        if (t < T && c < nchan) {
            const size_t n = (size_t)t * nchan + c;
            v = (codes[n / per] >> (nbit * (n % per))) & maskv;
        }
        tile[tt][cc] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int cc = i / 64, tt = i % 64;
        const int t = t0 + tt, c = c0 + cc;
        if (t < T && c < nchan) xt[(size_t)c * tpitch + t] = tile[tt][cc];
    }
}

// Brute-force dedispersion, tiled over (time, DM): one workgroup = 2048 output samples x DDM_DB
// neighbouring trial DMs, a thread = 8 consecutive samples (two packed dwords) of every DM of the block.
// For each channel the 8 samples at t + delay(dm, c) are 12 bytes fetched with ONE 16-byte-or-less load
// per lane (the delay is uniform over the wave: its aligned part goes into the scalar offset of the
// load, its low two bits into v_alignbyte) instead of eight 1-byte loads, and neighbouring DMs of the
// block hit the same cache lines.  The bytes are summed as packed 16-bit pairs (v_pk_add_u16), widened to
// 32 bits every 256 channels (256 x 255 < 2^16).  Integer arithmetic: the sums are exact whatever the order.
#ifndef DDM_DB
#define DDM_DB 4
#endif
#ifndef DDM_SAMPLES
#define DDM_SAMPLES 8
#endif
#ifndef DDM_CU
#define DDM_CU 4          // channels whose loads are in flight together
#endif
#define DDM_TILE (256 * DDM_SAMPLES)

// chans: the nact channels that are not zapped; delay: [ndm][nact] over those channels
__global__ __launch_bounds__(256) void k_dedisperse(const uint8_t *__restrict__ xt, const int32_t *__restrict__ chans,
                                                    const int32_t *__restrict__ delay, uint32_t *__restrict__ D,
                                                    int nact, int ndm, int tout, size_t tpitch, size_t dpitch)
{
    const int dm0 = blockIdx.y * DDM_DB;
    const int t = blockIdx.x * DDM_TILE + threadIdx.x * DDM_SAMPLES;      // 4-byte aligned (tpitch is a multiple of 64)
    // Lanes past the last output sample of the last tile have nothing to do, and their loads (up to a tile past
    // tout, plus the delay) would leave the last channel's row -- and, for the last channel, the allocation
    // (tpitch * nchan + 64 bytes).  No barrier in this kernel: a whole-lane exit is safe.  A live lane reads at
    // most t + d + 11 <= tout - 1 + max_delay + 11 = nsamp + 10, inside the row's pitch or the 64-byte pad.
    if (t >= tout) return;
    uint32_t lo[DDM_DB][DDM_SAMPLES / 4], hi[DDM_DB][DDM_SAMPLES / 4];   // packed u16 partial sums: bytes 0,2 / 1,3
    uint32_t acc[DDM_DB][DDM_SAMPLES];
    const int32_t *dl[DDM_DB];
#pragma unroll
    for (int j = 0; j < DDM_DB; ++j) {
        dl[j] = delay + (size_t)(dm0 + j < ndm ? dm0 + j : ndm - 1) * nact;
#pragma unroll
        for (int w = 0; w < DDM_SAMPLES / 4; ++w) lo[j][w] = hi[j][w] = 0u;
#pragma unroll
        for (int i = 0; i < DDM_SAMPLES; ++i) acc[j][i] = 0u;
    }
    auto flush = [&]() {
#pragma unroll
        for (int j = 0; j < DDM_DB; ++j) {
#pragma unroll
            for (int w = 0; w < DDM_SAMPLES / 4; ++w) {
                acc[j][4 * w + 0] += lo[j][w] & 0xffffu;
                acc[j][4 * w + 1] += hi[j][w] & 0xffffu;
                acc[j][4 * w + 2] += lo[j][w] >> 16;
                acc[j][4 * w + 3] += hi[j][w] >> 16;
                lo[j][w] = hi[j][w] = 0u;
            }
        }
    };
    // one channel of one DM: samples t+d .. t+d+DDM_SAMPLES-1 = DDM_SAMPLES/4 + 1 aligned dwords from (t + d) & ~3
    auto fetch = [&](int c, int j, uint32_t (&w)[DDM_SAMPLES / 4 + 1], unsigned &sh) {
        const int32_t d = dl[j][c];                                 // uniform -> scalar load
        const uint32_t *p = (const uint32_t *)(xt + (size_t)chans[c] * tpitch + t + (d & ~3));
#pragma unroll
        for (int i = 0; i <= DDM_SAMPLES / 4; ++i) w[i] = p[i];
        sh = (unsigned)(d & 3);
    };
    auto add = [&](int j, const uint32_t (&w)[DDM_SAMPLES / 4 + 1], unsigned sh) {
#pragma unroll
        for (int i = 0; i < DDM_SAMPLES / 4; ++i) {
            const uint32_t a = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);      // bytes sh.. of w[i+1]:w[i]
            lo[j][i] += a & 0x00ff00ffu;
            hi[j][i] += (a >> 8) & 0x00ff00ffu;
        }
    };
    // DDM_CU channels at a time: all their loads are issued before the first is used (the loop is bound by
    // load latency, not by anything it computes)
    int c = 0, since = 0;
    for (; c + DDM_CU <= nact; c += DDM_CU) {
        uint32_t w[DDM_CU][DDM_DB][DDM_SAMPLES / 4 + 1];
        unsigned sh[DDM_CU][DDM_DB];
#pragma unroll
        for (int u = 0; u < DDM_CU; ++u)
#pragma unroll
            for (int j = 0; j < DDM_DB; ++j) fetch(c + u, j, w[u][j], sh[u][j]);
#pragma unroll
        for (int u = 0; u < DDM_CU; ++u)
#pragma unroll
            for (int j = 0; j < DDM_DB; ++j) add(j, w[u][j], sh[u][j]);
        since += DDM_CU;
        if (since >= 240) {                                     // 16-bit sums: at most 257 channels of 255 between flushes
            flush();
            since = 0;
        }
    }
    for (; c < nact; ++c) {
#pragma unroll
        for (int j = 0; j < DDM_DB; ++j) {
            uint32_t w[DDM_SAMPLES / 4 + 1];
            unsigned sh;
            fetch(c, j, w, sh);
            add(j, w, sh);
        }
    }
    flush();
#pragma unroll
    for (int j = 0; j < DDM_DB; ++j) {
        if (dm0 + j >= ndm) break;
        uint32_t *out = D + (size_t)(dm0 + j) * dpitch + t;
#pragma unroll
        for (int i = 0; i < DDM_SAMPLES; i += 4) {
            if (t + i + 4 <= tout) {
                *(uint4 *)(out + i) = make_uint4(acc[j][i], acc[j][i + 1], acc[j][i + 2], acc[j][i + 3]);
            } else {
                for (int q = 0; q < 4; ++q)
                    if (t + i + q < tout) out[i + q] = acc[j][i + q];
            }
        }
    }
}

__device__ __forceinline__ double block_sum(double v, double *sh)
{
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double r = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
    return r;
}

// Inclusive prefix sums of each DM series (64-bit: a series sums to ~2e10), P[0] = 0: boxcar sums and the
// running baseline become differences of two entries.  One workgroup per DM.
__global__ __launch_bounds__(256) void k_prefix(const uint32_t *__restrict__ D, uint64_t *__restrict__ P, int tout,
                                                size_t dpitch, size_t ppitch)
{
    __shared__ uint64_t sh[256];
    const uint32_t *x = D + (size_t)blockIdx.x * dpitch;
    uint64_t *p = P + (size_t)blockIdx.x * ppitch;
    const int per = (tout + 255) / 256;
    const int lo = threadIdx.x * per, hi = min(lo + per, tout);
    uint64_t s = 0;
    for (int t = lo; t < hi; ++t) s += x[t];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const uint64_t v = sh[i];
            sh[i] = run;
            run += v;
        }
        p[0] = 0;
    }
    __syncthreads();
    uint64_t run = sh[threadIdx.x];
    for (int t = lo; t < hi; ++t) {
        run += x[t];
        p[t + 1] = run;
    }
}

// baseline under sample t: the mean of the series over the W samples around it (window clamped to the
// series), or the per-series constant when W == 0
__device__ __forceinline__ float baseline_at(const uint64_t *__restrict__ p, int t, int W, int tout, float gmean)
{
    if (W <= 0) return gmean;
    int lo = t - W / 2, hi = lo + W;
    if (lo < 0) { lo = 0; hi = min(W, tout); }
    if (hi > tout) { hi = tout; lo = max(0, tout - W); }
    return (float)((double)(p[hi] - p[lo]) / (double)(hi - lo));
}

// mean and rms of each DM series about its baseline, then once more over the samples within 3 rms (definition:
// include/pb_hip.h, under pb_search_set_baseline)
__global__ __launch_bounds__(256) void k_series_stats(const uint32_t *__restrict__ D, const uint64_t *__restrict__ P,
                                                      float *__restrict__ stats, int tout, int W, size_t dpitch,
                                                      size_t ppitch)
{
    __shared__ double sh[4];
    const uint32_t *x = D + (size_t)blockIdx.x * dpitch;
    const uint64_t *p = P + (size_t)blockIdx.x * ppitch;
    const float gmean0 = (float)((double)p[tout] / (double)tout);
    double s1 = 0, s2 = 0;
    for (int t = threadIdx.x; t < tout; t += 256) {
        const double v = (double)x[t] - (double)baseline_at(p, t, W, tout, gmean0);
        s1 += v;
        s2 += v * v;
    }
    s1 = block_sum(s1, sh);
    s2 = block_sum(s2, sh);
    double mean = s1 / tout, var = s2 / tout - mean * mean;
    double rms = sqrt(var > 0 ? var : 0);
    const double mean1 = mean, rms1 = rms;
    double c1 = 0, cn = 0;
    for (int t = threadIdx.x; t < tout; t += 256) {
        const double v = (double)x[t] - (double)baseline_at(p, t, W, tout, gmean0);
        if (fabs(v - mean1) <= 3 * rms1) {
            c1 += v;
            cn += 1;
        }
    }
    c1 = block_sum(c1, sh);
    cn = block_sum(cn, sh);
    if (cn > 0) {                                   // (the same in every lane: the barriers below are uniform)
        mean = c1 / cn;
        // The variance about the clipped mean, in a pass of its own: sum v^2 / cn - mean^2 cancels to a rounding error
        // of either sign where the clip leaves a constant (a blanked block with one glitch), and a positive one made
        // an rms of 1e-9 and S/N of 1e11 there.  Here every kept v equals the mean and the rms is exactly 0.
        double d2 = 0;
        for (int t = threadIdx.x; t < tout; t += 256) {
            const double v = (double)x[t] - (double)baseline_at(p, t, W, tout, gmean0);
            if (fabs(v - mean1) <= 3 * rms1) d2 += (v - mean) * (v - mean);
        }
        d2 = block_sum(d2, sh);
        // a Gaussian clipped at 3 sigma has 0.9733 of its variance left
        rms = sqrt(d2 / cn / 0.97330);
    }
    if (threadIdx.x == 0) {
        // [0]: level to subtract on top of the running baseline (W > 0) or the clipped mean itself (W == 0)
        stats[2 * blockIdx.x] = (float)(W > 0 ? mean : mean + (double)gmean0);
        stats[2 * blockIdx.x + 1] = (float)rms;
    }
}

// best boxcar per (DM, sample) from prefix sums; samples at or above `thresh` also go to the peak list
__global__ __launch_bounds__(256) void k_boxcar(const uint64_t *__restrict__ P, const float *__restrict__ stats,
                                                float *__restrict__ snr, uint8_t *__restrict__ wid, int tout,
                                                int nbox, int W, size_t dpitch, size_t ppitch, float thresh,
                                                int32_t *__restrict__ peaks, int max_peaks)
{
    const int dm = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= tout) return;
    const uint64_t *p = P + (size_t)dm * ppitch;
    const float lvl = stats[2 * dm], rms = stats[2 * dm + 1];
    float best = -1e30f;
    int bw = 0;
    for (int k = 0; k < nbox; ++k) {
        const int w = 1 << k;
        if (t + w > tout) break;
        const float sum = (float)(p[t + w] - p[t]);
        const float base = W > 0 ? baseline_at(p, t + w / 2, W, tout, 0.f) + lvl : lvl;
        const float sn = (sum - (float)w * base) / (rms * sqrtf((float)w));
        if (sn > best) {
            best = sn;
            bw = k;
        }
    }
    if (!(rms > 0)) best = 0.f;
    snr[(size_t)dm * dpitch + t] = best;
    wid[(size_t)dm * dpitch + t] = (uint8_t)bw;
    if (peaks && best >= thresh) {
        const int i = atomicAdd(peaks, 1);
        if (i < max_peaks) {
            peaks[1 + 4 * i] = dm;
            peaks[2 + 4 * i] = t;
            peaks[3 + 4 * i] = __float_as_int(best);
            peaks[4 + 4 * i] = bw;
        }
    }
}

// ---- RFI cleaning (definition: include/pb_hip.h, pb_search_set_rfi) ----

// Wave 0 of a workgroup, a[j] = count of bin 4 lane + j: the smallest bin whose cumulative count reaches `need`
// (which the 256 bins together always reach), the same in every lane.
__device__ __forceinline__ int first_bin_reaching(const uint32_t (&a)[4], uint32_t need)
{
    const int lane = threadIdx.x & 63;
    const uint32_t loc = a[0] + a[1] + a[2] + a[3];
    uint32_t inc = loc;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
    }
    const int first = __builtin_ctzll(__ballot(inc >= need));
    uint32_t c = inc - loc;
    int k = 3;
    for (int j = 0; j < 4; ++j) {
        c += a[j];
        if (c >= need) {
            k = j;
            break;
        }
    }
    return __shfl(4 * lane + k, first);
}

// Narrow pass, one workgroup per unzapped channel: the row's 256-bin histogram (one per wave in LDS, then summed),
// med = smallest v with cumulative count >= ceil(nsamp/2), mad = smallest d with #{|x - med| <= d} >= ceil(nsamp/2);
// with `replace`, every x with (float)|x - med| > tol * 1.4826f * (float)max(mad, 1) becomes med (16-byte loads,
// a 16-byte store only where a byte changed) and the flags are counted.  med goes to med_out for the broad pass.
// The row is read twice from memory (it is at most max_samples bytes: the second read mostly hits the cache).
__global__ __launch_bounds__(256) void k_rfi_narrow(uint8_t *__restrict__ xt, const int32_t *__restrict__ chans,
                                                    uint8_t *__restrict__ med_out, int nsamp, size_t tpitch, float tol,
                                                    int replace, unsigned long long *__restrict__ nflag)
{
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t tot[256];
    __shared__ int sh_med, sh_mad;
    __shared__ uint32_t sh_cnt[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 4 * 256; i += 256) hist[i >> 8][i & 255] = 0u;
    __syncthreads();
    uint8_t *row = xt + (size_t)chans[blockIdx.x] * tpitch;         // tpitch % 64 == 0: rows are 16-byte aligned
    uint4 *rv = (uint4 *)row;
    const int nvec = nsamp >> 4;
    for (int i = threadIdx.x; i < nvec; i += 256) {
        const uint4 v = rv[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) atomicAdd(&hist[wave][(w[j] >> (8 * b)) & 255u], 1u);
    }
    for (int t = 16 * nvec + threadIdx.x; t < nsamp; t += 256) atomicAdd(&hist[wave][row[t]], 1u);
    __syncthreads();
    tot[threadIdx.x] = hist[0][threadIdx.x] + hist[1][threadIdx.x] + hist[2][threadIdx.x] + hist[3][threadIdx.x];
    __syncthreads();
    if (wave == 0) {
        const uint32_t need = (uint32_t)(nsamp + 1) / 2;
        uint32_t a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = tot[4 * lane + j];
        const int med = first_bin_reaching(a, need);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = 4 * lane + j;                             // count of |x - med| == d
            a[j] = d == 0 ? tot[med] : (med - d >= 0 ? tot[med - d] : 0u) + (med + d < 256 ? tot[med + d] : 0u);
        }
        const int mad = first_bin_reaching(a, need);
        if (lane == 0) {
            sh_med = med;
            sh_mad = mad;
            med_out[blockIdx.x] = (uint8_t)med;
        }
    }
    __syncthreads();
    if (!replace) return;
    const int med = sh_med;
    // (float)d > thr for an integer d in 0..255 (exact in binary32) <=> d > dlim
    const float thr = tol * 1.4826f * (float)max(sh_mad, 1);
    const int dlim = thr >= 255.f ? 255 : (int)floorf(thr);
    const uint32_t mb = (uint32_t)med;
    uint32_t cnt = 0;
    for (int i = threadIdx.x; i < nvec; i += 256) {
        const uint4 v = rv[i];
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t changed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t o = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t x = (w[j] >> (8 * b)) & 255u;
                const bool f = abs((int)x - med) > dlim;
                cnt += f;
                changed |= f;
                o |= (f ? mb : x) << (8 * b);
            }
            w[j] = o;
        }
        if (changed) rv[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (int t = 16 * nvec + threadIdx.x; t < nsamp; t += 256) {
        if (abs((int)row[t] - med) > dlim) {
            row[t] = (uint8_t)med;
            ++cnt;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_down(cnt, o);
    if (lane == 0) sh_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long n = (unsigned long long)sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
        if (n) atomicAdd(nflag, n);
    }
}

// Broad pass, flagged samples: t is flagged when some t0 in [t - widest + 1, t] has best zero-DM S/N >= tol and
// best width w with t0 + w > t.  Each flagged t is appended once to tlist (order unspecified), *nbroad counts them.
// widest <= 64; the S/N / width of the 256 + 63 starts that can reach this workgroup's samples go through LDS.
__global__ __launch_bounds__(256) void k_rfi_broad_list(const float *__restrict__ snr, const uint8_t *__restrict__ wid,
                                                        int nsamp, float tol, int widest, int32_t *__restrict__ tlist,
                                                        unsigned long long *__restrict__ nbroad)
{
    __shared__ int end[256 + 64];               // end[i]: t0 + w of start t0 = base - 64 + i if it is flagged, else 0
    const int base = blockIdx.x * 256;
    for (int i = threadIdx.x; i < 256 + 64; i += 256) {
        const int t0 = base - 64 + i;
        int e = 0;
        if (t0 >= 0 && t0 < nsamp && snr[t0] >= tol) e = t0 + (1 << wid[t0]);
        end[i] = e;
    }
    __syncthreads();
    const int t = base + threadIdx.x;
    if (t >= nsamp) return;
    bool f = false;
    for (int k = 0; k < widest; ++k) f |= end[64 + threadIdx.x - k] > t;
    if (f) {
        const unsigned long long i = atomicAdd(nbroad, 1ull);
        tlist[i] = t;
    }
}

// Broad pass, mask: every flagged sample of every unzapped channel becomes that channel's median; a wave per
// channel, its lanes over the list.  Only the flagged samples are visited.
__global__ __launch_bounds__(256) void k_rfi_broad_mask(uint8_t *__restrict__ xt, const int32_t *__restrict__ chans,
                                                        const uint8_t *__restrict__ med, const int32_t *__restrict__ tlist,
                                                        const unsigned long long *__restrict__ nbroad, int nact,
                                                        size_t tpitch)
{
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= nact) return;
    const int n = (int)*nbroad;
    uint8_t *row = xt + (size_t)chans[k] * tpitch;
    const uint8_t m = med[k];
    for (int i = threadIdx.x & 63; i < n; i += 64) row[tlist[i]] = m;
}

// ---- per-candidate cutouts (definition: include/pb_hip.h, pb_search_set_cutouts) ----

typedef uint32_t cut_u32x4 __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes at a 4-byte aligned address

#ifndef CUT_CU
#define CUT_CU 4          // channels whose loads are in flight together
#endif

// 16 consecutive bytes of one channel's span, already shifted into place and masked, onto the unit's accumulators.
// TS = 1 / 2: a bin is 1 / 2 bytes; TS = 4: tscr >= 4, a bin is a whole number of dwords (v_sad_u8 sums a dword's bytes).
template <int TS>
__device__ __forceinline__ void cutout_add(uint32_t (&acc)[16 / TS], const uint32_t (&a)[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (TS == 1) {
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[(4 * i + b) % (16 / TS)] += (a[i] >> (8 * b)) & 255u;
        } else if (TS == 2) {
            acc[(2 * i) % (16 / TS)] = __builtin_amdgcn_sad_u8(a[i] & 0xffffu, 0u, acc[(2 * i) % (16 / TS)]);
            acc[(2 * i + 1) % (16 / TS)] = __builtin_amdgcn_sad_u8(a[i] >> 16, 0u, acc[(2 * i + 1) % (16 / TS)]);
        } else {
            acc[i % (16 / TS)] = __builtin_amdgcn_sad_u8(a[i], 0u, acc[i % (16 / TS)]);
        }
    }
}

// One workgroup's subband of one candidate.  The span of a channel is the nt * tscr bytes from xt[c][t0 + delay]; it is
// cut into 16-byte units, P lanes (a power of two) side by side take a channel's units, 256 / P channels go in
// parallel, and a lane keeps its unit's sums in registers over all the channels it visits.  Per (channel, unit) the
// bytes are five aligned dwords (one 16-byte and one 4-byte load) shifted by v_alignbyte as in k_dedisperse; the valid
// byte range [lo, hi) of the unit -- inside [0, nsamp) of the row and inside the span -- is computed per unit and only
// a unit that is cut by it is masked.  A unit with no valid byte loads nothing.  A unit with one reads at most 19
// bytes past nsamp - 1 (inside the row's pitch, the next row or the allocation's 64-byte pad) and, before the row, the
// previous row -- or, in the very first row, nothing: those dwords are not loaded.
template <int TS>
__device__ __forceinline__ void cutout_ft_body(uint32_t *bins, const uint8_t *__restrict__ xt,
                                               const int32_t *__restrict__ chans, const int32_t *__restrict__ dl,
                                               int first, int last, int t0, int lsh, int nt, int nsamp, size_t tpitch)
{
    constexpr int NA = 16 / TS;
    const int span = nt << lsh;
    const int nu = (span + 15) >> 4;
    int P = 256;
    while ((P >> 1) >= nu) P >>= 1;
    const int slots = 256 / P, slot = threadIdx.x / P, ul = threadIdx.x % P;
    for (int u = ul; u < nu; u += P) {
        const int b0 = u << 4;
        uint32_t acc[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) acc[i] = 0u;
        for (int k = first + slot; k < last; k += slots * CUT_CU) {
            uint32_t w[CUT_CU][5];
            int lo[CUT_CU], hi[CUT_CU];
            unsigned sh[CUT_CU];
#pragma unroll
            for (int q = 0; q < CUT_CU; ++q) {
                const int kk = k + q * slots;
                lo[q] = hi[q] = 0;
                sh[q] = 0u;
#pragma unroll
                for (int i = 0; i < 5; ++i) w[q][i] = 0u;
                if (kk >= last) continue;
                const int s0 = t0 + dl[kk] + b0;                        // block sample of the unit's first byte
                const int l = max(0, -s0), h = min(16, min(nsamp - s0, span - b0));
                if (h <= l) continue;
                lo[q] = l;
                hi[q] = h;
                sh[q] = (unsigned)(s0 & 3);
                const long long off = (long long)chans[kk] * (long long)tpitch + (long long)(s0 & ~3);
                if (off >= 0) {
                    const uint32_t *p = (const uint32_t *)(xt + off);
                    const cut_u32x4 v = *(const cut_u32x4 *)p;
                    w[q][0] = v.x;
                    w[q][1] = v.y;
                    w[q][2] = v.z;
                    w[q][3] = v.w;
                    w[q][4] = p[4];
                } else {
#pragma unroll
                    for (int i = 0; i < 5; ++i)
                        if (off + 4 * i >= 0) w[q][i] = *(const uint32_t *)(xt + off + 4 * i);
                }
            }
#pragma unroll
            for (int q = 0; q < CUT_CU; ++q) {
                uint32_t a[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = __builtin_amdgcn_alignbyte(w[q][i + 1], w[q][i], sh[q]);
                if (lo[q] > 0 || hi[q] < 16) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int li = min(max(lo[q] - 4 * i, 0), 4), hj = min(max(hi[q] - 4 * i, 0), 4);
                        uint32_t m = 0u;
                        if (hj > li) m = (hj == 4 ? 0xffffffffu : (1u << (8 * hj)) - 1u) & ~((1u << (8 * li)) - 1u);
                        a[i] &= m;
                    }
                }
                cutout_add<TS>(acc, a);
            }
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int b = b0 + i * (TS == 4 ? 4 : TS);                  // first span byte of accumulator i
            if (b < span && acc[i]) atomicAdd(&bins[b >> lsh], acc[i]);
        }
    }
}

// Frequency-time cutouts: grid (subband, candidate).  req: [n][3] = DM index, peak sample, time-scrunch factor (checked
// on the host); subrun: [nsub][2] the subband's run [first, last) of chans[]; ft, fth: [n][nsub][nt].  The sums of the
// workgroup's lanes meet in nt LDS bins; the hit counts are arithmetic (the overlap of each bin, shifted by each
// channel's delay, with [0, nsamp)).
__global__ __launch_bounds__(256) void k_cutout_ft(const uint8_t *__restrict__ xt, const int32_t *__restrict__ chans,
                                                   const int32_t *__restrict__ delay, const int32_t *__restrict__ req,
                                                   const int32_t *__restrict__ subrun, uint32_t *__restrict__ ft,
                                                   uint32_t *__restrict__ fth, int nact, int nsamp, int nt, size_t tpitch)
{
    extern __shared__ uint32_t cut_bins[];
    const int sub = blockIdx.x, cand = blockIdx.y;
    const int dmi = req[3 * cand], tpk = req[3 * cand + 1], tscr = req[3 * cand + 2];
    const int lsh = 31 - __clz(tscr);
    const int t0 = tpk - ((nt / 2) << lsh);
    const int first = subrun[2 * sub], last = subrun[2 * sub + 1];
    const int32_t *dl = delay + (size_t)dmi * nact;
    for (int j = threadIdx.x; j < nt; j += 256) cut_bins[j] = 0u;
    __syncthreads();
    if (tscr == 1)
        cutout_ft_body<1>(cut_bins, xt, chans, dl, first, last, t0, lsh, nt, nsamp, tpitch);
    else if (tscr == 2)
        cutout_ft_body<2>(cut_bins, xt, chans, dl, first, last, t0, lsh, nt, nsamp, tpitch);
    else
        cutout_ft_body<4>(cut_bins, xt, chans, dl, first, last, t0, lsh, nt, nsamp, tpitch);
    __syncthreads();
    const size_t o = ((size_t)cand * gridDim.x + sub) * nt;
    for (int j = threadIdx.x; j < nt; j += 256) {
        const int b = t0 + (j << lsh);
        uint32_t n = 0u;
        for (int k = first; k < last; ++k) {
            const int s0 = b + dl[k];
            n += (uint32_t)max(min(s0 + tscr, nsamp) - max(s0, 0), 0);
        }
        ft[o + j] = cut_bins[j];
        fth[o + j] = n;
    }
}

// DM-time cutouts: grid (DM row, candidate); dt, dth: [n][ndmrow][nt].  tscr >= 4: a lane reads four consecutive
// samples of the row (one 16-byte load where all four are inside [0, tout)), tscr / 4 neighbouring lanes make a bin.
__global__ __launch_bounds__(256) void k_cutout_dt(const uint32_t *__restrict__ D, const int32_t *__restrict__ req,
                                                   uint32_t *__restrict__ dt, uint32_t *__restrict__ dth, int ndm,
                                                   int tout, int nt, size_t dpitch)
{
    const int row = blockIdx.x, cand = blockIdx.y, ndmrow = gridDim.x;
    const int dmi = req[3 * cand], tpk = req[3 * cand + 1], tscr = req[3 * cand + 2];
    const int lsh = 31 - __clz(tscr);
    const int t0 = tpk - ((nt / 2) << lsh);
    const int dm = dmi - ndmrow / 2 + row;
    const bool in = dm >= 0 && dm < ndm;
    uint32_t *out = dt + ((size_t)cand * ndmrow + row) * nt;
    uint32_t *outh = dth + ((size_t)cand * ndmrow + row) * nt;
    for (int j = threadIdx.x; j < nt; j += 256) {
        const int b = t0 + (j << lsh);
        outh[j] = in ? (uint32_t)max(min(b + tscr, tout) - max(b, 0), 0) : 0u;
        if (!in) out[j] = 0u;
    }
    if (!in) return;
    const uint32_t *x = D + (size_t)dm * dpitch;
    if (tscr < 4) {
        for (int j = threadIdx.x; j < nt; j += 256) {
            const int b = t0 + (j << lsh);
            uint32_t s = 0u;
            for (int e = 0; e < tscr; ++e)
                if (b + e >= 0 && b + e < tout) s += x[b + e];
            out[j] = s;
        }
        return;
    }
    const int g = tscr >> 2;                    // lanes per bin: 1..16, groups aligned inside a wave
    const int nq = nt * g;
    for (int base = 0; base < nq; base += 256) {
        const int i = base + threadIdx.x;
        uint32_t s = 0u;
        if (i < nq) {
            const int t = t0 + 4 * i;
            if (t >= 0 && t + 4 <= tout) {
                const cut_u32x4 v = *(const cut_u32x4 *)(x + t);
                s = v.x + v.y + v.z + v.w;
            } else {
                for (int e = 0; e < 4; ++e)
                    if (t + e >= 0 && t + e < tout) s += x[t + e];
            }
        }
        for (int o = 1; o < g; o <<= 1) s += __shfl_xor(s, o);
        if (i < nq && (i & (g - 1)) == 0) out[i >> (lsh - 2)] = s;
    }
}

// ---- giants and their clusters (definition: include/pb_hip.h, pb_search_set_giants) ----
// Integer work throughout: binary32 values are only compared (>= thresh), never combined, and a maximum over S/N is a
// maximum over giant_key of their bits.  Counts, sums, minima and maxima meet in integer atomics, whose result does
// not depend on the order of arrival; every position in a list comes from an exclusive scan.

#define GI_W PB_GIANT_WORDS   // words of a giant and of a candidate
#define GI_CU 8               // 64-sample chunks of the write pass whose loads are in flight together
#define GI_SEG 16             // chunks one wave of the count pass takes

// S/N bits -> unsigned key in the order of the binary32 comparison (-0 equals +0; never given a NaN: a NaN is not hot)
__device__ __forceinline__ uint32_t giant_key(uint32_t b)
{
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// m: hot mask of a 64-sample chunk (bit i = sample 64 c + i), p: the chunk before it.  The hot samples that start a
// run: those with no hot sample among the sep samples before them.  `near` = OR of m << k, k = 1 .. sep, built by
// doubling along the bits of sep, plus what the previous chunk's last sep samples reach: its highest hot bit j covers
// the positions i <= j + sep - 64.
__device__ __forceinline__ uint64_t giant_starts(uint64_t m, uint64_t p, int sep)
{
    uint64_t near = m << 1;
    int c = 1;
    for (int b = 30 - __clz(sep); b >= 0; --b) {
        near |= near << c;
        c <<= 1;
        if ((sep >> b) & 1) {
            ++c;
            near |= m << c;
        }
    }
    const int n = p ? sep - __clzll((long long)p) : 0;
    if (n > 0) near |= n >= 64 ? ~0ull : (1ull << n) - 1ull;
    return m & ~near;
}

// one chunk's sample of this lane, a NaN (never hot) outside [t_lo, t_hi)
__device__ __forceinline__ float giant_load(const float *__restrict__ row, int t, int t_lo, int t_hi)
{
    return (t >= t_lo && t < t_hi) ? row[t] : __int_as_float(0x7fc00000);
}

// Count pass: giants per series = run starts, which a chunk and the chunk before it decide.  grid (stretches of
// 4 GI_SEG chunks from t_lo's chunk on, series); a wave takes GI_SEG chunks and adds its count to cnt[series].
__global__ __launch_bounds__(256) void k_giant_count(const float *__restrict__ snr, int32_t *__restrict__ cnt, int t_lo,
                                                     int t_hi, float thresh, int sep, size_t dpitch)
{
    const int lane = threadIdx.x & 63;
    const int c_lo = t_lo >> 6, c_end = (t_hi + 63) >> 6;
    const int c0 = c_lo + (blockIdx.x * 4 + (threadIdx.x >> 6)) * GI_SEG;
    if (c0 >= c_end) return;                                            // (the whole wave)
    const float *row = snr + (size_t)blockIdx.y * dpitch;
    float v[GI_SEG];
#pragma unroll
    for (int j = 0; j < GI_SEG; ++j) v[j] = giant_load(row, (c0 + j) * 64 + lane, t_lo, t_hi);
    uint64_t p = c0 > c_lo ? __ballot(giant_load(row, (c0 - 1) * 64 + lane, t_lo, t_hi) >= thresh) : 0ull;
    int n = 0;
#pragma unroll
    for (int j = 0; j < GI_SEG; ++j) {
        const uint64_t m = __ballot(v[j] >= thresh);
        n += __popcll(giant_starts(m, p, sep));
        p = m;
    }
    if (lane == 0 && n) atomicAdd(&cnt[blockIdx.y], n);
}

// Exclusive sums off[0 .. n] of cnt[0 .. n) by one workgroup; *total = off[n], *over = (off[n] > cap) where asked for.
__global__ __launch_bounds__(256) void k_giant_scan(const int32_t *__restrict__ cnt, int32_t *__restrict__ off, int n,
                                                    int32_t *__restrict__ total, int32_t *__restrict__ over, int cap)
{
    __shared__ int wsum[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int run = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < n ? cnt[i] : 0;
        int inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(inc, o);
            if (lane >= o) inc += y;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) woff += wsum[w];
            tot += wsum[w];
        }
        if (i < n) off[i] = run + woff + inc - v;
        run += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        off[n] = run;
        if (total) *total = run;
        if (over) *over = run > cap ? 1 : 0;
    }
}

// the largest key among the lanes of `piece` (the other lanes count as 0)
__device__ __forceinline__ uint64_t giant_wave_max(uint64_t key, uint64_t piece, int lane)
{
    uint64_t k = ((piece >> lane) & 1ull) ? key : 0ull;
    if (__popcll(piece) == 1) return __shfl(k, __builtin_ctzll(piece));
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t y = __shfl_xor(k, o);
        k = y > k ? y : k;
    }
    return k;
}

// Write pass, a wave per series (nothing is read for a series without giants, nothing at all after an overflow): the
// chunks in order, GI_CU loads in flight; the run that is open lives in wave-uniform registers -- begin, last hot
// sample, hot samples, the largest (S/N key, ~t) -- and is written as giant row_off[series] + k when the next run
// starts or the range ends.  A chunk's hot samples below its first run start continue the open run; each start bit
// opens a run that holds the chunk's hot samples up to the next start bit.
__global__ __launch_bounds__(256) void k_giant_write(const float *__restrict__ snr, const uint8_t *__restrict__ wid,
                                                     const int32_t *__restrict__ row_off, const int32_t *__restrict__ ctl,
                                                     int32_t *__restrict__ giants, int32_t *__restrict__ lab, int ndm,
                                                     int t_lo, int t_hi, float thresh, int sep, int cap, size_t dpitch)
{
    const int d = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (d >= ndm || ctl[1]) return;                                     // (the whole wave)
    int out = row_off[d];
    const int out_end = row_off[d + 1];
    if (out == out_end) return;
    const float *row = snr + (size_t)d * dpitch;
    const uint8_t *wrow = wid + (size_t)d * dpitch;
    const int c_lo = t_lo >> 6, c_end = (t_hi + 63) >> 6;
    bool open = false;
    int begin = 0, last = 0, npts = 0;
    uint64_t best = 0ull, p = 0ull;
    auto emit = [&]() {
        if (lane == 0 && out < out_end && out < cap) {
            const int peak = (int)(0xffffffffu - (uint32_t)best);
            int4 *g = (int4 *)(giants + (size_t)out * GI_W);
            g[0] = make_int4(d, begin, last + 1, npts);
            g[1] = make_int4(peak, __float_as_int(row[peak]), (int)wrow[peak], out);
            lab[out] = out;
        }
        ++out;
    };
    for (int cb = c_lo; cb < c_end; cb += GI_CU) {
        float v[GI_CU];
#pragma unroll
        for (int j = 0; j < GI_CU; ++j) v[j] = giant_load(row, (cb + j) * 64 + lane, t_lo, t_hi);
#pragma unroll
        for (int j = 0; j < GI_CU; ++j) {
            const bool hot = v[j] >= thresh;
            const uint64_t m = __ballot(hot);
            if (m == 0ull) {
                p = 0ull;
                continue;
            }
            const int base = (cb + j) * 64;
            const uint64_t key = ((uint64_t)giant_key((uint32_t)__float_as_int(v[j])) << 32) |
                                 (uint64_t)(0xffffffffu - (uint32_t)(base + lane));
            uint64_t s = giant_starts(m, p, sep);
            p = m;
            uint64_t piece = m & (s ? (1ull << __builtin_ctzll(s)) - 1ull : ~0ull);
            if (piece) {                                                // (a run is open: these samples are no starts)
                const uint64_t k = giant_wave_max(key, piece, lane);
                best = k > best ? k : best;
                npts += __popcll(piece);
                last = base + 63 - __clzll((long long)piece);
            }
            while (s) {                                                 // at most 64 start bits
                const int i = __builtin_ctzll(s);
                s &= s - 1ull;
                if (open) emit();
                piece = m & (s ? (1ull << __builtin_ctzll(s)) - 1ull : ~0ull) & ~((1ull << i) - 1ull);
                open = true;
                begin = base + i;
                npts = __popcll(piece);
                last = base + 63 - __clzll((long long)piece);
                best = giant_wave_max(key, piece, lane);
            }
        }
    }
    if (open) emit();
}

__device__ __forceinline__ int giant_lab_load(const int32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Hooking, a wave per giant a, its lanes over the rows dmi_a - 1 down to dmi_a - sep_dm (every link is met once, from
// its later giant).  In a row begin and end ascend, so a's partners are a window: the first b with
// end_b + sep_time > begin_a by bisection, then on while begin_b < end_a + sep_time.  A link whose two labels differ
// hangs the larger label under the smaller (atomicMin) and raises ctl[3].  Labels only ever fall, and stay inside the
// cluster, so reading one that is being changed is harmless: the sweep after it looks again.
__global__ __launch_bounds__(256) void k_giant_hook(const int32_t *__restrict__ giants, const int32_t *__restrict__ row_off,
                                                    int32_t *__restrict__ lab, int32_t *__restrict__ ctl, int G,
                                                    int sep_time, int sep_dm, int sep_filter)
{
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= G) return;
    const int4 ga = *(const int4 *)(giants + (size_t)a * GI_W);         // dmi, begin, end, npts
    const int tf = giants[(size_t)a * GI_W + 6];
    const int r_lo = ga.x - sep_dm > 0 ? ga.x - sep_dm : 0;
    int la = giant_lab_load(lab + a);
    bool changed = false;
    for (int r = ga.x - 1 - lane; r >= r_lo; r -= 64) {
        int lo = row_off[r], hi = row_off[r + 1];
        const int row_end = hi;
        for (int it = 0; it < 32 && lo < hi; ++it) {
            const int mid = (lo + hi) >> 1;
            if (giants[(size_t)mid * GI_W + 2] + sep_time > ga.y)
                hi = mid;
            else
                lo = mid + 1;
        }
        for (int b = lo; b < row_end; ++b) {
            const int4 gb = *(const int4 *)(giants + (size_t)b * GI_W);
            if (!(gb.y < ga.z + sep_time)) break;
            const int df = giants[(size_t)b * GI_W + 6] - tf;
            if ((df < 0 ? -df : df) > sep_filter) continue;
            const int lb = giant_lab_load(lab + b);
            if (lb != la) {
                atomicMin(&lab[lb > la ? lb : la], lb < la ? lb : la);
                la = lb < la ? lb : la;
                changed = true;
            }
        }
    }
    if (changed) __hip_atomic_store(ctl + 3, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pointer jumping: every giant takes the root of its chain (a chain is shorter than G)
__global__ __launch_bounds__(256) void k_giant_jump(int32_t *__restrict__ lab, int G)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= G) return;
    int r = giant_lab_load(lab + a);
    for (int i = 0; i < G; ++i) {
        const int rr = giant_lab_load(lab + r);
        if (rr == r) break;
        r = rr;
    }
    __hip_atomic_store(lab + a, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Merge, first half: a lane per giant.  Its label goes into its record; under its label meet the largest
// (S/N key, ~index) -- so of equal S/N the smallest index wins --, the member count, the points, INT_MAX - begin and
// end.  Neighbouring giants mostly share a label: a wave whose giants all do reduces first and sends one atomic of
// each kind.  tile_cnt[workgroup] = the roots (label == index) among its 256 giants.
__global__ __launch_bounds__(256) void k_giant_reduce(int32_t *__restrict__ giants, const int32_t *__restrict__ lab,
                                                      unsigned long long *__restrict__ best, int32_t *__restrict__ acc,
                                                      int32_t *__restrict__ tile_cnt, int G)
{
    __shared__ int nroot[4];
    const int a = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool live = a < G;
    int r = -1, members = 0, npts = 0, nb = 0, e = 0;
    unsigned long long key = 0ull;
    if (live) {
        int32_t *g = giants + (size_t)a * GI_W;
        r = lab[a];
        g[7] = r;
        key = ((unsigned long long)giant_key((uint32_t)g[5]) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)a);
        members = 1;
        npts = g[3];
        nb = 0x7fffffff - g[1];
        e = g[2];
    }
    const int r0 = __shfl(r, 0);
    if (__all(r == r0 || !live)) {                                      // (lane 0 is live in every wave that has a live lane)
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long yk = __shfl_xor(key, o);
            key = yk > key ? yk : key;
            members += __shfl_xor(members, o);
            npts += __shfl_xor(npts, o);
            nb = max(nb, __shfl_xor(nb, o));
            e = max(e, __shfl_xor(e, o));
        }
        if (lane != 0) r = -1;
    }
    if (r >= 0 && members > 0) {
        atomicMax(&best[r], key);
        atomicAdd(&acc[4 * (size_t)r], members);
        atomicAdd(&acc[4 * (size_t)r + 1], npts);
        atomicMax(&acc[4 * (size_t)r + 2], nb);
        atomicMax(&acc[4 * (size_t)r + 3], e);
    }
    const uint64_t roots = __ballot(live && lab[live ? a : 0] == a);
    if (lane == 0) nroot[threadIdx.x >> 6] = __popcll(roots);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = nroot[0] + nroot[1] + nroot[2] + nroot[3];
}

// Merge, second half: the roots in index order = the clusters in label order; root a is candidate
// tile_off[workgroup] + its rank among the workgroup's roots.  A candidate: S/N bits, peak, tfilt, dmi of the winning
// member, members, points, smallest begin, largest end.
__global__ __launch_bounds__(256) void k_giant_cands(const int32_t *__restrict__ giants, const int32_t *__restrict__ lab,
                                                     const unsigned long long *__restrict__ best,
                                                     const int32_t *__restrict__ acc, const int32_t *__restrict__ tile_off,
                                                     int32_t *__restrict__ cands, int G, int cap)
{
    __shared__ int nroot[4];
    const int a = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool root = a < G && lab[a < G ? a : 0] == a;
    const uint64_t roots = __ballot(root);
    if (lane == 0) nroot[wave] = __popcll(roots);
    __syncthreads();
    if (!root) return;
    int idx = tile_off[blockIdx.x] + __popcll(roots & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) idx += nroot[w];
    if (idx >= cap) return;
    const int w = (int)(0xffffffffu - (uint32_t)best[a]);                // (a root is a member of its own cluster: best[a] is set)
    if (w < 0 || w >= G) return;
    const int32_t *g = giants + (size_t)w * GI_W;
    const int32_t *c = acc + 4 * (size_t)a;
    int4 *o = (int4 *)(cands + (size_t)idx * GI_W);
    o[0] = make_int4(g[5], g[4], g[6], g[0]);
    o[1] = make_int4(c[0], c[1], 0x7fffffff - c[2], c[3]);
}

// ---- refinement of a candidate's DM, width and S/N (definition: include/pb_hip.h, pb_search_set_refine) ----

#define RF_MAXL 2048      // samples of one fine series about a peak, 2 (H + M); the statistics hold it in LDS
#define RF_CH 1024        // channels whose delays are in LDS together
#define RF_CU 4           // channels whose loads are in flight together

// fine trial k of a request: DM (double)dm_lo + k (double)dm_step; evaluated only inside [0, the grid's last DM]
__device__ __forceinline__ bool refine_trial(const int32_t *__restrict__ reqi, const float *__restrict__ reqf, int cand,
                                             int k, double dm_last, double &dm)
{
    dm = (double)reqf[2 * cand] + (double)k * (double)reqf[2 * cand + 1];
    return reqi[4 * cand + 2] == 0 && dm >= 0.0 && dm <= dm_last;
}

// The fine series: grid (fine trial, request).  series[cand][k][j] = q_k[t_pk - HM + j] = the sum over the unzapped
// channels of xt[c][t + delay_k[c]] for t in [0, tout), 0 outside (and all 0 for a trial or request that is not
// evaluated).  A lane takes 8 consecutive samples as in k_dedisperse -- three aligned dwords shifted by v_alignbyte,
// packed 16-bit sums widened before they can overflow -- P = ceil(L / 8) lanes side by side cover the series and the
// 256 / P groups of them share the channels; the groups' sums meet in LDS.  The delays of RF_CH channels at a time are
// made in LDS by the whole workgroup with delay_samples, the function the trial DMs' table is made with.
// Reads: a lane with a sample in [0, tout) reads at most 11 bytes past t + delay <= tout - 1 + max_delay = nsamp - 1 (the
// trial's DM is not above the grid's last, and the delay grows with the DM), as k_dedisperse does; what it reads for
// its samples outside [0, tout) -- the previous row, the pad -- is never written out; a dword before the allocation
// (first row, t < 0) is not loaded.  So no byte at or beyond nsamp is ever summed into an output.
__global__ __launch_bounds__(256) void k_refine_series(const uint8_t *__restrict__ xt, const int32_t *__restrict__ chans,
                                                       const double *__restrict__ gterm, const int32_t *__restrict__ reqi,
                                                       const float *__restrict__ reqf, uint32_t *__restrict__ series,
                                                       int nact, int tout, int L, int HM, double tsamp, double dm_last,
                                                       size_t tpitch)
{
    __shared__ int32_t dl[RF_CH];
    __shared__ uint32_t part[256 * 8];
    const int k = blockIdx.x, cand = blockIdx.y;
    uint32_t *out = series + ((size_t)cand * gridDim.x + k) * L;
    double dm;
    if (!refine_trial(reqi, reqf, cand, k, dm_last, dm)) {              // the same in every lane
        for (int j = threadIdx.x; j < L; j += 256) out[j] = 0u;
        return;
    }
    const int P = (L + 7) >> 3, G = 256 / P;                            // P <= 256: pb_search_set_refine
    const int grp = threadIdx.x / P, ul = threadIdx.x % P;
    const int t0 = reqi[4 * cand] - HM;
    const int ts = t0 + 8 * ul;
    const bool live = grp < G && ts < tout && ts + 8 > 0;
    uint32_t lo[2] = {0u, 0u}, hi[2] = {0u, 0u}, acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0u;
    auto flush = [&]() {
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            acc[4 * w + 0] += lo[w] & 0xffffu;
            acc[4 * w + 1] += hi[w] & 0xffffu;
            acc[4 * w + 2] += lo[w] >> 16;
            acc[4 * w + 3] += hi[w] >> 16;
            lo[w] = hi[w] = 0u;
        }
    };
    for (int c0 = 0; c0 < nact; c0 += RF_CH) {
        const int nc = min(RF_CH, nact - c0);
        __syncthreads();
        for (int i = threadIdx.x; i < nc; i += 256) dl[i] = delay_samples(dm, gterm[c0 + i], tsamp);
        __syncthreads();
        if (!live) continue;
        int since = 0;
        for (int i = grp; i < nc; i += G * RF_CU) {
            uint32_t w[RF_CU][3];
            unsigned sh[RF_CU];
#pragma unroll
            for (int q = 0; q < RF_CU; ++q) {
                const int ii = i + q * G;
                w[q][0] = w[q][1] = w[q][2] = 0u;
                sh[q] = 0u;
                if (ii >= nc) continue;
                const int s0 = ts + dl[ii];                             // block sample of the lane's first byte
                sh[q] = (unsigned)(s0 & 3);
                const long long off = (long long)chans[c0 + ii] * (long long)tpitch + (long long)(s0 & ~3);
                if (off >= 0) {
                    const uint32_t *p = (const uint32_t *)(xt + off);
                    w[q][0] = p[0];
                    w[q][1] = p[1];
                    w[q][2] = p[2];
                } else {
#pragma unroll
                    for (int e = 0; e < 3; ++e)
                        if (off + 4 * e >= 0) w[q][e] = *(const uint32_t *)(xt + off + 4 * e);
                }
            }
#pragma unroll
            for (int q = 0; q < RF_CU; ++q) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const uint32_t a = __builtin_amdgcn_alignbyte(w[q][e + 1], w[q][e], sh[q]);
                    lo[e] += a & 0x00ff00ffu;
                    hi[e] += (a >> 8) & 0x00ff00ffu;
                }
            }
            since += RF_CU;
            if (since >= 240) {                                         // 16-bit sums: at most 257 channels of 255
                flush();
                since = 0;
            }
        }
        flush();
    }
    if (grp < G) {
#pragma unroll
        for (int i = 0; i < 8; ++i) part[(grp * P + ul) * 8 + i] = acc[i];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < L; j += 256) {
        uint32_t v = 0u;
        for (int g = 0; g < G; ++g) v += part[g * P * 8 + j];
        const int t = t0 + j;
        out[j] = (t >= 0 && t < tout) ? v : 0u;
    }
}

__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t *sh)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

__device__ __forceinline__ uint64_t block_max_u64(uint64_t v, uint64_t *sh)
{
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t y = (uint64_t)__shfl_down((unsigned long long)v, o);
        v = y > v ? y : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint64_t a = sh[0] > sh[1] ? sh[0] : sh[1], b = sh[2] > sh[3] ? sh[2] : sh[3];
    return a > b ? a : b;
}

// a double as a u64 that orders the same way (no NaN); never 0
__device__ __forceinline__ uint64_t ordered_key(double v)
{
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// src[0 .. n) -> dst ascending, both in LDS: every element counts the elements that go before it
__device__ __forceinline__ void refine_sort(const uint32_t *src, int n, uint32_t *dst)
{
    for (int i = threadIdx.x; i < n; i += 256) {
        const uint32_t v = src[i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t u = src[j];
            r += (u < v) || (u == v && j < i);
        }
        dst[r] = v;
    }
    __syncthreads();
}

// first index in (i, n) whose value exceeds s[i] + v, n if none (s ascending)
__device__ __forceinline__ int refine_upper(const uint32_t *s, int n, int i, uint32_t v)
{
    const uint64_t lim = (uint64_t)s[i] + v;
    int lo = i + 1, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint64_t)s[mid] <= lim) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// number of pairs i < j with s[j] - s[i] <= v (the same in every lane)
__device__ __forceinline__ uint32_t refine_pairs_le(const uint32_t *s, int n, uint32_t v, uint32_t *sh)
{
    uint32_t c = 0;
    for (int i = threadIdx.x; i < n; i += 256) c += (uint32_t)(refine_upper(s, n, i, v) - i - 1);
    return block_sum_u32(c, sh);
}

// Qn of the ascending s[0 .. n), n >= 2: 2.2219 x the 25th percentile of the np = n (n - 1) / 2 absolute pair differences,
// interpolated as np.percentile does -- position (np - 1) / 4 = r + f / 4, value d[r] + (f / 4) (d[r + 1] - d[r]), exact
// in double for integers.  d[r] by bisection on the value over the count of pairs at or below it; d[r + 1] is d[r] when
// more than r + 1 pairs are at or below d[r], else the smallest difference above it.  Uniform over the workgroup.
__device__ __forceinline__ double refine_qn(const uint32_t *s, int n, uint32_t *sh, uint64_t *sh64)
{
    const uint32_t np = (uint32_t)n * (uint32_t)(n - 1) / 2u, r = (np - 1u) >> 2, f = (np - 1u) & 3u;
    uint32_t lo = 0u, hi = s[n - 1] - s[0];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (refine_pairs_le(s, n, mid, sh) >= r + 1u) hi = mid; else lo = mid + 1u;
    }
    uint32_t dhi = lo;
    if (f && refine_pairs_le(s, n, lo, sh) < r + 2u) {
        uint64_t best = 0;                                              // ~(smallest difference above lo)
        for (int i = threadIdx.x; i < n; i += 256) {
            const int j = refine_upper(s, n, i, lo);
            if (j < n) {
                const uint64_t key = ~(uint64_t)(s[j] - s[i]);
                best = key > best ? key : best;
            }
        }
        dhi = (uint32_t)~block_max_u64(best, sh64);
    }
    return 2.2219 * ((double)lo + 0.25 * (double)f * ((double)dhi - (double)lo));
}

// The DM pass, one workgroup per (fine trial, request): the window of the fine series in LDS, its median and Qn from a
// sorted copy, the largest top-hat smoothed value with tophat_smooth's edge ramps at the ends of the whole series.
__global__ __launch_bounds__(256) void k_refine_dm(const uint32_t *__restrict__ series, const int32_t *__restrict__ reqi,
                                                   const float *__restrict__ reqf, double *__restrict__ sn_dm, int tout,
                                                   int H, int M, double dm_last)
{
    __shared__ uint32_t ext[RF_MAXL], srt[RF_MAXL];
    __shared__ uint32_t sh[4];
    __shared__ uint64_t sh64[4];
    const int k = blockIdx.x, cand = blockIdx.y, L = 2 * (H + M);
    double dm;
    if (!refine_trial(reqi, reqf, cand, k, dm_last, dm)) {              // the same in every lane
        if (threadIdx.x == 0) sn_dm[(size_t)cand * gridDim.x + k] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const int tpk = reqi[4 * cand], w = reqi[4 * cand + 1];
    const int i0 = max(0, tpk - H), i1 = min(tout, tpk + H), n = i1 - i0, e0 = i0 - (tpk - H - M);
    const uint32_t *q = series + ((size_t)cand * gridDim.x + k) * L;
    for (int j = threadIdx.x; j < L; j += 256) ext[j] = q[j];
    __syncthreads();
    refine_sort(ext + e0, n, srt);
    const uint32_t med2 = srt[(n - 1) >> 1] + srt[n >> 1];
    const double qn = refine_qn(srt, n, sh, sh64);
    uint64_t key = 0;                                                   // the values are >= 0: their bits order as they do
    for (int a = threadIdx.x; a < n; a += 256) {
        const int t = i0 + a, h = min(w >> 1, min(t, tout - 1 - t));    // h <= M: the terms are inside ext
        uint64_t sum = 0;
        for (int e = e0 + a - h; e <= e0 + a + h; ++e) sum += ext[e];
        const uint64_t b = (uint64_t)__double_as_longlong((double)sum / (double)(2 * h + 1));
        key = b > key ? b : key;
    }
    key = block_max_u64(key, sh64);
    if (threadIdx.x == 0) {
        const double mx = __longlong_as_double((long long)key), med = 0.5 * (double)med2;
        sn_dm[(size_t)cand * gridDim.x + k] = qn > 0.0 ? (mx - med) / (qn / sqrt((double)w)) : 0.0;
    }
}

// The width pass, one workgroup per request: kbest = the first maximum of the request's sn_dm (NaN never wins), then on
// that trial's series the off-pulse median and Qn and, for each odd width, the first maximum of the running mean.
__global__ __launch_bounds__(256) void k_refine_width(const uint32_t *__restrict__ series, const int32_t *__restrict__ reqi,
                                                      const double *__restrict__ sn_dm, int32_t *__restrict__ kbest,
                                                      double *__restrict__ opt_sn, int32_t *__restrict__ opt_loc, int tout,
                                                      int H, int M, int nstep, int nw)
{
    __shared__ uint32_t ext[RF_MAXL], off[RF_MAXL], srt[RF_MAXL];
    __shared__ uint32_t sh[4];
    __shared__ uint64_t sh64[4];
    const int cand = blockIdx.x, L = 2 * (H + M);
    uint64_t vkey = 0;
    if (reqi[4 * cand + 2] == 0) {
        for (int k = threadIdx.x; k < nstep; k += 256) {
            const double v = sn_dm[(size_t)cand * nstep + k];
            if (v == v) {
                const uint64_t o = ordered_key(v);
                vkey = o > vkey ? o : vkey;
            }
        }
    }
    vkey = block_max_u64(vkey, sh64);
    if (vkey == 0) {                                                    // nothing evaluated; the same in every lane
        if (threadIdx.x == 0) kbest[cand] = -1;
        for (int iw = threadIdx.x; iw < nw; iw += 256) {
            opt_sn[(size_t)cand * nw + iw] = __longlong_as_double(0x7ff8000000000000ll);
            opt_loc[(size_t)cand * nw + iw] = -1;
        }
        return;
    }
    uint64_t ikey = 0;
    for (int k = threadIdx.x; k < nstep; k += 256) {
        const double v = sn_dm[(size_t)cand * nstep + k];
        if (v == v && ordered_key(v) == vkey) {
            const uint64_t o = ~(uint64_t)k;
            ikey = o > ikey ? o : ikey;
        }
    }
    const int kb = (int)~block_max_u64(ikey, sh64);
    if (threadIdx.x == 0) kbest[cand] = kb;
    const int tpk = reqi[4 * cand];
    const int i0 = max(0, tpk - H), i1 = min(tout, tpk + H), n = i1 - i0, e0 = i0 - (tpk - H - M);
    const uint32_t *q = series + ((size_t)cand * nstep + kb) * L;
    for (int j = threadIdx.x; j < L; j += 256) ext[j] = q[j];
    __syncthreads();
    const int n4 = n / 4, n34 = 3 * n / 4, noff = n4 + n - n34;          // int(0.25 n), int(0.75 n)
    for (int j = threadIdx.x; j < noff; j += 256) off[j] = j < n4 ? ext[e0 + j] : ext[e0 + n34 + (j - n4)];
    __syncthreads();
    refine_sort(off, noff, srt);
    const double med = 0.5 * (double)(srt[(noff - 1) >> 1] + srt[noff >> 1]);
    const double qn = refine_qn(srt, noff, sh, sh64);
    for (int iw = 0; iw < nw; ++iw) {
        const int w = 2 * iw + 1;
        uint64_t key = 0;                                               // (sum, first position) as one number
        for (int a = w + threadIdx.x; a < n - w; a += 256) {
            uint32_t sum = 0;                                           // below 2^32: pb_search_set_refine
            for (int e = e0 + a - iw; e <= e0 + a + iw; ++e) sum += ext[e];
            const uint64_t o = ((uint64_t)sum << 32) | (uint64_t)(0xffffffffu - (uint32_t)a);
            key = o > key ? o : key;
        }
        key = block_max_u64(key, sh64);
        if (threadIdx.x == 0) {
            const double mean = (double)(uint32_t)(key >> 32) / (double)w;
            opt_loc[(size_t)cand * nw + iw] = (int32_t)(0xffffffffu - (uint32_t)key);
            opt_sn[(size_t)cand * nw + iw] = qn > 0.0 ? (mean - med) / qn * sqrt((double)w) : 0.0;
        }
    }
}

extern "C" const char *pb_search_last_error(const pb_search *s) { return s ? s->err.c_str() : g_search_err.c_str(); }

static int search_create(int device, int nchan, int max_samples, float fch1_mhz, float foff_mhz, float tsamp_s,
                         const std::vector<double> &dms, int boxcar_max, const int *zap_ranges, int nzap,
                         pb_search **out);

extern "C" int pb_search_create(int device, int nchan, int max_samples, float fch1_mhz, float foff_mhz, float tsamp_s,
                                float dm_min, float dm_max, float dm_step, int boxcar_max, const int *zap_ranges,
                                int nzap, pb_search **out)
{
    if (!out || !(dm_step > 0) || dm_max < dm_min) {
        g_search_err = "pb_search_create: bad argument";
        return PB_EINVAL;
    }
    const int ndm = (int)floor((dm_max - dm_min) / dm_step + 1e-6) + 1;
    std::vector<double> dms(ndm);
    for (int i = 0; i < ndm; ++i) dms[i] = (double)dm_min + (double)i * (double)dm_step;
    return search_create(device, nchan, max_samples, fch1_mhz, foff_mhz, tsamp_s, dms, boxcar_max, zap_ranges, nzap, out);
}

// The same over an explicit list of trial DMs (ascending), e.g. a tolerance-spaced one
extern "C" int pb_search_create_list(int device, int nchan, int max_samples, float fch1_mhz, float foff_mhz,
                                     float tsamp_s, const float *dm_list, int ndm, int boxcar_max,
                                     const int *zap_ranges, int nzap, pb_search **out)
{
    if (!out || !dm_list || ndm < 1) {
        g_search_err = "pb_search_create_list: bad argument";
        return PB_EINVAL;
    }
    std::vector<double> dms(dm_list, dm_list + ndm);
    for (int i = 1; i < ndm; ++i)
        if (!(dms[i] > dms[i - 1])) {
            g_search_err = "pb_search_create_list: the DM list must be strictly ascending";
            return PB_EINVAL;
        }
    return search_create(device, nchan, max_samples, fch1_mhz, foff_mhz, tsamp_s, dms, boxcar_max, zap_ranges, nzap, out);
}

static int search_create(int device, int nchan, int max_samples, float fch1_mhz, float foff_mhz, float tsamp_s,
                         const std::vector<double> &dms, int boxcar_max, const int *zap_ranges, int nzap,
                         pb_search **out)
{
    const float dm_min = (float)dms.front();
    if (!out || nchan < 1 || max_samples < 64 || boxcar_max < 1) {
        g_search_err = "pb_search_create: bad argument";
        return PB_EINVAL;
    }
    if (!(dm_min >= 0) || device < 0) {
        // a negative DM would give negative delays (reads before the block); a negative device goes to hipSetDevice
        g_search_err = "pb_search_create: dm_min and device must be >= 0";
        return PB_EINVAL;
    }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev) {
        g_search_err = "pb_search_create: no HIP device (no CPU fallback)";
        return PB_EHIP;
    }
    pb_search *s = new pb_search();
    s->device = device;
    s->nchan = nchan;
    s->max_samples = max_samples;
    s->fch1 = fch1_mhz;
    s->foff = foff_mhz;
    s->tsamp = tsamp_s;
    s->dm_min = dm_min;
    s->dm_step = dms.size() > 1 ? (float)(dms[1] - dms[0]) : 0.f;
    s->ndm = (int)dms.size();
    s->nbox = 0;
    while ((1 << s->nbox) <= boxcar_max) s->nbox++;
    s->d_codes = s->d_xt = s->d_wid = nullptr;
    s->d_delay = nullptr;
    s->d_chans = nullptr;
    s->d_D = nullptr;
    s->d_stats = s->d_snr = nullptr;
    s->stream = nullptr;
    s->d_P = nullptr;
    s->d_peaks = nullptr;
    s->max_peaks = 1 << 20;
    s->baseline = 0;
    s->last_tout = 0;
    for (int i = 0; i < 6; ++i) s->ms[i] = 0.f;
    for (int i = 0; i < 7; ++i) s->ev[i] = nullptr;
    s->rfi_narrow = s->rfi_broad = 0;
    s->rfi_tol = 5.0f;
    s->rfi_nbox = 5;
    s->last_nsamp = s->rfi_ran = 0;
    s->d_zdelay = s->d_tlist = nullptr;
    s->d_med = s->d_zwid = nullptr;
    s->d_z = nullptr;
    s->d_zP = nullptr;
    s->d_zstats = s->d_zsnr = nullptr;
    s->d_rcnt = nullptr;
    s->ev_rfi = nullptr;
    s->n_narrow = 0;
    s->n_broad = 0;
    s->rfi_ms = 0.f;
    s->cut_nsub = s->cut_nt = s->cut_ndmrow = s->cut_max = 0;
    s->d_cut_req = s->d_cut_sub = nullptr;
    s->d_cut = s->h_cut = nullptr;
    for (int i = 0; i < 3; ++i) s->ev_cut[i] = nullptr;
    s->cut_ms[0] = s->cut_ms[1] = 0.f;
    s->dm_last = dms.back();
    s->rf_nstep = s->rf_H = s->rf_wmax = s->rf_max = 0;
    s->d_rf_g = s->d_rf_out = s->h_rf = nullptr;
    s->d_rf_reqi = nullptr;
    s->d_rf_reqf = nullptr;
    for (int i = 0; i < 3; ++i) s->ev_rf[i] = nullptr;
    s->rf_ms[0] = s->rf_ms[1] = 0.f;
    s->gi_tout = s->gi_sep_time = s->gi_sep_dm = s->gi_sep_filter = s->gi_max = s->gi_last = s->gi_sweeps = 0;
    s->d_gi_cnt = s->d_gi_row = s->d_gi = s->d_gi_lab = s->d_gi_acc = s->d_gi_tile = s->d_gi_out = s->h_gi = nullptr;
    s->d_gi_best = nullptr;
    for (int i = 0; i < 4; ++i) s->ev_gi[i] = nullptr;
    s->gi_ms[0] = s->gi_ms[1] = s->gi_ms[2] = 0.f;
    // delay table in double on the host; the top of the band (highest frequency) is the reference
    std::vector<int32_t> chans;
    for (int c = 0; c < nchan; ++c) {
        bool zap = false;
        for (int z = 0; z < nzap; ++z)
            if (c >= zap_ranges[2 * z] && c < zap_ranges[2 * z + 1]) zap = true;
        if (!zap) chans.push_back(c);
    }
    s->nact = (int)chans.size();
    if (s->nact == 0) {
        g_search_err = "pb_search_create: every channel is zapped";
        delete s;
        return PB_EINVAL;
    }
    std::vector<int32_t> delay((size_t)s->ndm * s->nact);
    const double ftop = foff_mhz < 0 ? fch1_mhz : fch1_mhz + (nchan - 1) * foff_mhz;
    s->ftop = ftop;
    int maxd = 0;
    for (int i = 0; i < s->ndm; ++i) {
        const double dm = dms[i];
        for (int k = 0; k < s->nact; ++k) {
            const double f = (double)fch1_mhz + (double)chans[k] * (double)foff_mhz;
            const int32_t di = delay_samples(dm, delay_chan_term(f, ftop), (double)tsamp_s);
            delay[(size_t)i * s->nact + k] = di;
            if (di > maxd) maxd = di;
        }
    }
    s->max_delay = maxd;
    s->tpitch = ((size_t)max_samples + 63) / 64 * 64;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_codes, (size_t)max_samples * nchan);
    // + 64: the dedispersion kernel fetches whole dwords around its 8 samples (up to 11 bytes past the last one)
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_xt, s->tpitch * nchan + 64);
    if (e == hipSuccess) e = hipMemset(s->d_xt, 0, s->tpitch * nchan + 64);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_delay, delay.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_chans, chans.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(s->d_chans, chans.data(), chans.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_D, (size_t)s->ndm * s->tpitch * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_stats, (size_t)s->ndm * 2 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_snr, (size_t)s->ndm * s->tpitch * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_wid, (size_t)s->ndm * s->tpitch);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_P, (size_t)s->ndm * (s->tpitch + 8) * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_peaks, (size_t)(1 + 4 * s->max_peaks) * sizeof(int32_t));
    for (int i = 0; i < 7 && e == hipSuccess; ++i) e = hipEventCreate(&s->ev[i]);
    if (e == hipSuccess) e = hipMemcpy(s->d_delay, delay.data(), delay.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        g_search_err = std::string("pb_search_create: ") + hipGetErrorString(e);
        pb_search_destroy(s);
        return PB_EHIP;
    }
    *out = s;
    return PB_OK;
}

static void cutouts_free(pb_search *s)
{
    if (s->d_cut_req) (void)hipFree(s->d_cut_req);
    if (s->d_cut_sub) (void)hipFree(s->d_cut_sub);
    if (s->d_cut) (void)hipFree(s->d_cut);
    if (s->h_cut) (void)hipHostFree(s->h_cut);
    for (int i = 0; i < 3; ++i) {
        if (s->ev_cut[i]) (void)hipEventDestroy(s->ev_cut[i]);
        s->ev_cut[i] = nullptr;
    }
    s->d_cut_req = s->d_cut_sub = nullptr;
    s->d_cut = s->h_cut = nullptr;
    s->cut_nsub = s->cut_nt = s->cut_ndmrow = s->cut_max = 0;
}

static void refine_free(pb_search *s)
{
    if (s->d_rf_g) (void)hipFree(s->d_rf_g);
    if (s->d_rf_reqi) (void)hipFree(s->d_rf_reqi);
    if (s->d_rf_reqf) (void)hipFree(s->d_rf_reqf);
    if (s->d_rf_out) (void)hipFree(s->d_rf_out);
    if (s->h_rf) (void)hipHostFree(s->h_rf);
    for (int i = 0; i < 3; ++i) {
        if (s->ev_rf[i]) (void)hipEventDestroy(s->ev_rf[i]);
        s->ev_rf[i] = nullptr;
    }
    s->d_rf_g = s->d_rf_out = s->h_rf = nullptr;
    s->d_rf_reqi = nullptr;
    s->d_rf_reqf = nullptr;
    s->rf_nstep = s->rf_H = s->rf_wmax = s->rf_max = 0;
}

static void giants_free(pb_search *s)
{
    void *p[] = {s->d_gi_cnt, s->d_gi_row, s->d_gi, s->d_gi_lab, s->d_gi_best, s->d_gi_acc, s->d_gi_tile, s->d_gi_out};
    for (void *q : p)
        if (q) (void)hipFree(q);
    if (s->h_gi) (void)hipHostFree(s->h_gi);
    for (int i = 0; i < 4; ++i) {
        if (s->ev_gi[i]) (void)hipEventDestroy(s->ev_gi[i]);
        s->ev_gi[i] = nullptr;
    }
    s->d_gi_cnt = s->d_gi_row = s->d_gi = s->d_gi_lab = s->d_gi_acc = s->d_gi_tile = s->d_gi_out = s->h_gi = nullptr;
    s->d_gi_best = nullptr;
    s->gi_sep_time = s->gi_sep_dm = s->gi_sep_filter = s->gi_max = s->gi_last = s->gi_sweeps = 0;
}

extern "C" void pb_search_destroy(pb_search *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    void *p[] = {s->d_codes, s->d_xt, s->d_delay, s->d_D, s->d_stats, s->d_snr, s->d_wid, s->d_P, s->d_peaks, s->d_chans,
                 s->d_zdelay, s->d_med, s->d_z, s->d_zP, s->d_zstats, s->d_zsnr, s->d_zwid, s->d_tlist, s->d_rcnt};
    for (int i = 0; i < 7; ++i)
        if (s->ev[i]) (void)hipEventDestroy(s->ev[i]);
    if (s->ev_rfi) (void)hipEventDestroy(s->ev_rfi);
    cutouts_free(s);
    refine_free(s);
    giants_free(s);
    for (void *q : p)
        if (q) (void)hipFree(q);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

extern "C" int pb_search_info(const pb_search *s, int *ndm, int *nbox, int *max_delay)
{
    if (!s) return PB_EINVAL;
    if (ndm) *ndm = s->ndm;
    if (nbox) *nbox = s->nbox;
    if (max_delay) *max_delay = s->max_delay;
    return PB_OK;
}

extern "C" int pb_search_set_baseline(pb_search *s, int window_samples)
{
    if (!s || window_samples < 0) return PB_EINVAL;
    s->baseline = window_samples;
    return PB_OK;
}

extern "C" int pb_search_set_rfi(pb_search *s, int narrow, int broad, float tol, int rfi_boxcar_max)
{
    std::string &err = s ? s->err : g_search_err;
    if (!(tol > 0) || !std::isfinite(tol)) {
        err = "pb_search_set_rfi: tol must be > 0 and finite";
        return PB_EINVAL;
    }
    if (rfi_boxcar_max < 1 || rfi_boxcar_max > 64 || (rfi_boxcar_max & (rfi_boxcar_max - 1))) {
        err = "pb_search_set_rfi: rfi_boxcar_max must be a power of two in 1..64";
        return PB_EINVAL;
    }
    if (!s) {
        g_search_err = "pb_search_set_rfi: no search handle";
        return PB_EINVAL;
    }
    if ((narrow || broad) && !s->d_rcnt) {
        // the buffers of the cleaning, once: the zero-DM series has its own (the others are sized per trial DM)
        const size_t tp = s->tpitch;
        SCHK(s, hipSetDevice(s->device));
        SCHK(s, hipMalloc((void **)&s->d_zdelay, (size_t)s->nact * sizeof(int32_t)));
        SCHK(s, hipMemset(s->d_zdelay, 0, (size_t)s->nact * sizeof(int32_t)));
        SCHK(s, hipMalloc((void **)&s->d_med, (size_t)s->nact));
        SCHK(s, hipMalloc((void **)&s->d_z, tp * sizeof(uint32_t)));
        SCHK(s, hipMalloc((void **)&s->d_zP, (tp + 8) * sizeof(uint64_t)));
        SCHK(s, hipMalloc((void **)&s->d_zstats, 2 * sizeof(float)));
        SCHK(s, hipMalloc((void **)&s->d_zsnr, tp * sizeof(float)));
        SCHK(s, hipMalloc((void **)&s->d_zwid, tp));
        SCHK(s, hipMalloc((void **)&s->d_tlist, tp * sizeof(int32_t)));
        SCHK(s, hipEventCreate(&s->ev_rfi));
        SCHK(s, hipMalloc((void **)&s->d_rcnt, 2 * sizeof(unsigned long long)));
    }
    s->rfi_narrow = narrow != 0;
    s->rfi_broad = broad != 0;
    s->rfi_tol = tol;
    s->rfi_nbox = 0;
    while ((1 << s->rfi_nbox) <= rfi_boxcar_max) s->rfi_nbox++;
    return PB_OK;
}

// RFI cleaning of the transposed block in place (both parts or one), between ev[2] and ev_rfi
static int search_clean(pb_search *s, int nsamp)
{
    const size_t ppitch = s->tpitch + 8;
    SCHK(s, hipMemsetAsync(s->d_rcnt, 0, 2 * sizeof(unsigned long long), s->stream));
    k_rfi_narrow<<<s->nact, 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->d_med, nsamp, s->tpitch, s->rfi_tol,
                                                 s->rfi_narrow, s->d_rcnt);
    if (s->rfi_broad) {
        dim3 gz((nsamp + DDM_TILE - 1) / DDM_TILE, 1);
        k_dedisperse<<<gz, 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->d_zdelay, s->d_z, s->nact, 1, nsamp, s->tpitch,
                                                s->tpitch);
        k_prefix<<<1, 256, 0, s->stream>>>(s->d_z, s->d_zP, nsamp, s->tpitch, ppitch);
        k_series_stats<<<1, 256, 0, s->stream>>>(s->d_z, s->d_zP, s->d_zstats, nsamp, s->baseline, s->tpitch, ppitch);
        dim3 gb((nsamp + 255) / 256, 1);
        k_boxcar<<<gb, 256, 0, s->stream>>>(s->d_zP, s->d_zstats, s->d_zsnr, s->d_zwid, nsamp, s->rfi_nbox, s->baseline,
                                            s->tpitch, ppitch, 0.f, nullptr, 0);
        k_rfi_broad_list<<<gb, 256, 0, s->stream>>>(s->d_zsnr, s->d_zwid, nsamp, s->rfi_tol, 1 << (s->rfi_nbox - 1),
                                                    s->d_tlist, s->d_rcnt + 1);
        k_rfi_broad_mask<<<(s->nact + 3) / 4, 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->d_med, s->d_tlist,
                                                                   s->d_rcnt + 1, s->nact, s->tpitch);
    }
    SCHK(s, hipEventRecord(s->ev_rfi, s->stream));
    return PB_OK;
}

static int search_run(pb_search *s, const void *codes, int codes_on_device, int nsamp, int nbit, float thresh,
                      bool want_peaks)
{
    if (!s || !codes) return PB_EINVAL;
    if (nsamp > s->max_samples || !(nbit == 8 || nbit == 4 || nbit == 2)) {
        s->err = "pb_search_run: block too long or bad nbit";
        return PB_EINVAL;
    }
    const int tout = nsamp - s->max_delay;
    if (tout < 64) {
        s->err = "pb_search_run: block shorter than the largest dispersion delay";
        return PB_EINVAL;
    }
    SCHK(s, hipSetDevice(s->device));
    const size_t nbytes = (size_t)nsamp * s->nchan * nbit / 8;
    const uint8_t *d_codes = (const uint8_t *)codes;
    SCHK(s, hipEventRecord(s->ev[0], s->stream));
    if (!codes_on_device) {
        SCHK(s, hipMemcpyAsync(s->d_codes, codes, nbytes, hipMemcpyHostToDevice, s->stream));
        d_codes = s->d_codes;
    }
    SCHK(s, hipEventRecord(s->ev[1], s->stream));
    dim3 gt((nsamp + 63) / 64, (s->nchan + 63) / 64);
    k_transpose_codes<<<gt, 256, 0, s->stream>>>(d_codes, s->d_xt, nsamp, s->nchan, nbit, s->tpitch);
    SCHK(s, hipEventRecord(s->ev[2], s->stream));
    s->rfi_ran = s->rfi_narrow || s->rfi_broad;
    if (s->rfi_ran) {
        const int rc = search_clean(s, nsamp);
        if (rc) return rc;
    }
    dim3 gd((tout + 255) / 256, s->ndm);
    dim3 gdd((tout + DDM_TILE - 1) / DDM_TILE, (s->ndm + DDM_DB - 1) / DDM_DB);
    k_dedisperse<<<gdd, 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->d_delay, s->d_D, s->nact, s->ndm, tout, s->tpitch, s->tpitch);
    SCHK(s, hipEventRecord(s->ev[3], s->stream));
    const size_t ppitch = s->tpitch + 8;
    k_prefix<<<s->ndm, 256, 0, s->stream>>>(s->d_D, s->d_P, tout, s->tpitch, ppitch);
    k_series_stats<<<s->ndm, 256, 0, s->stream>>>(s->d_D, s->d_P, s->d_stats, tout, s->baseline, s->tpitch, ppitch);
    SCHK(s, hipEventRecord(s->ev[4], s->stream));
    if (want_peaks) SCHK(s, hipMemsetAsync(s->d_peaks, 0, sizeof(int32_t), s->stream));
    k_boxcar<<<gd, 256, 0, s->stream>>>(s->d_P, s->d_stats, s->d_snr, s->d_wid, tout, s->nbox, s->baseline, s->tpitch,
                                        ppitch, thresh, want_peaks ? s->d_peaks : nullptr, s->max_peaks);
    SCHK(s, hipEventRecord(s->ev[5], s->stream));
    SCHK(s, hipGetLastError());
    s->last_tout = tout;
    s->last_nsamp = nsamp;
    s->gi_tout = tout;
    return PB_OK;
}

// after the run's last event: stage times, and the cleaning's time and counts (the dedispersion stage starts where
// the cleaning ends)
static int search_times(pb_search *s)
{
    for (int i = 0; i < 6; ++i) {
        float ms = 0.f;
        const hipEvent_t a = (i == 2 && s->rfi_ran) ? s->ev_rfi : s->ev[i];
        if (hipEventElapsedTime(&ms, a, s->ev[i + 1]) == hipSuccess) s->ms[i] = ms;
    }
    s->n_narrow = 0;
    s->n_broad = 0;
    s->rfi_ms = 0.f;
    if (s->rfi_ran) {
        unsigned long long c[2];
        SCHK(s, hipMemcpy(c, s->d_rcnt, sizeof c, hipMemcpyDeviceToHost));
        s->n_narrow = c[0];
        s->n_broad = (int)c[1];
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s->ev[2], s->ev_rfi) == hipSuccess) s->rfi_ms = ms;
    }
    return PB_OK;
}

// codes: nsamp x nchan samples of nbit bits in SIGPROC order (host, or device if codes_on_device).
// Outputs (host, any may be NULL): snr [ndm][tout] float, width_log2 [ndm][tout] u8,
// series [ndm][tout] u32 (the dedispersed sums), stats [ndm][2]; tout = nsamp - max_delay.
extern "C" int pb_search_run(pb_search *s, const void *codes, int codes_on_device, int nsamp, int nbit, float *snr,
                             uint8_t *width_log2, uint32_t *series, float *stats, int *tout_out)
{
    int rc = search_run(s, codes, codes_on_device, nsamp, nbit, 0.f, false);
    if (rc) return rc;
    const int tout = s->last_tout;
    SCHK(s, hipStreamSynchronize(s->stream));
    if (snr) SCHK(s, hipMemcpy2D(snr, tout * sizeof(float), s->d_snr, s->tpitch * sizeof(float), tout * sizeof(float), s->ndm, hipMemcpyDeviceToHost));
    if (width_log2) SCHK(s, hipMemcpy2D(width_log2, tout, s->d_wid, s->tpitch, tout, s->ndm, hipMemcpyDeviceToHost));
    if (series) SCHK(s, hipMemcpy2D(series, tout * sizeof(uint32_t), s->d_D, s->tpitch * sizeof(uint32_t), tout * sizeof(uint32_t), s->ndm, hipMemcpyDeviceToHost));
    if (stats) SCHK(s, hipMemcpy(stats, s->d_stats, (size_t)s->ndm * 2 * sizeof(float), hipMemcpyDeviceToHost));
    SCHK(s, hipEventRecord(s->ev[6], s->stream));
    SCHK(s, hipEventSynchronize(s->ev[6]));
    rc = search_times(s);
    if (rc) return rc;
    if (tout_out) *tout_out = tout;
    return PB_OK;
}

// The search as the production chain uses it: only the (DM, sample) points at or above `threshold` come back
// (what heimdall's giant finder starts from), not the S/N planes: peaks[4 i ..] = DM index, sample, S/N
// (float bits), log2 width; *npeaks may exceed max_out when the list was truncated.  The list is in arrival order
// and holds max_peaks points; the giant finder and the labelling themselves are pb_search_giants, on the planes.
extern "C" int pb_search_peaks(pb_search *s, const void *codes, int codes_on_device, int nsamp, int nbit,
                               float threshold, int32_t *peaks, int max_out, int *npeaks, int *tout_out)
{
    if (!peaks || !npeaks || max_out < 1) return PB_EINVAL;
    int rc = search_run(s, codes, codes_on_device, nsamp, nbit, threshold, true);
    if (rc) return rc;
    int32_t n = 0;
    SCHK(s, hipMemcpyAsync(&n, s->d_peaks, sizeof n, hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipStreamSynchronize(s->stream));
    const int ncopy = std::min(std::min((int)n, max_out), s->max_peaks);      // never past the device list
    if (ncopy > 0) SCHK(s, hipMemcpy(peaks, s->d_peaks + 1, (size_t)ncopy * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    SCHK(s, hipEventRecord(s->ev[6], s->stream));
    SCHK(s, hipEventSynchronize(s->ev[6]));
    rc = search_times(s);
    if (rc) return rc;
    *npeaks = n;
    if (tout_out) *tout_out = s->last_tout;
    return PB_OK;
}

extern "C" int pb_search_timers(const pb_search *s, float *ms6)
{
    if (!s || !ms6) return PB_EINVAL;
    for (int i = 0; i < 6; ++i) ms6[i] = s->ms[i];
    return PB_OK;
}

extern "C" int pb_search_rfi_info(const pb_search *s, uint64_t *n_narrow, int *n_broad_samples, float *ms)
{
    if (!s) return PB_EINVAL;
    if (n_narrow) *n_narrow = s->n_narrow;
    if (n_broad_samples) *n_broad_samples = s->n_broad;
    if (ms) *ms = s->rfi_ms;
    return PB_OK;
}

extern "C" int pb_search_fetch_clean(pb_search *s, uint8_t *xt, size_t nbytes)
{
    if (!s || !xt) return PB_EINVAL;
    const size_t n = s->last_nsamp;
    if (n == 0 || nbytes < n * s->nchan) {
        s->err = "pb_search_fetch_clean: no block searched yet, or the buffer is smaller than nchan x nsamp";
        return PB_EINVAL;
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    SCHK(s, hipMemcpy2D(xt, n, s->d_xt, s->tpitch, n, s->nchan, hipMemcpyDeviceToHost));
    return PB_OK;
}

#define CUT_MAX_NT 8192          // the bins of a frequency-time cutout live in LDS (4 bytes each)

extern "C" int pb_search_set_cutouts(pb_search *s, int nsub, int nt, int ndmrow, int max_cands)
{
    if (!s) {
        g_search_err = "pb_search_set_cutouts: no search handle";
        return PB_EINVAL;
    }
    if (max_cands < 0) {
        s->err = "pb_search_set_cutouts: max_cands must be >= 0";
        return PB_EINVAL;
    }
    if (max_cands > 0) {
        if (nsub < 1 || s->nchan % nsub) {
            s->err = "pb_search_set_cutouts: nsub must divide the number of channels";
            return PB_EINVAL;
        }
        if (nt < 2 || (nt & 1) || ndmrow < 2 || (ndmrow & 1)) {
            s->err = "pb_search_set_cutouts: nt and ndmrow must be positive and even";
            return PB_EINVAL;
        }
        if ((long long)nt * 64 > (long long)s->max_samples || nt > CUT_MAX_NT) {
            s->err = "pb_search_set_cutouts: nt * 64 must not exceed max_samples (and nt 8192)";
            return PB_EINVAL;
        }
        if ((long long)max_cands * ((long long)nsub + ndmrow) * nt > (1ll << 28)) {
            s->err = "pb_search_set_cutouts: max_cands cutouts of this geometry exceed 2 GiB";
            return PB_EINVAL;
        }
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    cutouts_free(s);
    if (max_cands == 0) return PB_OK;
    // zapped channels are left out of chans[], so a subband's channels are one run of it
    std::vector<int32_t> chans(s->nact), run(2 * (size_t)nsub);
    SCHK(s, hipMemcpy(chans.data(), s->d_chans, chans.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int per = s->nchan / nsub;
    int k = 0;
    for (int b = 0; b < nsub; ++b) {
        run[2 * b] = k;
        while (k < s->nact && chans[k] < (b + 1) * per) ++k;
        run[2 * b + 1] = k;
    }
    const size_t nout = 2 * (size_t)max_cands * ((size_t)nsub + ndmrow) * nt;
    hipError_t e = hipMalloc((void **)&s->d_cut_req, (size_t)max_cands * 3 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_cut_sub, run.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(s->d_cut_sub, run.data(), run.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_cut, nout * sizeof(uint32_t));
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_cut, (nout + (size_t)max_cands * 3) * sizeof(uint32_t), hipHostMallocDefault);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&s->ev_cut[i]);
    if (e != hipSuccess) {
        cutouts_free(s);
        s->err = std::string("pb_search_set_cutouts: ") + hipGetErrorString(e);
        return PB_EHIP;
    }
    s->cut_nsub = nsub;
    s->cut_nt = nt;
    s->cut_ndmrow = ndmrow;
    s->cut_max = max_cands;
    return PB_OK;
}

extern "C" int pb_search_cutouts(pb_search *s, const int32_t *cands3, int n, uint32_t *ft, uint32_t *ft_hits, uint32_t *dt,
                                 uint32_t *dt_hits)
{
    if (!s) {
        g_search_err = "pb_search_cutouts: no search handle";
        return PB_EINVAL;
    }
    if (s->cut_max == 0) {
        s->err = "pb_search_cutouts: cutouts are not switched on (pb_search_set_cutouts)";
        return PB_EINVAL;
    }
    if (s->last_nsamp == 0) {
        s->err = "pb_search_cutouts: no block searched yet";
        return PB_EINVAL;
    }
    if (!cands3 || n < 0 || n > s->cut_max) {
        s->err = "pb_search_cutouts: no request list, or more requests than max_cands";
        return PB_EINVAL;
    }
    for (int i = 0; i < n; ++i) {
        const int dmi = cands3[3 * i], t = cands3[3 * i + 1], ts = cands3[3 * i + 2];
        if (dmi < 0 || dmi >= s->ndm || t < 0 || t >= s->last_tout || ts < 1 || ts > 64 || (ts & (ts - 1))) {
            s->err = "pb_search_cutouts: request " + std::to_string(i) + " out of range (DM index in [0, ndm), peak sample in "
                     "[0, tout) of the last run, tscr a power of two in 1..64)";
            return PB_EINVAL;
        }
    }
    if (n == 0) return PB_OK;
    const int nsub = s->cut_nsub, nt = s->cut_nt, nrow = s->cut_ndmrow;
    const size_t nf = (size_t)n * nsub * nt, nd = (size_t)n * nrow * nt, nout = 2 * (nf + nd);
    uint32_t *d_ft = s->d_cut, *d_fth = d_ft + nf, *d_dt = d_fth + nf, *d_dth = d_dt + nd;
    int32_t *h_req = (int32_t *)(s->h_cut + 2 * (size_t)s->cut_max * ((size_t)nsub + nrow) * nt);
    SCHK(s, hipSetDevice(s->device));
    for (int i = 0; i < 3 * n; ++i) h_req[i] = cands3[i];
    SCHK(s, hipMemcpyAsync(s->d_cut_req, h_req, (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    SCHK(s, hipEventRecord(s->ev_cut[0], s->stream));
    k_cutout_ft<<<dim3(nsub, n), 256, (size_t)nt * sizeof(uint32_t), s->stream>>>(
        s->d_xt, s->d_chans, s->d_delay, s->d_cut_req, s->d_cut_sub, d_ft, d_fth, s->nact, s->last_nsamp, nt, s->tpitch);
    k_cutout_dt<<<dim3(nrow, n), 256, 0, s->stream>>>(s->d_D, s->d_cut_req, d_dt, d_dth, s->ndm, s->last_tout, nt, s->tpitch);
    SCHK(s, hipEventRecord(s->ev_cut[1], s->stream));
    SCHK(s, hipMemcpyAsync(s->h_cut, s->d_cut, nout * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipEventRecord(s->ev_cut[2], s->stream));
    SCHK(s, hipGetLastError());
    SCHK(s, hipEventSynchronize(s->ev_cut[2]));
    for (int i = 0; i < 2; ++i)
        if (hipEventElapsedTime(&s->cut_ms[i], s->ev_cut[0], s->ev_cut[i + 1]) != hipSuccess) s->cut_ms[i] = 0.f;
    if (ft) memcpy(ft, s->h_cut, nf * sizeof(uint32_t));
    if (ft_hits) memcpy(ft_hits, s->h_cut + nf, nf * sizeof(uint32_t));
    if (dt) memcpy(dt, s->h_cut + 2 * nf, nd * sizeof(uint32_t));
    if (dt_hits) memcpy(dt_hits, s->h_cut + 2 * nf + nd, nd * sizeof(uint32_t));
    return PB_OK;
}

extern "C" int pb_search_cutout_timers(const pb_search *s, float *ms2)
{
    if (!s || !ms2) return PB_EINVAL;
    ms2[0] = s->cut_ms[0];
    ms2[1] = s->cut_ms[1];
    return PB_OK;
}

extern "C" int pb_search_set_refine(pb_search *s, int nstep, int half_window, int wmax, int max_cands)
{
    if (!s) {
        g_search_err = "pb_search_set_refine: no search handle";
        return PB_EINVAL;
    }
    if (max_cands < 0) {
        s->err = "pb_search_set_refine: max_cands must be >= 0";
        return PB_EINVAL;
    }
    if (max_cands > 0) {
        if (nstep < 1 || nstep > 4096) {
            s->err = "pb_search_set_refine: nstep must be in 1..4096";
            return PB_EINVAL;
        }
        if (wmax < 2 || wmax > 64 || (wmax & 1)) {
            s->err = "pb_search_set_refine: wmax must be even and in 2..64";
            return PB_EINVAL;
        }
        if (half_window < 2 * wmax || 2 * (half_window + wmax / 2) > RF_MAXL) {
            s->err = "pb_search_set_refine: half_window must be at least 2 wmax (a full window holds 4 wmax samples) and "
                     "half_window + wmax / 2 at most 1024";
            return PB_EINVAL;
        }
        if ((long long)s->nact * 255 * wmax >= (1ll << 32)) {
            s->err = "pb_search_set_refine: too many channels for 32-bit running sums";
            return PB_EINVAL;
        }
        if ((long long)max_cands * nstep * 2 * (half_window + wmax / 2) > (1ll << 28)) {
            s->err = "pb_search_set_refine: max_cands requests of this geometry exceed 1 GiB";
            return PB_EINVAL;
        }
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    refine_free(s);
    if (max_cands == 0) return PB_OK;
    std::vector<int32_t> chans(s->nact);
    SCHK(s, hipMemcpy(chans.data(), s->d_chans, chans.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<double> g(s->nact);
    for (int k = 0; k < s->nact; ++k)
        g[k] = delay_chan_term((double)s->fch1 + (double)chans[k] * (double)s->foff, s->ftop);
    const size_t L = 2 * ((size_t)half_window + wmax / 2), nw = wmax / 2;
    const size_t nd = (size_t)max_cands * (nstep + nw), ni = (size_t)max_cands * (1 + nw), ns = (size_t)max_cands * nstep * L;
    hipError_t e = hipMalloc((void **)&s->d_rf_g, g.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(s->d_rf_g, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_rf_reqi, (size_t)max_cands * 4 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_rf_reqf, (size_t)max_cands * 2 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_rf_out, nd * sizeof(double) + (ni + ns) * sizeof(int32_t));
    if (e == hipSuccess)
        e = hipHostMalloc((void **)&s->h_rf, nd * sizeof(double) + (ni + ns + (size_t)max_cands * 6) * sizeof(int32_t),
                          hipHostMallocDefault);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&s->ev_rf[i]);
    if (e != hipSuccess) {
        refine_free(s);
        s->err = std::string("pb_search_set_refine: ") + hipGetErrorString(e);
        return PB_EHIP;
    }
    s->rf_nstep = nstep;
    s->rf_H = half_window;
    s->rf_wmax = wmax;
    s->rf_max = max_cands;
    return PB_OK;
}

extern "C" int pb_search_refine(pb_search *s, const int32_t *req_i2, const float *req_f2, int n, int32_t *status,
                                double *sn_dm, int32_t *kbest, double *opt_sn, int32_t *opt_loc, uint32_t *series)
{
    if (!s) {
        g_search_err = "pb_search_refine: no search handle";
        return PB_EINVAL;
    }
    if (s->rf_max == 0) {
        s->err = "pb_search_refine: refinement is not switched on (pb_search_set_refine)";
        return PB_EINVAL;
    }
    if (s->last_nsamp == 0) {
        s->err = "pb_search_refine: no block searched yet";
        return PB_EINVAL;
    }
    if (!req_i2 || !req_f2 || n < 0 || n > s->rf_max) {
        s->err = "pb_search_refine: no request list, or more requests than max_cands";
        return PB_EINVAL;
    }
    const int T = s->last_tout, H = s->rf_H, M = s->rf_wmax / 2, nstep = s->rf_nstep, nw = M;
    for (int i = 0; i < n; ++i) {
        const int t = req_i2[2 * i], w = req_i2[2 * i + 1];
        if (t < 0 || t >= T || w < 1 || w > s->rf_wmax || !std::isfinite(req_f2[2 * i]) || !std::isfinite(req_f2[2 * i + 1])) {
            s->err = "pb_search_refine: request " + std::to_string(i) + " out of range (peak sample in [0, tout) of the last "
                     "run, width in 1..wmax, dm_lo and dm_step finite)";
            return PB_EINVAL;
        }
    }
    if (n == 0) return PB_OK;
    const size_t L = 2 * ((size_t)H + M);
    const size_t nd = (size_t)n * (nstep + nw), ni = (size_t)n * (1 + nw), ns = (size_t)n * nstep * L;
    // one buffer, so one copy: the doubles, the integers, then the series (copied only when it is asked for)
    double *d_sn = s->d_rf_out, *d_osn = d_sn + (size_t)n * nstep;
    int32_t *d_kb = (int32_t *)(s->d_rf_out + nd), *d_loc = d_kb + n;
    uint32_t *d_ser = (uint32_t *)(d_kb + ni);
    const size_t maxw = (size_t)s->rf_max * (nstep + nw) * 2 + (size_t)s->rf_max * (1 + nw) + (size_t)s->rf_max * nstep * L;
    int32_t *h_reqi = (int32_t *)s->h_rf + maxw;
    float *h_reqf = (float *)(h_reqi + 4 * (size_t)s->rf_max);
    std::vector<int32_t> st(n);
    for (int i = 0; i < n; ++i) {
        const int t = req_i2[2 * i], w = req_i2[2 * i + 1];
        st[i] = std::min(T, t + H) - std::max(0, t - H) < 4 * s->rf_wmax ? 1 : 0;
        h_reqi[4 * i] = t;
        h_reqi[4 * i + 1] = w | 1;                                      // an even width becomes width + 1
        h_reqi[4 * i + 2] = st[i];
        h_reqi[4 * i + 3] = 0;
        h_reqf[2 * i] = req_f2[2 * i];
        h_reqf[2 * i + 1] = req_f2[2 * i + 1];
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipMemcpyAsync(s->d_rf_reqi, h_reqi, (size_t)n * 4 * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    SCHK(s, hipMemcpyAsync(s->d_rf_reqf, h_reqf, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, s->stream));
    SCHK(s, hipEventRecord(s->ev_rf[0], s->stream));
    k_refine_series<<<dim3(nstep, n), 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->d_rf_g, s->d_rf_reqi, s->d_rf_reqf, d_ser,
                                                           s->nact, T, (int)L, H + M, (double)s->tsamp, s->dm_last, s->tpitch);
    k_refine_dm<<<dim3(nstep, n), 256, 0, s->stream>>>(d_ser, s->d_rf_reqi, s->d_rf_reqf, d_sn, T, H, M, s->dm_last);
    k_refine_width<<<n, 256, 0, s->stream>>>(d_ser, s->d_rf_reqi, d_sn, d_kb, d_osn, d_loc, T, H, M, nstep, nw);
    SCHK(s, hipEventRecord(s->ev_rf[1], s->stream));
    const size_t nbytes = nd * sizeof(double) + (ni + (series ? ns : 0)) * sizeof(int32_t);
    SCHK(s, hipMemcpyAsync(s->h_rf, s->d_rf_out, nbytes, hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipEventRecord(s->ev_rf[2], s->stream));
    SCHK(s, hipGetLastError());
    SCHK(s, hipEventSynchronize(s->ev_rf[2]));
    for (int i = 0; i < 2; ++i)
        if (hipEventElapsedTime(&s->rf_ms[i], s->ev_rf[0], s->ev_rf[i + 1]) != hipSuccess) s->rf_ms[i] = 0.f;
    const double *h_sn = s->h_rf, *h_osn = h_sn + (size_t)n * nstep;
    const int32_t *h_kb = (const int32_t *)(s->h_rf + nd), *h_loc = h_kb + n;
    if (status) memcpy(status, st.data(), (size_t)n * sizeof(int32_t));
    if (sn_dm) memcpy(sn_dm, h_sn, (size_t)n * nstep * sizeof(double));
    if (kbest) memcpy(kbest, h_kb, (size_t)n * sizeof(int32_t));
    if (opt_sn) memcpy(opt_sn, h_osn, (size_t)n * nw * sizeof(double));
    if (opt_loc) memcpy(opt_loc, h_loc, (size_t)n * nw * sizeof(int32_t));
    if (series) memcpy(series, h_kb + ni, ns * sizeof(uint32_t));
    return PB_OK;
}

extern "C" int pb_search_refine_timers(const pb_search *s, float *ms2)
{
    if (!s || !ms2) return PB_EINVAL;
    ms2[0] = s->rf_ms[0];
    ms2[1] = s->rf_ms[1];
    return PB_OK;
}

// ---- giants and their clusters: host side (the kernels stand before the refinement's) ----

#define GI_MAX_GIANTS (1 << 22)

extern "C" int pb_search_set_giants(pb_search *s, int sep_time, int sep_dm, int sep_filter, int max_giants)
{
    if (!s) {
        g_search_err = "pb_search_set_giants: no search handle";
        return PB_EINVAL;
    }
    if (max_giants < 0 || max_giants > GI_MAX_GIANTS) {
        s->err = "pb_search_set_giants: max_giants must be in 0..4194304";
        return PB_EINVAL;
    }
    if (max_giants > 0) {
        if (sep_time < 1 || sep_time > 64) {
            s->err = "pb_search_set_giants: sep_time must be in 1..64 (a chunk of 64 samples looks one chunk back)";
            return PB_EINVAL;
        }
        if (sep_dm < 0 || sep_filter < 0) {
            s->err = "pb_search_set_giants: sep_dm and sep_filter must be >= 0";
            return PB_EINVAL;
        }
        if ((long long)s->ndm * (long long)s->max_samples >= (1ll << 31)) {
            s->err = "pb_search_set_giants: ndm x max_samples must stay below 2^31 (32-bit counts)";
            return PB_EINVAL;
        }
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    giants_free(s);
    if (max_giants == 0) return PB_OK;
    const size_t cap = (size_t)max_giants, ntile = (cap + 255) / 256;
    hipError_t e = hipMalloc((void **)&s->d_gi_cnt, (size_t)s->ndm * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_gi_row, ((size_t)s->ndm + 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_gi, cap * GI_W * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_gi_lab, cap * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_gi_best, cap * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_gi_acc, cap * 4 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_gi_tile, (2 * ntile + 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_gi_out, (16 + cap * GI_W) * sizeof(int32_t));
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_gi, (16 + cap * GI_W) * sizeof(int32_t), hipHostMallocDefault);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&s->ev_gi[i]);
    if (e != hipSuccess) {
        giants_free(s);
        s->err = std::string("pb_search_set_giants: ") + hipGetErrorString(e);
        return PB_EHIP;
    }
    s->gi_sep_time = sep_time;
    s->gi_sep_dm = sep_dm;
    s->gi_sep_filter = sep_filter;
    s->gi_max = max_giants;
    return PB_OK;
}

extern "C" int pb_search_set_planes(pb_search *s, const float *snr, const uint8_t *width_log2, int tout)
{
    if (!s) {
        g_search_err = "pb_search_set_planes: no search handle";
        return PB_EINVAL;
    }
    if (!snr || !width_log2 || tout < 1 || tout > s->max_samples) {
        s->err = "pb_search_set_planes: no planes, or tout outside 1..max_samples";
        return PB_EINVAL;
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    SCHK(s, hipMemcpy2D(s->d_snr, s->tpitch * sizeof(float), snr, (size_t)tout * sizeof(float), (size_t)tout * sizeof(float),
                        s->ndm, hipMemcpyHostToDevice));
    SCHK(s, hipMemcpy2D(s->d_wid, s->tpitch, width_log2, (size_t)tout, (size_t)tout, s->ndm, hipMemcpyHostToDevice));
    s->gi_tout = tout;
    return PB_OK;
}

extern "C" int pb_search_giants(pb_search *s, float thresh, int t_lo, int t_hi, int32_t *cands, int max_out, int *ncands,
                                int *ngiants, int *overflow)
{
    if (!s) {
        g_search_err = "pb_search_giants: no search handle";
        return PB_EINVAL;
    }
    if (s->gi_max == 0) {
        s->err = "pb_search_giants: the stage is not switched on (pb_search_set_giants)";
        return PB_EINVAL;
    }
    if (s->gi_tout == 0) {
        s->err = "pb_search_giants: no block searched and no planes set yet";
        return PB_EINVAL;
    }
    if (t_lo < 0 || t_lo >= t_hi || t_hi > s->gi_tout) {
        s->err = "pb_search_giants: the sample range must satisfy 0 <= t_lo < t_hi <= tout of the planes";
        return PB_EINVAL;
    }
    if (thresh != thresh || max_out < 0 || (max_out > 0 && !cands) || !ncands || !ngiants || !overflow) {
        s->err = "pb_search_giants: NaN threshold, or an output is missing";
        return PB_EINVAL;
    }
    const int cap = s->gi_max, ndm = s->ndm, sep = s->gi_sep_time;
    int32_t *ctl = s->d_gi_out, *d_cands = s->d_gi_out + 16;
    s->gi_last = 0;
    s->gi_sweeps = 0;
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipMemsetAsync(s->d_gi_cnt, 0, (size_t)ndm * sizeof(int32_t), s->stream));
    SCHK(s, hipMemsetAsync(ctl, 0, 16 * sizeof(int32_t), s->stream));
    SCHK(s, hipEventRecord(s->ev_gi[0], s->stream));
    const int nchunk = ((t_hi + 63) >> 6) - (t_lo >> 6);
    k_giant_count<<<dim3((nchunk + 4 * GI_SEG - 1) / (4 * GI_SEG), ndm), 256, 0, s->stream>>>(s->d_snr, s->d_gi_cnt, t_lo, t_hi,
                                                                                               thresh, sep, s->tpitch);
    k_giant_scan<<<1, 256, 0, s->stream>>>(s->d_gi_cnt, s->d_gi_row, ndm, ctl, ctl + 1, cap);
    // G decides every grid that follows: the one word the host waits for before the end
    SCHK(s, hipMemcpyAsync(s->h_gi, ctl, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipStreamSynchronize(s->stream));
    const int G = s->h_gi[0], over = s->h_gi[1];
    const bool work = !over && G > 0;
    if (work)
        k_giant_write<<<(ndm + 3) / 4, 256, 0, s->stream>>>(s->d_snr, s->d_wid, s->d_gi_row, ctl, s->d_gi, s->d_gi_lab, ndm, t_lo,
                                                            t_hi, thresh, sep, cap, s->tpitch);
    SCHK(s, hipEventRecord(s->ev_gi[1], s->stream));
    if (work) {
        // every sweep that changes a label takes a root away, so G + 1 sweeps are the most there can be
        for (int sweep = 0;; ++sweep) {
            if (sweep > G + 1) {
                s->err = "pb_search_giants: the labelling did not settle";
                return PB_ESTATE;
            }
            SCHK(s, hipMemsetAsync(ctl + 3, 0, sizeof(int32_t), s->stream));
            k_giant_hook<<<(G + 3) / 4, 256, 0, s->stream>>>(s->d_gi, s->d_gi_row, s->d_gi_lab, ctl, G, sep, s->gi_sep_dm,
                                                             s->gi_sep_filter);
            k_giant_jump<<<(G + 255) / 256, 256, 0, s->stream>>>(s->d_gi_lab, G);
            SCHK(s, hipMemcpyAsync(s->h_gi + 3, ctl + 3, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
            SCHK(s, hipStreamSynchronize(s->stream));
            s->gi_sweeps = sweep + 1;
            if (!s->h_gi[3]) break;
        }
        const int ntile = (G + 255) / 256;
        int32_t *tile_cnt = s->d_gi_tile, *tile_off = s->d_gi_tile + (cap + 255) / 256;
        SCHK(s, hipMemsetAsync(s->d_gi_best, 0, (size_t)G * sizeof(unsigned long long), s->stream));
        SCHK(s, hipMemsetAsync(s->d_gi_acc, 0, (size_t)G * 4 * sizeof(int32_t), s->stream));
        k_giant_reduce<<<ntile, 256, 0, s->stream>>>(s->d_gi, s->d_gi_lab, s->d_gi_best, s->d_gi_acc, tile_cnt, G);
        k_giant_scan<<<1, 256, 0, s->stream>>>(tile_cnt, tile_off, ntile, ctl + 2, nullptr, 0);
        k_giant_cands<<<ntile, 256, 0, s->stream>>>(s->d_gi, s->d_gi_lab, s->d_gi_best, s->d_gi_acc, tile_off, d_cands, G, cap);
    }
    SCHK(s, hipEventRecord(s->ev_gi[2], s->stream));
    // one copy: the control words and the candidate table (a cluster holds a giant or more, so G rows are enough)
    const int nrow = work ? std::min(G, max_out) : 0;
    SCHK(s, hipMemcpyAsync(s->h_gi, s->d_gi_out, (16 + (size_t)nrow * GI_W) * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipEventRecord(s->ev_gi[3], s->stream));
    SCHK(s, hipGetLastError());
    SCHK(s, hipEventSynchronize(s->ev_gi[3]));
    float ms[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < 3; ++i)
        if (hipEventElapsedTime(&ms[i], s->ev_gi[i == 2 ? 0 : i], s->ev_gi[i == 2 ? 3 : i + 1]) != hipSuccess) ms[i] = 0.f;
    for (int i = 0; i < 3; ++i) s->gi_ms[i] = ms[i];
    const int nc = work ? s->h_gi[2] : 0;
    if (nc > 0 && max_out > 0) memcpy(cands, s->h_gi + 16, (size_t)std::min(nc, max_out) * GI_W * sizeof(int32_t));
    s->gi_last = work ? G : 0;
    *ncands = nc;
    *ngiants = G;
    *overflow = over;
    return PB_OK;
}

extern "C" int pb_search_giant_list(pb_search *s, int32_t *out, int max_out, int *n)
{
    if (!s) {
        g_search_err = "pb_search_giant_list: no search handle";
        return PB_EINVAL;
    }
    if (s->gi_max == 0 || !n || max_out < 0 || (max_out > 0 && !out)) {
        s->err = "pb_search_giant_list: the stage is not switched on, or an output is missing";
        return PB_EINVAL;
    }
    const int k = std::min(s->gi_last, max_out);
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    if (k > 0) SCHK(s, hipMemcpy(out, s->d_gi, (size_t)k * GI_W * sizeof(int32_t), hipMemcpyDeviceToHost));
    *n = s->gi_last;
    return PB_OK;
}

extern "C" int pb_search_giant_timers(const pb_search *s, float *ms3, int *nsweeps)
{
    if (!s || !ms3) return PB_EINVAL;
    for (int i = 0; i < 3; ++i) ms3[i] = s->gi_ms[i];
    if (nsweeps) *nsweeps = s->gi_sweeps;
    return PB_OK;
}
