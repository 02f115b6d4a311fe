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
// The optional stages that act on what a run leaves on the device have a file each, kernels and host side together:
// per-candidate cutouts (search_cutout.hip), a candidate's DM, width and S/N refined on a fine DM grid
// (search_refine.hip), giants and clusters of giants (search_giants.hip), a candidate's Stokes spectra and rotation measure
// (search_pol.hip, which also supplies the transposition of a four-product block), the sub-band search for band-limited
// bursts (search_subband.hip, which runs k_prefix .. k_boxcar on its band series through search_series_launch and
// search_boxcar_launch).  The streaming stage (search_stream.hip)
// stands before the cleaning instead: it fills the channel-major block piece by piece and enters at search_block.  This file is the core -- create .. destroy,
// run / peaks, the kernels of steps 1-3 -- and the cleaning, which launches k_dedisperse .. k_boxcar for its zero-DM
// series.  The handle and the host helpers: search_internal.h; the device helpers: search_dev.h.
#include "search_internal.h"
#include "search_dev.h"

std::string g_search_err;

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
// block hit the same cache lines.  This is the byte gather of search_dev.h, whose statement of what a lane may read
// and of the 16-bit sums holds here; it is written out in this kernel, the search's hot one, because the shared form
// did not compile to the same instructions.  Integer arithmetic: the sums are exact whatever the order.
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
    // tout, plus the delay) would leave what the gather may read.  No barrier in this kernel: a whole-lane exit is
    // safe.  A live lane's first byte is t + d <= tout - 1 + max_delay = nsamp - 1.
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
            const uint32_t a = gather_align(w[i], w[i + 1], sh);
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
        if (since >= GATHER_FLUSH) {
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
    const uint32_t inc = wave_inclusive_sum(loc);
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
    cnt = block_sum(cnt, sh_cnt);
    if (threadIdx.x == 0 && cnt) atomicAdd(nflag, (unsigned long long)cnt);
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

extern "C" const char *pb_search_last_error(const pb_search *s) { return s ? s->err.c_str() : g_search_err.c_str(); }

static int search_create(int device, int nchan, int max_samples, float fch1_mhz, float foff_mhz, float tsamp_s,
                         const std::vector<double> &dms, int boxcar_max, const int *zap_ranges, int nzap,
                         pb_search **out);

extern "C" int pb_search_create(int device, int nchan, int max_samples, float fch1_mhz, float foff_mhz, float tsamp_s,
                                float dm_min, float dm_max, float dm_step, int boxcar_max, const int *zap_ranges,
                                int nzap, pb_search **out)
{
    if (!out || !(dm_step > 0) || dm_max < dm_min) return search_fail(nullptr, "pb_search_create", "bad argument");
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
    if (!out || !dm_list || ndm < 1) return search_fail(nullptr, "pb_search_create_list", "bad argument");
    std::vector<double> dms(dm_list, dm_list + ndm);
    for (int i = 1; i < ndm; ++i)
        if (!(dms[i] > dms[i - 1])) return search_fail(nullptr, "pb_search_create_list", "the DM list must be strictly ascending");
    return search_create(device, nchan, max_samples, fch1_mhz, foff_mhz, tsamp_s, dms, boxcar_max, zap_ranges, nzap, out);
}

static int search_create(int device, int nchan, int max_samples, float fch1_mhz, float foff_mhz, float tsamp_s,
                         const std::vector<double> &dms, int boxcar_max, const int *zap_ranges, int nzap,
                         pb_search **out)
{
    const float dm_min = (float)dms.front();
    if (!out || nchan < 1 || max_samples < 64 || boxcar_max < 1) return search_fail(nullptr, "pb_search_create", "bad argument");
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
    s->ndm = (int)dms.size();
    while ((1 << s->nbox) <= boxcar_max) s->nbox++;
    s->dm_last = dms.back();
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
    // + 64: the pad that the byte gather may read into past the last row (search_dev.h)
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_xt, s->tpitch * nchan + 64);
    if (e == hipSuccess) e = hipMemset(s->d_xt, 0, s->tpitch * nchan + 64);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_delay, delay.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_chans, chans.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(s->d_chans, chans.data(), chans.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_D, (size_t)s->ndm * s->tpitch * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_stats, (size_t)s->ndm * 2 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_snr, (size_t)s->ndm * s->tpitch * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_wid, (size_t)s->ndm * s->tpitch);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_P, (size_t)s->ndm * s->ppitch() * sizeof(uint64_t));
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

void search_rfi_free(pb_search *s)
{
    search_release({s->rfi.d_zdelay, s->rfi.d_med, s->rfi.d_z, s->rfi.d_zP, s->rfi.d_zstats, s->rfi.d_zsnr, s->rfi.d_zwid,
                    s->rfi.d_tlist, s->rfi.d_rcnt}, nullptr, s->rfi.ev, 1);
    s->rfi = {};
}

extern "C" void pb_search_destroy(pb_search *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    search_rfi_free(s);
    search_rfichan_free(s);
    search_cutouts_free(s);
    search_refine_free(s);
    search_giants_free(s);
    search_gulp_free(s);
    search_pol_free(s);
    search_subbands_free(s);
    search_periodic_free(s);
    search_release({s->d_codes, s->d_xt, s->d_delay, s->d_D, s->d_stats, s->d_snr, s->d_wid, s->d_P, s->d_peaks, s->d_chans},
                   nullptr, s->ev, 7);
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
    const char *fn = "pb_search_set_rfi";
    if (!(tol > 0) || !std::isfinite(tol)) return search_fail(s, fn, "tol must be > 0 and finite");
    if (rfi_boxcar_max < 1 || rfi_boxcar_max > 64 || (rfi_boxcar_max & (rfi_boxcar_max - 1)))
        return search_fail(s, fn, "rfi_boxcar_max must be a power of two in 1..64");
    if (!s) return search_fail(s, fn, "no search handle");
    if ((narrow || broad) && !s->rfi.d_rcnt) {
        // the buffers of the cleaning, once: the zero-DM series has its own (the others are sized per trial DM)
        const size_t tp = s->tpitch;
        SCHK(s, hipSetDevice(s->device));
        SCHK(s, hipMalloc((void **)&s->rfi.d_zdelay, (size_t)s->nact * sizeof(int32_t)));
        SCHK(s, hipMemset(s->rfi.d_zdelay, 0, (size_t)s->nact * sizeof(int32_t)));
        SCHK(s, hipMalloc((void **)&s->rfi.d_med, (size_t)s->nact));
        SCHK(s, hipMalloc((void **)&s->rfi.d_z, tp * sizeof(uint32_t)));
        SCHK(s, hipMalloc((void **)&s->rfi.d_zP, s->ppitch() * sizeof(uint64_t)));
        SCHK(s, hipMalloc((void **)&s->rfi.d_zstats, 2 * sizeof(float)));
        SCHK(s, hipMalloc((void **)&s->rfi.d_zsnr, tp * sizeof(float)));
        SCHK(s, hipMalloc((void **)&s->rfi.d_zwid, tp));
        SCHK(s, hipMalloc((void **)&s->rfi.d_tlist, tp * sizeof(int32_t)));
        SCHK(s, hipEventCreate(&s->rfi.ev[0]));
        SCHK(s, hipMalloc((void **)&s->rfi.d_rcnt, 2 * sizeof(unsigned long long)));
    }
    s->rfi.narrow = narrow != 0;
    s->rfi.broad = broad != 0;
    s->rfi.tol = tol;
    s->rfi.nbox = 0;
    while ((1 << s->rfi.nbox) <= rfi_boxcar_max) s->rfi.nbox++;
    return PB_OK;
}

// RFI cleaning of the transposed block in place (both parts or one), between ev[2] and rfi.ev[0]
static int search_clean(pb_search *s, int nsamp)
{
    const size_t ppitch = s->ppitch();
    SCHK(s, hipMemsetAsync(s->rfi.d_rcnt, 0, 2 * sizeof(unsigned long long), s->stream));
    k_rfi_narrow<<<s->nact, 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->rfi.d_med, nsamp, s->tpitch, s->rfi.tol,
                                                 s->rfi.narrow, s->rfi.d_rcnt);
    if (s->rfi.broad) {
        dim3 gz((nsamp + DDM_TILE - 1) / DDM_TILE, 1);
        k_dedisperse<<<gz, 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->rfi.d_zdelay, s->rfi.d_z, s->nact, 1, nsamp, s->tpitch,
                                                s->tpitch);
        k_prefix<<<1, 256, 0, s->stream>>>(s->rfi.d_z, s->rfi.d_zP, nsamp, s->tpitch, ppitch);
        k_series_stats<<<1, 256, 0, s->stream>>>(s->rfi.d_z, s->rfi.d_zP, s->rfi.d_zstats, nsamp, s->baseline, s->tpitch, ppitch);
        dim3 gb((nsamp + 255) / 256, 1);
        k_boxcar<<<gb, 256, 0, s->stream>>>(s->rfi.d_zP, s->rfi.d_zstats, s->rfi.d_zsnr, s->rfi.d_zwid, nsamp, s->rfi.nbox, s->baseline,
                                            s->tpitch, ppitch, 0.f, nullptr, 0);
        k_rfi_broad_list<<<gb, 256, 0, s->stream>>>(s->rfi.d_zsnr, s->rfi.d_zwid, nsamp, s->rfi.tol, 1 << (s->rfi.nbox - 1),
                                                    s->rfi.d_tlist, s->rfi.d_rcnt + 1);
        k_rfi_broad_mask<<<(s->nact + 3) / 4, 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->rfi.d_med, s->rfi.d_tlist,
                                                                   s->rfi.d_rcnt + 1, s->nact, s->tpitch);
    }
    SCHK(s, hipEventRecord(s->rfi.ev[0], s->stream));
    return PB_OK;
}

void search_series_launch(pb_search *s, const uint32_t *D, uint64_t *P, float *stats, int nrow, int tout)
{
    k_prefix<<<nrow, 256, 0, s->stream>>>(D, P, tout, s->tpitch, s->ppitch());
    k_series_stats<<<nrow, 256, 0, s->stream>>>(D, P, stats, tout, s->baseline, s->tpitch, s->ppitch());
}

void search_boxcar_launch(pb_search *s, const uint64_t *P, const float *stats, float *snr, uint8_t *wid, int nrow, int tout)
{
    k_boxcar<<<dim3((tout + 255) / 256, nrow), 256, 0, s->stream>>>(P, stats, snr, wid, tout, s->nbox, s->baseline, s->tpitch,
                                                                    s->ppitch(), 0.f, nullptr, 0);
}

// From the channel-major block on: d_xt holds nsamp samples per channel and ev[2] has been recorded.  The cleaning (in
// place; `cleaned`: the block has been cleaned already and is read as it lies), dedispersion, prefix sums and
// statistics, boxcars.  What pb_search_run / pb_search_peaks run after their transpose, and pb_search_gulp_run /
// pb_search_gulp_peaks (search_stream.hip) on the accumulated block.
int search_block(pb_search *s, int nsamp, float thresh, bool want_peaks, bool cleaned)
{
    const int tout = nsamp - s->max_delay;
    s->rfi.ran = s->rfi.narrow || s->rfi.broad;
    // the channel stage (search_rfichan.hip) comes first; a block cleaned already keeps the results of its first search
    s->chan.launched = s->chan.tol > 0 && !cleaned;
    s->chan.ran = s->chan.launched || (s->chan.tol > 0 && s->chan.have);
    if (s->chan.launched) {
        const int rc = search_rfichan_launch(s, nsamp);
        if (rc) return rc;
    }
    if (s->chan.tol > 0 && !s->rfi.ran) SCHK(s, hipEventRecord(s->chan.ev[2], s->stream));
    if (s->rfi.ran && cleaned) {
        SCHK(s, hipEventRecord(s->rfi.ev[0], s->stream));
    } else if (s->rfi.ran) {
        const int rc = search_clean(s, nsamp);
        if (rc) return rc;
    }
    dim3 gd((tout + 255) / 256, s->ndm);
    dim3 gdd((tout + DDM_TILE - 1) / DDM_TILE, (s->ndm + DDM_DB - 1) / DDM_DB);
    k_dedisperse<<<gdd, 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->d_delay, s->d_D, s->nact, s->ndm, tout, s->tpitch, s->tpitch);
    SCHK(s, hipEventRecord(s->ev[3], s->stream));
    const size_t ppitch = s->ppitch();
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
    s->plane_tout = tout;
    return PB_OK;
}

static int search_run(pb_search *s, const void *codes, int codes_on_device, int nsamp, int nbit, float thresh,
                      bool want_peaks)
{
    if (!s || !codes) return PB_EINVAL;
    if (nsamp > s->max_samples || !(nbit == 8 || nbit == 4 || nbit == 2))
        return search_fail(s, "pb_search_run", "block too long or bad nbit");
    const int tout = nsamp - s->max_delay;
    if (tout < 64) return search_fail(s, "pb_search_run", "block shorter than the largest dispersion delay");
    SCHK(s, hipSetDevice(s->device));
    const bool pol = s->pol.max > 0;                    // the block is [nsamp][4][nchan] (pb_search_set_pol)
    if (pol && nbit != 8) return search_fail(s, "pb_search_run", "with polarisation on the block must be 8-bit");
    const size_t nbytes = (size_t)nsamp * s->nchan * nbit / 8 * (pol ? 4 : 1);
    const uint8_t *d_codes = (const uint8_t *)codes;
    s->gp.fill = 0;                                     // the transpose overwrites the accumulated block of the gulp stage
    s->gp.cleaned = 0;
    s->gp.tail_n = 0;
    SCHK(s, hipEventRecord(s->ev[0], s->stream));
    if (!codes_on_device) {
        uint8_t *stage = pol ? s->pol.d_codes : s->d_codes;
        SCHK(s, hipMemcpyAsync(stage, codes, nbytes, hipMemcpyHostToDevice, s->stream));
        d_codes = stage;
    }
    SCHK(s, hipEventRecord(s->ev[1], s->stream));
    if (pol) {
        const int rc = search_pol_transpose(s, d_codes, nsamp);
        if (rc) return rc;
    } else {
        dim3 gt((nsamp + 63) / 64, (s->nchan + 63) / 64);
        k_transpose_codes<<<gt, 256, 0, s->stream>>>(d_codes, s->d_xt, nsamp, s->nchan, nbit, s->tpitch);
    }
    SCHK(s, hipEventRecord(s->ev[2], s->stream));
    return search_block(s, nsamp, thresh, want_peaks, false);
}

// after the run's last event: stage times, and the cleaning's time and counts (the dedispersion stage starts where
// the cleaning ends)
static int search_times(pb_search *s)
{
    // the dedispersion starts where the cleaning window ends: after narrow / broad, else after the channel stage
    hipEvent_t dd = s->rfi.ran ? s->rfi.ev[0] : (s->chan.tol > 0 ? s->chan.ev[2] : s->ev[2]);
    for (int i = 0; i < 6; ++i) s->ms[i] = search_ms(i == 2 ? dd : s->ev[i], s->ev[i + 1]);
    s->rfi.n_narrow = 0;
    s->rfi.n_broad = 0;
    s->rfi.ms = 0.f;
    if (s->rfi.ran) {
        unsigned long long c[2];
        SCHK(s, hipMemcpy(c, s->rfi.d_rcnt, sizeof c, hipMemcpyDeviceToHost));
        s->rfi.n_narrow = c[0];
        s->rfi.n_broad = (int)c[1];
        s->rfi.ms = search_ms(s->chan.launched ? s->chan.ev[1] : s->ev[2], s->rfi.ev[0]);
    }
    return PB_OK;
}

// the planes, series and statistics of the run that was just queued -> host, then the stage times
int search_run_out(pb_search *s, float *snr, uint8_t *width_log2, uint32_t *series, float *stats, int *tout_out)
{
    const int tout = s->last_tout;
    SCHK(s, hipStreamSynchronize(s->stream));
    if (snr) SCHK(s, hipMemcpy2D(snr, tout * sizeof(float), s->d_snr, s->tpitch * sizeof(float), tout * sizeof(float), s->ndm, hipMemcpyDeviceToHost));
    if (width_log2) SCHK(s, hipMemcpy2D(width_log2, tout, s->d_wid, s->tpitch, tout, s->ndm, hipMemcpyDeviceToHost));
    if (series) SCHK(s, hipMemcpy2D(series, tout * sizeof(uint32_t), s->d_D, s->tpitch * sizeof(uint32_t), tout * sizeof(uint32_t), s->ndm, hipMemcpyDeviceToHost));
    if (stats) SCHK(s, hipMemcpy(stats, s->d_stats, (size_t)s->ndm * 2 * sizeof(float), hipMemcpyDeviceToHost));
    SCHK(s, hipEventRecord(s->ev[6], s->stream));
    SCHK(s, hipEventSynchronize(s->ev[6]));
    const int rc = search_times(s);
    if (rc) return rc;
    if (tout_out) *tout_out = tout;
    return PB_OK;
}

// the peak list of the run that was just queued -> host, then the stage times
int search_peaks_out(pb_search *s, int32_t *peaks, int max_out, int *npeaks, int *tout_out)
{
    int32_t n = 0;
    SCHK(s, hipMemcpyAsync(&n, s->d_peaks, sizeof n, hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipStreamSynchronize(s->stream));
    const int ncopy = std::min(std::min((int)n, max_out), s->max_peaks);      // never past the device list
    if (ncopy > 0) SCHK(s, hipMemcpy(peaks, s->d_peaks + 1, (size_t)ncopy * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    SCHK(s, hipEventRecord(s->ev[6], s->stream));
    SCHK(s, hipEventSynchronize(s->ev[6]));
    const int rc = search_times(s);
    if (rc) return rc;
    *npeaks = n;
    if (tout_out) *tout_out = s->last_tout;
    return PB_OK;
}

// codes: nsamp x nchan samples of nbit bits in SIGPROC order (host, or device if codes_on_device).
// Outputs (host, any may be NULL): snr [ndm][tout] float, width_log2 [ndm][tout] u8,
// series [ndm][tout] u32 (the dedispersed sums), stats [ndm][2]; tout = nsamp - max_delay.
extern "C" int pb_search_run(pb_search *s, const void *codes, int codes_on_device, int nsamp, int nbit, float *snr,
                             uint8_t *width_log2, uint32_t *series, float *stats, int *tout_out)
{
    const int rc = search_run(s, codes, codes_on_device, nsamp, nbit, 0.f, false);
    return rc ? rc : search_run_out(s, snr, width_log2, series, stats, tout_out);
}

// The search as the production chain uses it: only the (DM, sample) points at or above `threshold` come back
// (what heimdall's giant finder starts from), not the S/N planes: peaks[4 i ..] = DM index, sample, S/N
// (float bits), log2 width; *npeaks may exceed max_out when the list was truncated.  The list is in arrival order
// and holds max_peaks points; the giant finder and the labelling themselves are pb_search_giants, on the planes.
extern "C" int pb_search_peaks(pb_search *s, const void *codes, int codes_on_device, int nsamp, int nbit,
                               float threshold, int32_t *peaks, int max_out, int *npeaks, int *tout_out)
{
    if (!peaks || !npeaks || max_out < 1) return PB_EINVAL;
    const int rc = search_run(s, codes, codes_on_device, nsamp, nbit, threshold, true);
    return rc ? rc : search_peaks_out(s, peaks, max_out, npeaks, tout_out);
}

extern "C" int pb_search_timers(const pb_search *s, float *ms6)
{
    return search_get_ms(s, s ? s->ms : nullptr, 6, ms6);
}

extern "C" int pb_search_rfi_info(const pb_search *s, uint64_t *n_narrow, int *n_broad_samples, float *ms)
{
    if (!s) return PB_EINVAL;
    if (n_narrow) *n_narrow = s->rfi.n_narrow;
    if (n_broad_samples) *n_broad_samples = s->rfi.n_broad;
    if (ms) *ms = s->rfi.ms;
    return PB_OK;
}

extern "C" int pb_search_fetch_clean(pb_search *s, uint8_t *xt, size_t nbytes)
{
    if (!s || !xt) return PB_EINVAL;
    const size_t n = s->last_nsamp;
    if (n == 0 || nbytes < n * s->nchan)
        return search_fail(s, "pb_search_fetch_clean", "no block searched yet, or the buffer is smaller than nchan x nsamp");
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    SCHK(s, hipMemcpy2D(xt, n, s->d_xt, s->tpitch, n, s->nchan, hipMemcpyDeviceToHost));
    return PB_OK;
}
