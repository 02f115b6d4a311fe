// Sub-band search of the block that a run leaves on the device (definition: include/pb_hip.h, pb_search_set_subbands /
// pb_search_subbands): k_dedisperse_sub, k_band_sum, k_band_best and their host side.  The statistics and boxcars of a band
// are the core's own kernels on the band rows (search_series_launch, search_boxcar_launch: search_run.hip).
#include "search_internal.h"
#include "search_dev.h"

// k_dedisperse's tiling (search_run.hip): 2048 output samples x 4 neighbouring trial DMs per workgroup, 8 samples per lane
#define SBD_DB 4
#define SBD_SAMPLES 8
#define SBD_CU 4          // channels whose loads are in flight together
#define SBD_TILE (256 * SBD_SAMPLES)

// Dedispersion per base sub-band: grid (time tile, block of SBD_DB rows of the chunk, sub-band).  A workgroup sums the run
// [first, last) of chans[] that is its sub-band (subrun: [nsb][2]) for the chunk's rows r0 .. r0 + 3 = the trial DMs
// dm0 + r0 .. and writes S[sub][row][t], S laid out [nsb][nrow][dpitch].  This is k_dedisperse's byte gather with the
// channel loop cut to one run: every unzapped channel is in exactly one sub-band, so the byte planes are read as often as
// the main dedispersion reads them.  The two invariants of search_dev.h:
//   Reads.  A live lane has t <= tout - 1 and every delay of the main table is <= max_delay, so its first byte is at
//           t + d <= tout - 1 + max_delay = nsamp - 1 (tout is the last search's: nsamp - max_delay).
//   16 bits.  `since` counts the channels added since the last flush in steps of SBD_CU = 4 and flushes at GATHER_FLUSH =
//           240, so at most 240 channels go in between two flushes of the loop; after the last check `since` is at most
//           236 and the tail adds at most SBD_CU - 1 = 3 more before the final flush: never more than 254 channels.
// An empty run adds nothing and the zeros are written.
__global__ __launch_bounds__(256) void k_dedisperse_sub(const uint8_t *__restrict__ xt, const int32_t *__restrict__ chans,
                                                        const int32_t *__restrict__ delay, const int32_t *__restrict__ subrun,
                                                        uint32_t *__restrict__ S, int nact, int dm0, int nrow, int tout,
                                                        size_t tpitch, size_t dpitch)
{
    const int r0 = blockIdx.y * SBD_DB, sub = blockIdx.z;
    const int t = blockIdx.x * SBD_TILE + threadIdx.x * SBD_SAMPLES;      // 4-byte aligned (tpitch is a multiple of 64)
    if (t >= tout) return;                                                // no barrier in this kernel: a whole-lane exit is safe
    const int first = subrun[2 * sub], last = subrun[2 * sub + 1];
    uint32_t lo[SBD_DB][SBD_SAMPLES / 4], hi[SBD_DB][SBD_SAMPLES / 4];   // packed u16 partial sums: bytes 0,2 / 1,3
    uint32_t acc[SBD_DB][SBD_SAMPLES];
    const int32_t *dl[SBD_DB];
#pragma unroll
    for (int j = 0; j < SBD_DB; ++j) {
        dl[j] = delay + (size_t)(dm0 + (r0 + j < nrow ? r0 + j : nrow - 1)) * nact;
#pragma unroll
        for (int w = 0; w < SBD_SAMPLES / 4; ++w) lo[j][w] = hi[j][w] = 0u;
#pragma unroll
        for (int i = 0; i < SBD_SAMPLES; ++i) acc[j][i] = 0u;
    }
    auto flush = [&]() {
#pragma unroll
        for (int j = 0; j < SBD_DB; ++j) {
#pragma unroll
            for (int w = 0; w < SBD_SAMPLES / 4; ++w) {
                acc[j][4 * w + 0] += lo[j][w] & 0xffffu;
                acc[j][4 * w + 1] += hi[j][w] & 0xffffu;
                acc[j][4 * w + 2] += lo[j][w] >> 16;
                acc[j][4 * w + 3] += hi[j][w] >> 16;
                lo[j][w] = hi[j][w] = 0u;
            }
        }
    };
    // one channel of one DM: samples t+d .. t+d+SBD_SAMPLES-1 = SBD_SAMPLES/4 + 1 aligned dwords from (t + d) & ~3
    auto fetch = [&](int c, int j, uint32_t (&w)[SBD_SAMPLES / 4 + 1], unsigned &sh) {
        const int32_t d = dl[j][c];                                 // uniform -> scalar load
        const uint32_t *p = (const uint32_t *)(xt + (size_t)chans[c] * tpitch + t + (d & ~3));
#pragma unroll
        for (int i = 0; i <= SBD_SAMPLES / 4; ++i) w[i] = p[i];
        sh = (unsigned)(d & 3);
    };
    auto add = [&](int j, const uint32_t (&w)[SBD_SAMPLES / 4 + 1], unsigned sh) {
#pragma unroll
        for (int i = 0; i < SBD_SAMPLES / 4; ++i) {
            const uint32_t a = gather_align(w[i], w[i + 1], sh);
            lo[j][i] += a & 0x00ff00ffu;
            hi[j][i] += (a >> 8) & 0x00ff00ffu;
        }
    };
    int c = first, since = 0;
    for (; c + SBD_CU <= last; c += SBD_CU) {
        uint32_t w[SBD_CU][SBD_DB][SBD_SAMPLES / 4 + 1];
        unsigned sh[SBD_CU][SBD_DB];
#pragma unroll
        for (int u = 0; u < SBD_CU; ++u)
#pragma unroll
            for (int j = 0; j < SBD_DB; ++j) fetch(c + u, j, w[u][j], sh[u][j]);
#pragma unroll
        for (int u = 0; u < SBD_CU; ++u)
#pragma unroll
            for (int j = 0; j < SBD_DB; ++j) add(j, w[u][j], sh[u][j]);
        since += SBD_CU;
        if (since >= GATHER_FLUSH) {
            flush();
            since = 0;
        }
    }
    for (; c < last; ++c) {
#pragma unroll
        for (int j = 0; j < SBD_DB; ++j) {
            uint32_t w[SBD_SAMPLES / 4 + 1];
            unsigned sh;
            fetch(c, j, w, sh);
            add(j, w, sh);
        }
    }
    flush();
#pragma unroll
    for (int j = 0; j < SBD_DB; ++j) {
        if (r0 + j >= nrow) break;
        uint32_t *out = S + ((size_t)sub * nrow + r0 + j) * dpitch + t;
#pragma unroll
        for (int i = 0; i < SBD_SAMPLES; i += 4) {
            if (t + i + 4 <= tout) {
                *(uint4 *)(out + i) = make_uint4(acc[j][i], acc[j][i + 1], acc[j][i + 2], acc[j][i + 3]);
            } else {
                for (int q = 0; q < 4; ++q)
                    if (t + i + q < tout) out[i + q] = acc[j][i + q];
            }
        }
    }
}

// Band series: grid (4 x 256 samples, row of the chunk, band).  B[band][row][t] = the sum of S[s][row][t] over the band's base
// sub-bands (bands: [nbands][2] = first, count), four samples per lane; exact u32.
__global__ __launch_bounds__(256) void k_band_sum(const uint32_t *__restrict__ S, const int32_t *__restrict__ bands,
                                                  uint32_t *__restrict__ B, int nrow, int tout, size_t dpitch)
{
    const int t = (blockIdx.x * 256 + threadIdx.x) * 4, r = blockIdx.y, b = blockIdx.z;
    if (t >= tout) return;
    const int first = bands[2 * b], count = bands[2 * b + 1];
    const bool whole = t + 4 <= tout;
    uint32_t a[4] = {0u, 0u, 0u, 0u};
    for (int s = first; s < first + count; ++s) {
        const uint32_t *x = S + ((size_t)s * nrow + r) * dpitch + t;
        if (whole) {
            const uint4 v = *(const uint4 *)x;
            a[0] += v.x;
            a[1] += v.y;
            a[2] += v.z;
            a[3] += v.w;
        } else {
            for (int q = 0; q < 4; ++q)
                if (t + q < tout) a[q] += x[q];
        }
    }
    uint32_t *out = B + ((size_t)b * nrow + r) * dpitch + t;
    if (whole) {
        *(uint4 *)out = make_uint4(a[0], a[1], a[2], a[3]);
    } else {
        for (int q = 0; q < 4; ++q)
            if (t + q < tout) out[q] = a[q];
    }
}

// Best band per cell and the points: grid (256 samples, row of the chunk).  bsnr, bwid: the band planes [nbands][nrow][dpitch];
// fsnr: the full-band S/N planes [ndm][dpitch], row dm0 + r.  The best band is band 0 unless a later one is larger in
// binary32 (a tie, -0 against +0 included, keeps the smaller index) or the best so far is a NaN and the later one is not.
// A cell inside [t_lo, t_hi) whose best S/N is >= thresh and > the full-band S/N is appended to pts (count word, then
// PB_SUBPOINT_WORDS words per point, the first max_pts of them in arrival order; the count is exact).  obest .. oband: the
// best planes of row best_row for pb_search_subband_dm, else null.
__global__ __launch_bounds__(256) void k_band_best(const float *__restrict__ bsnr, const uint8_t *__restrict__ bwid,
                                                   const float *__restrict__ fsnr, int nbands, int nrow, int dm0, int tout,
                                                   size_t dpitch, float thresh, int t_lo, int t_hi, int32_t *__restrict__ pts,
                                                   int max_pts, int best_row, float *__restrict__ obest,
                                                   uint8_t *__restrict__ owid, uint8_t *__restrict__ oband)
{
    const int t = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (t >= tout) return;
    float best = bsnr[(size_t)r * dpitch + t];
    int bi = 0;
    for (int b = 1; b < nbands; ++b) {
        const float v = bsnr[((size_t)b * nrow + r) * dpitch + t];
        if (v > best || (best != best && v == v)) {
            best = v;
            bi = b;
        }
    }
    const int wl = bwid[((size_t)bi * nrow + r) * dpitch + t];
    if (obest && r == best_row) {
        obest[t] = best;
        owid[t] = (uint8_t)wl;
        oband[t] = (uint8_t)bi;
    }
    if (!pts || t < t_lo || t >= t_hi) return;
    const float full = fsnr[(size_t)(dm0 + r) * dpitch + t];
    if (best >= thresh && best > full) {
        const int i = atomicAdd(pts, 1);
        if (i < max_pts) {
            int32_t *p = pts + 1 + (size_t)PB_SUBPOINT_WORDS * i;
            p[0] = dm0 + r;
            p[1] = t;
            p[2] = __float_as_int(best);
            p[3] = wl;
            p[4] = bi;
            p[5] = __float_as_int(full);
        }
    }
}

#define SUB_MAX_BANDS 64
#define SUB_BUDGET (1ull << 30)         // dm_chunk = 0: the stage's buffers stay within this

void search_subbands_free(pb_search *s)
{
    search_release({s->sub.d_run, s->sub.d_bands, s->sub.d_S, s->sub.d_B, s->sub.d_P, s->sub.d_stats, s->sub.d_snr, s->sub.d_wid,
                    s->sub.d_pts, s->sub.d_best, s->sub.d_bestw},
                   nullptr, s->sub.ev.data(), (int)s->sub.ev.size());
    s->sub = {};
}

extern "C" int pb_search_set_subbands(pb_search *s, int nsb, const int32_t *bands2, int nbands, int dm_chunk, int max_points)
{
    const char *fn = "pb_search_set_subbands";
    if (!s) return search_fail(s, fn, "no search handle");
    if (nbands < 0 || nbands > SUB_MAX_BANDS) return search_fail(s, fn, "nbands must be in 0..64");
    if (nbands > 0) {
        if (s->pol.max > 0) return search_fail(s, fn, "not with polarisation switched on (pb_search_set_pol)");
        if (!(nsb == 2 || nsb == 4 || nsb == 8 || nsb == 16) || s->nchan % nsb)
            return search_fail(s, fn, "nsb must be 2, 4, 8 or 16 and divide the number of channels");
        if (!bands2) return search_fail(s, fn, "no band list");
        for (int b = 0; b < nbands; ++b) {
            const int first = bands2[2 * b], count = bands2[2 * b + 1];
            if (first < 0 || count < 1 || count >= nsb || first + count > nsb)
                return search_fail(s, fn, "band " + std::to_string(b) + " is not a run (first, count) of base sub-bands with "
                                          "1 <= count < nsb inside the band (the whole band is the ordinary search)");
        }
        if (dm_chunk < 0 || max_points < 1 || max_points > (1 << 26))
            return search_fail(s, fn, "dm_chunk must be >= 0 and max_points in 1..2^26");
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    search_subbands_free(s);
    if (nbands == 0) return PB_OK;
    std::vector<int32_t> run;
    if (int rc = search_sub_runs(s, nsb, run)) return rc;
    // bytes of the stage per trial DM of a chunk: S, and per band B, P, S/N, width, statistics
    const size_t tp = s->tpitch, pp = s->ppitch();
    const size_t per = (size_t)nsb * tp * 4 + (size_t)nbands * (tp * 4 + pp * 8 + tp * 4 + tp + 8);
    int chunk = dm_chunk;
    if (chunk == 0) chunk = std::max(4, (int)std::min<size_t>(SUB_BUDGET / per, 1u << 20) & ~3);
    chunk = std::min(chunk, 65535 / nbands);            // k_boxcar has the band rows in the grid's y
    chunk = std::min(chunk, s->ndm);
    const size_t rows = (size_t)chunk * nbands;
    const int nchunk = (s->ndm + chunk - 1) / chunk;
    hipError_t e = hipMalloc((void **)&s->sub.d_run, run.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(s->sub.d_run, run.data(), run.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->sub.d_bands, (size_t)nbands * 2 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(s->sub.d_bands, bands2, (size_t)nbands * 2 * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->sub.d_S, (size_t)nsb * chunk * tp * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->sub.d_B, rows * tp * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->sub.d_P, rows * pp * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->sub.d_stats, rows * 2 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&s->sub.d_snr, rows * tp * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&s->sub.d_wid, rows * tp);
    if (e == hipSuccess) e = hipMalloc((void **)&s->sub.d_pts, (1 + (size_t)PB_SUBPOINT_WORDS * max_points) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->sub.d_best, tp * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&s->sub.d_bestw, 2 * tp);
    s->sub.ev.assign(3 * (size_t)nchunk + 2, nullptr);  // per chunk: start, dedispersed, statistics; then kernels done, copy done
    for (size_t i = 0; i < s->sub.ev.size() && e == hipSuccess; ++i) e = hipEventCreate(&s->sub.ev[i]);
    if (e != hipSuccess) {
        search_subbands_free(s);
        s->err = std::string("pb_search_set_subbands: ") + hipGetErrorString(e);
        return PB_EHIP;
    }
    s->sub.nsb = nsb;
    s->sub.chunk = chunk;
    s->sub.max = max_points;
    s->sub.nbands = nbands;                 // (last: the stage is on only once everything exists)
    return PB_OK;
}

// The stage's kernels on the nrow trial DMs from dm0 on (nrow <= chunk); where ev is not null, ev[1] is recorded behind the
// dedispersion and ev[2] behind the statistics.  want_pts: append the points; best_row >= 0: keep that row's best planes
// (pb_search_subband_dm).
static int sub_rows(pb_search *s, int dm0, int nrow, float thresh, int t_lo, int t_hi, bool want_pts, int best_row,
                    hipEvent_t *ev)
{
    const int tout = s->last_tout, nb = s->sub.nbands;
    const size_t tp = s->tpitch;
    dim3 gd((tout + SBD_TILE - 1) / SBD_TILE, (nrow + SBD_DB - 1) / SBD_DB, s->sub.nsb);
    k_dedisperse_sub<<<gd, 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->d_delay, s->sub.d_run, s->sub.d_S, s->nact, dm0, nrow,
                                                tout, tp, tp);
    if (ev) SCHK(s, hipEventRecord(ev[1], s->stream));
    dim3 gs((tout + 1023) / 1024, nrow, nb);
    k_band_sum<<<gs, 256, 0, s->stream>>>(s->sub.d_S, s->sub.d_bands, s->sub.d_B, nrow, tout, tp);
    search_series_launch(s, s->sub.d_B, s->sub.d_P, s->sub.d_stats, nrow * nb, tout);
    if (ev) SCHK(s, hipEventRecord(ev[2], s->stream));
    search_boxcar_launch(s, s->sub.d_P, s->sub.d_stats, s->sub.d_snr, s->sub.d_wid, nrow * nb, tout);
    dim3 gb((tout + 255) / 256, nrow);
    k_band_best<<<gb, 256, 0, s->stream>>>(s->sub.d_snr, s->sub.d_wid, s->d_snr, nb, nrow, dm0, tout, tp, thresh, t_lo, t_hi,
                                           want_pts ? s->sub.d_pts : nullptr, s->sub.max, best_row,
                                           best_row >= 0 ? s->sub.d_best : nullptr, s->sub.d_bestw, s->sub.d_bestw + tp);
    return PB_OK;
}

// the checks that pb_search_subbands and pb_search_subband_dm share
static int sub_enter(pb_search *s, const char *fn)
{
    if (int rc = search_enter(s, fn, s && s->sub.nbands, "the sub-band search is not switched on (pb_search_set_subbands)",
                              s && s->last_nsamp, "no block searched yet"))
        return rc;
    if (s->pol.max > 0) return search_fail(s, fn, "not with polarisation switched on (pb_search_set_pol)");
    if (s->plane_tout != s->last_tout)
        return search_fail(s, fn, "the planes on the device are not the last search's (pb_search_set_planes replaced them)");
    return PB_OK;
}

extern "C" int pb_search_subbands(pb_search *s, float thresh, int t_lo, int t_hi, int32_t *points, int max_out, int *npoints,
                                  int *overflow)
{
    const char *fn = "pb_search_subbands";
    if (int rc = sub_enter(s, fn)) return rc;
    if (!points || !npoints || !overflow || max_out < 1) return search_fail(s, fn, "an output pointer is missing, or max_out < 1");
    if (thresh != thresh) return search_fail(s, fn, "the threshold is a NaN");
    if (t_lo < 0 || t_hi <= t_lo || t_hi > s->last_tout) return search_fail(s, fn, "need 0 <= t_lo < t_hi <= tout of the last search");
    SCHK(s, hipSetDevice(s->device));
    hipEvent_t *ev = s->sub.ev.data();
    const int chunk = s->sub.chunk;
    int k = 0;
    SCHK(s, hipMemsetAsync(s->sub.d_pts, 0, sizeof(int32_t), s->stream));
    for (int dm0 = 0; dm0 < s->ndm; dm0 += chunk, ++k) {
        SCHK(s, hipEventRecord(ev[3 * k], s->stream));
        if (int rc = sub_rows(s, dm0, std::min(chunk, s->ndm - dm0), thresh, t_lo, t_hi, true, -1, ev + 3 * k)) return rc;
    }
    SCHK(s, hipEventRecord(ev[3 * k], s->stream));
    SCHK(s, hipGetLastError());
    int32_t n = 0;
    SCHK(s, hipMemcpyAsync(&n, s->sub.d_pts, sizeof n, hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipStreamSynchronize(s->stream));
    const int cap = std::min(max_out, s->sub.max);
    const int ncopy = std::min((int)n, cap);
    if (ncopy > 0)
        SCHK(s, hipMemcpyAsync(points, s->sub.d_pts + 1, (size_t)ncopy * PB_SUBPOINT_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipEventRecord(ev[3 * k + 1], s->stream));
    SCHK(s, hipEventSynchronize(ev[3 * k + 1]));
    for (int i = 0; i < 3; ++i) s->sub.ms[i] = 0.f;
    for (int c = 0; c < k; ++c)
        for (int i = 0; i < 3; ++i) s->sub.ms[i] += search_ms(ev[3 * c + i], ev[3 * c + i + 1]);
    s->sub.ms[3] = search_ms(ev[0], ev[3 * k + 1]);
    *npoints = n;
    *overflow = n > cap;
    return PB_OK;
}

extern "C" int pb_search_subband_dm(pb_search *s, int dmi, uint32_t *sub, float *band_snr, uint8_t *band_wid, float *band_stats,
                                    float *best_snr, uint8_t *best_wid, uint8_t *best_band)
{
    const char *fn = "pb_search_subband_dm";
    if (int rc = sub_enter(s, fn)) return rc;
    if (dmi < 0 || dmi >= s->ndm) return search_fail(s, fn, "the DM index must be in [0, ndm)");
    SCHK(s, hipSetDevice(s->device));
    // the pass that pb_search_subbands makes over the chunk that holds dmi: row r of its nrow rows
    const int dm0 = dmi / s->sub.chunk * s->sub.chunk, r = dmi - dm0;
    const size_t nrow = std::min(s->sub.chunk, s->ndm - dm0);
    if (int rc = sub_rows(s, dm0, (int)nrow, 0.f, 0, 0, false, r, nullptr)) return rc;
    SCHK(s, hipGetLastError());
    SCHK(s, hipStreamSynchronize(s->stream));
    const size_t tout = s->last_tout, tp = s->tpitch, nb = s->sub.nbands;
    if (sub) SCHK(s, hipMemcpy2D(sub, tout * 4, s->sub.d_S + r * tp, nrow * tp * 4, tout * 4, s->sub.nsb, hipMemcpyDeviceToHost));
    if (band_snr) SCHK(s, hipMemcpy2D(band_snr, tout * 4, s->sub.d_snr + r * tp, nrow * tp * 4, tout * 4, nb, hipMemcpyDeviceToHost));
    if (band_wid) SCHK(s, hipMemcpy2D(band_wid, tout, s->sub.d_wid + r * tp, nrow * tp, tout, nb, hipMemcpyDeviceToHost));
    if (band_stats) SCHK(s, hipMemcpy2D(band_stats, 2 * sizeof(float), s->sub.d_stats + 2 * r, nrow * 2 * sizeof(float), 2 * sizeof(float), nb, hipMemcpyDeviceToHost));
    if (best_snr) SCHK(s, hipMemcpy(best_snr, s->sub.d_best, tout * 4, hipMemcpyDeviceToHost));
    if (best_wid) SCHK(s, hipMemcpy(best_wid, s->sub.d_bestw, tout, hipMemcpyDeviceToHost));
    if (best_band) SCHK(s, hipMemcpy(best_band, s->sub.d_bestw + tp, tout, hipMemcpyDeviceToHost));
    return PB_OK;
}

extern "C" int pb_search_subband_timers(const pb_search *s, float *ms4) { return search_get_ms(s, s ? s->sub.ms : nullptr, 4, ms4); }
