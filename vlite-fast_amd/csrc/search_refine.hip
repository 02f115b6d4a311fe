// A candidate's DM, width and S/N refined on a fine DM grid with the reference's estimator (analysis/loc_step0.py:
// refine_dm, optimize_pulse), from the block that a run leaves on the device (definition: include/pb_hip.h,
// pb_search_set_refine / pb_search_refine): k_refine_series, k_refine_dm, k_refine_width, their LDS sort and Qn, and
// their host side.  Plain HIP C++ throughout.
#include "search_internal.h"
#include "search_dev.h"

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
// evaluated).  A lane takes 8 consecutive samples through the byte gather of search_dev.h, as k_dedisperse does;
// P = ceil(L / 8) lanes side by side cover the series and the 256 / P groups of them share the channels; the groups'
// sums meet in LDS.  The delays of RF_CH channels at a time are made in LDS by the whole workgroup with
// delay_samples, the function the trial DMs' table is made with.
// Reads: a live lane has a sample t in [0, tout), and t + delay <= tout - 1 + max_delay = nsamp - 1 (the trial's DM is
// not above the grid's last, and the delay grows with the DM); its first byte is at most 7 below that, possibly
// before the row: the guarded load.  What it sums for its samples outside [0, tout) is never written out.
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
                gather_load_guarded<2>(xt, (long long)chans[c0 + ii] * (long long)tpitch + (long long)(s0 & ~3), w[q]);
            }
#pragma unroll
            for (int q = 0; q < RF_CU; ++q) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const uint32_t a = gather_align(w[q][e], w[q][e + 1], sh[q]);
                    lo[e] += a & 0x00ff00ffu;
                    hi[e] += (a >> 8) & 0x00ff00ffu;
                }
            }
            since += RF_CU;
            if (since >= GATHER_FLUSH) {
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
    return block_sum(c, sh);
}

// Qn of the ascending s[0 .. n), n >= 2: 2.2219 x the 25th percentile of the np = n (n - 1) / 2 absolute pair differences,
// interpolated as np.percentile does -- position (np - 1) / 4 = r + f / 4, value d[r] + (f / 4) (d[r + 1] - d[r]), exact
// in double for integers.  d[r] by bisection on the value over the count of pairs at or below it; d[r + 1] is d[r] when
// more than r + 1 pairs are at or below d[r], else the smallest difference above it.  Uniform over the workgroup.
__device__ __forceinline__ double refine_qn(const uint32_t *s, int n, uint32_t *sh, unsigned long long *sh64)
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
        dhi = (uint32_t)~block_max(best, sh64);
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
    __shared__ unsigned long long sh64[4];
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
    key = block_max(key, sh64);
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
    __shared__ unsigned long long sh64[4];
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
    vkey = block_max(vkey, sh64);
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
    const int kb = (int)~block_max(ikey, sh64);
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
        key = block_max(key, sh64);
        if (threadIdx.x == 0) {
            const double mean = (double)(uint32_t)(key >> 32) / (double)w;
            opt_loc[(size_t)cand * nw + iw] = (int32_t)(0xffffffffu - (uint32_t)key);
            opt_sn[(size_t)cand * nw + iw] = qn > 0.0 ? (mean - med) / qn * sqrt((double)w) : 0.0;
        }
    }
}

// One call's staging buffer, as offsets in 32-bit words: sn_dm [n][nstep] and opt_sn [n][nw] (double, at even
// offsets), kbest [n] and opt_loc [n][nw] (i32), then the fine series about each peak [n][nstep][2 (H + M)] (u32); the
// page-locked copy holds the same and then the requests' integers [n][4] and floats [n][2].  One buffer, so one copy:
// everything below `ser`, or below `reqi` when the series is asked for.
struct refine_layout {
    size_t sn, osn, kb, loc, ser, reqi, reqf, total;
};

static refine_layout refine_layout_of(const pb_search *s, size_t n)
{
    const size_t nw = s->rf.wmax / 2, L = 2 * ((size_t)s->rf.H + nw);
    refine_layout l;
    l.sn = 0;
    l.osn = l.sn + 2 * n * s->rf.nstep;
    l.kb = l.osn + 2 * n * nw;
    l.loc = l.kb + n;
    l.ser = l.loc + n * nw;
    l.reqi = l.ser + n * s->rf.nstep * L;
    l.reqf = l.reqi + 4 * n;
    l.total = l.reqf + 2 * n;
    return l;
}

void search_refine_free(pb_search *s)
{
    search_release({s->rf.d_g, s->rf.d_reqi, s->rf.d_reqf, s->rf.d_out}, s->rf.h_out, s->rf.ev, 3);
    s->rf = {};
}

extern "C" int pb_search_set_refine(pb_search *s, int nstep, int half_window, int wmax, int max_cands)
{
    const char *fn = "pb_search_set_refine";
    if (!s) return search_fail(s, fn, "no search handle");
    if (max_cands < 0) return search_fail(s, fn, "max_cands must be >= 0");
    if (max_cands > 0) {
        if (nstep < 1 || nstep > 4096) return search_fail(s, fn, "nstep must be in 1..4096");
        if (wmax < 2 || wmax > 64 || (wmax & 1)) return search_fail(s, fn, "wmax must be even and in 2..64");
        if (half_window < 2 * wmax || 2 * (half_window + wmax / 2) > RF_MAXL)
            return search_fail(s, fn, "half_window must be at least 2 wmax (a full window holds 4 wmax samples) and "
                                      "half_window + wmax / 2 at most 1024");
        if ((long long)s->nact * 255 * wmax >= (1ll << 32)) return search_fail(s, fn, "too many channels for 32-bit running sums");
        if ((long long)max_cands * nstep * 2 * (half_window + wmax / 2) > (1ll << 28))
            return search_fail(s, fn, "max_cands requests of this geometry exceed 1 GiB");
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    search_refine_free(s);
    if (max_cands == 0) return PB_OK;
    std::vector<int32_t> chans(s->nact);
    SCHK(s, hipMemcpy(chans.data(), s->d_chans, chans.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<double> g(s->nact);
    for (int k = 0; k < s->nact; ++k)
        g[k] = delay_chan_term((double)s->fch1 + (double)chans[k] * (double)s->foff, s->ftop);
    s->rf.nstep = nstep;
    s->rf.H = half_window;
    s->rf.wmax = wmax;
    const refine_layout M = refine_layout_of(s, (size_t)max_cands);
    hipError_t e = hipMalloc((void **)&s->rf.d_g, g.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(s->rf.d_g, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->rf.d_reqi, (size_t)max_cands * 4 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->rf.d_reqf, (size_t)max_cands * 2 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&s->rf.d_out, M.reqi * sizeof(int32_t));
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->rf.h_out, M.total * sizeof(int32_t), hipHostMallocDefault);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&s->rf.ev[i]);
    if (e != hipSuccess) {
        search_refine_free(s);
        s->err = std::string("pb_search_set_refine: ") + hipGetErrorString(e);
        return PB_EHIP;
    }
    s->rf.max = max_cands;                  // (last: the stage is on only once everything exists)
    return PB_OK;
}

extern "C" int pb_search_refine(pb_search *s, const int32_t *req_i2, const float *req_f2, int n, int32_t *status,
                                double *sn_dm, int32_t *kbest, double *opt_sn, int32_t *opt_loc, uint32_t *series)
{
    const char *fn = "pb_search_refine";
    if (int rc = search_enter(s, fn, s && s->rf.max, "refinement is not switched on (pb_search_set_refine)",
                              s && s->last_nsamp, "no block searched yet"))
        return rc;
    if (!req_i2 || !req_f2 || n < 0 || n > s->rf.max) return search_fail(s, fn, "no request list, or more requests than max_cands");
    const int T = s->last_tout, H = s->rf.H, M = s->rf.wmax / 2, nstep = s->rf.nstep, nw = M;
    for (int i = 0; i < n; ++i) {
        const int t = req_i2[2 * i], w = req_i2[2 * i + 1];
        if (t < 0 || t >= T || w < 1 || w > s->rf.wmax || !std::isfinite(req_f2[2 * i]) || !std::isfinite(req_f2[2 * i + 1]))
            return search_fail(s, fn, "request " + std::to_string(i) + " out of range (peak sample in [0, tout) of the last "
                                      "run, width in 1..wmax, dm_lo and dm_step finite)");
    }
    if (n == 0) return PB_OK;
    const refine_layout l = refine_layout_of(s, (size_t)n), lmax = refine_layout_of(s, (size_t)s->rf.max);
    int32_t *d = s->rf.d_out, *h = s->rf.h_out;
    int32_t *h_reqi = h + lmax.reqi;
    float *h_reqf = (float *)(h + lmax.reqf);
    std::vector<int32_t> st(n);
    for (int i = 0; i < n; ++i) {
        const int t = req_i2[2 * i], w = req_i2[2 * i + 1];
        st[i] = std::min(T, t + H) - std::max(0, t - H) < 4 * s->rf.wmax ? 1 : 0;
        h_reqi[4 * i] = t;
        h_reqi[4 * i + 1] = w | 1;                                      // an even width becomes width + 1
        h_reqi[4 * i + 2] = st[i];
        h_reqi[4 * i + 3] = 0;
        h_reqf[2 * i] = req_f2[2 * i];
        h_reqf[2 * i + 1] = req_f2[2 * i + 1];
    }
    double *d_sn = (double *)(d + l.sn), *d_osn = (double *)(d + l.osn);
    uint32_t *d_ser = (uint32_t *)(d + l.ser);
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipMemcpyAsync(s->rf.d_reqi, h_reqi, (size_t)n * 4 * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    SCHK(s, hipMemcpyAsync(s->rf.d_reqf, h_reqf, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, s->stream));
    SCHK(s, hipEventRecord(s->rf.ev[0], s->stream));
    k_refine_series<<<dim3(nstep, n), 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->rf.d_g, s->rf.d_reqi, s->rf.d_reqf, d_ser,
                                                           s->nact, T, 2 * (H + M), H + M, (double)s->tsamp, s->dm_last, s->tpitch);
    k_refine_dm<<<dim3(nstep, n), 256, 0, s->stream>>>(d_ser, s->rf.d_reqi, s->rf.d_reqf, d_sn, T, H, M, s->dm_last);
    k_refine_width<<<n, 256, 0, s->stream>>>(d_ser, s->rf.d_reqi, d_sn, d + l.kb, d_osn, d + l.loc, T, H, M, nstep, nw);
    SCHK(s, hipEventRecord(s->rf.ev[1], s->stream));
    SCHK(s, hipMemcpyAsync(h, d, (series ? l.reqi : l.ser) * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipEventRecord(s->rf.ev[2], s->stream));
    SCHK(s, hipGetLastError());
    SCHK(s, hipEventSynchronize(s->rf.ev[2]));
    for (int i = 0; i < 2; ++i) s->rf.ms[i] = search_ms(s->rf.ev[0], s->rf.ev[i + 1]);
    auto fetch = [&](void *dst, size_t from, size_t to) {               // the words [from, to) of the copy
        if (dst) memcpy(dst, h + from, (to - from) * sizeof(int32_t));
    };
    if (status) memcpy(status, st.data(), (size_t)n * sizeof(int32_t));
    fetch(sn_dm, l.sn, l.osn);
    fetch(opt_sn, l.osn, l.kb);
    fetch(kbest, l.kb, l.loc);
    fetch(opt_loc, l.loc, l.ser);
    fetch(series, l.ser, l.reqi);
    return PB_OK;
}

extern "C" int pb_search_refine_timers(const pb_search *s, float *ms2) { return search_get_ms(s, s ? s->rf.ms : nullptr, 2, ms2); }
