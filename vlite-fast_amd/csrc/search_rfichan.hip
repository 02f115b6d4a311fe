// The channel stage of the search's RFI cleaning (definition: include/pb_hip.h, pb_search_set_rfi_chan): channels whose
// spread over the whole block is an outlier among their neighbours' are flagged and filled with their rounded mean,
// before k_rfi_narrow and the broad pass.  Everything is exact integer arithmetic except the one binary64 comparison
// of k_rfichan_lag.  Four kernels, launched by search_rfichan_launch on the search's stream between the stage's two
// events:
//
//   k_rfichan_moments   one workgroup per unzapped channel: sum x and sum x^2 over [0, nsamp) with v_sad_u8 and
//                       v_dot4_u32_u8 on 16-byte loads -> sum[a], S[a] = nsamp sq - sum^2, fill[a]
//   k_rfichan_lag       one workgroup per signed lag: d[a] = S[a] - S[j(a)] sorted in LDS (bitonic, padded to a power of
//                       two with INT64_MAX), the three order statistics at the ranks of nact, the outlier bytes tab[l][a]
//   k_rfichan_vote      phase 0: recv[a] and cast[j(a)] counted from tab with integer atomics; phase 1 (a launch of its
//                       own: every count is final): mask[a] and nflag
//   k_rfichan_fill      one workgroup per unzapped channel, those that are not flagged leave at once: 16-byte stores of
//                       the splatted fill byte over [0, nsamp)
//
// What a lane may touch.  Rows: chans[a] < nchan for a < nact, a row is tpitch bytes, tpitch a multiple of 64 and
// >= max_samples >= nsamp.  k_rfichan_moments loads the 16-byte units u < ceil(nsamp / 16): the last one ends at
// 16 ceil(nsamp / 16) <= tpitch, inside the row, and its bytes at or beyond nsamp are masked to 0 before they are summed.
// k_rfichan_fill stores through stream_store16 with [lo, hi) = [0, nsamp): no byte at or beyond nsamp is written.  The
// per-channel arrays are indexed by a < nact (j(a) is clamped into [0, nact)), tab by l * nact + a with l < nlag.
//
// Limits (pb_search_set_rfi_chan refuses a handle beyond them).  RFICHAN_MAX_SAMPLES: a lane of k_rfichan_moments keeps
// u32 sums and widens them once, after its loop; it takes at most ceil(2^23 / 16 / 256) = 2048 units = 8192 dwords, one
// v_dot4_u32_u8 adds at most 4 x 255^2 = 260 100, so its sum stays below 8192 x 260 100 < 2^32 (16 512 dwords would be
// the end).  The same bound keeps 255^2 nsamp^2 < 2^63, so S, d, d - med and q3 - q1 are exact in int64.
// RFICHAN_MAX_NACT: the sort holds npad <= 8192 int64 = 64 KiB of LDS.
#include "search_internal.h"
#include "search_dev.h"

#include <climits>

#define RFICHAN_MAX_SAMPLES (1 << 23)
#define RFICHAN_MAX_NACT 8192
#define RFICHAN_MAX_LAGS 64             // 2 x 23 signed lags at radius 8192

// mom: [2][nact] = sum, S
__global__ __launch_bounds__(256) void k_rfichan_moments(const uint8_t *__restrict__ xt, const int32_t *__restrict__ chans,
                                                         int64_t *__restrict__ mom, uint8_t *__restrict__ fill, int nact,
                                                         int nsamp, size_t tpitch)
{
    __shared__ unsigned long long sh[4];
    const int a = blockIdx.x;
    const uint4 *rv = (const uint4 *)(xt + (size_t)chans[a] * tpitch);      // tpitch % 64 == 0: rows are 16-byte aligned
    const int nfull = nsamp >> 4, rem = nsamp & 15;
    uint32_t s1 = 0, s2 = 0;                                                // widened after the loop (RFICHAN_MAX_SAMPLES)
    for (int i = threadIdx.x; i < nfull; i += 256) {
        const uint4 v = rv[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s1 = __builtin_amdgcn_sad_u8(w[j], 0u, s1);
            s2 = __builtin_amdgcn_udot4(w[j], w[j], s2, false);
        }
    }
    if (rem && (int)threadIdx.x == (nfull & 255)) {
        // the partial last unit: inside the row's pitch; its bytes at or beyond nsamp count as 0
        const uint4 v = rv[nfull];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nb = min(max(rem - 4 * j, 0), 4);
            const uint32_t m = nb >= 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u;
            s1 = __builtin_amdgcn_sad_u8(w[j] & m, 0u, s1);
            s2 = __builtin_amdgcn_udot4(w[j] & m, w[j] & m, s2, false);
        }
    }
    const unsigned long long sum = block_sum((unsigned long long)s1, sh);
    const unsigned long long sq = block_sum((unsigned long long)s2, sh);
    if (threadIdx.x == 0) {
        const int64_t n = nsamp;
        mom[a] = (int64_t)sum;
        mom[nact + a] = n * (int64_t)sq - (int64_t)sum * (int64_t)sum;
        fill[a] = (uint8_t)((2 * (int64_t)sum + n) / (2 * n));
    }
}

// d[a] of the signed lag L
__device__ __forceinline__ int64_t rfichan_diff(const int64_t *__restrict__ S, int a, int L, int nact)
{
    return S[a] - S[min(max(a - L, 0), nact - 1)];
}

// One workgroup per signed lag; dynamic LDS: npad int64, npad = the power of two >= nact.
__global__ __launch_bounds__(256) void k_rfichan_lag(const int64_t *__restrict__ S, const int32_t *__restrict__ lags,
                                                     uint8_t *__restrict__ tab, int nact, int npad, float tol)
{
    extern __shared__ long long rfichan_d[];
    long long *d = rfichan_d;
    const int L = lags[blockIdx.x];
    for (int i = threadIdx.x; i < npad; i += 256) d[i] = i < nact ? (long long)rfichan_diff(S, i, L, nact) : LLONG_MAX;
    __syncthreads();
    // bitonic sort, ascending: every pair (i, i ^ j) with i the lower index is one thread's, between two barriers
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < npad; i += 256) {
                const int p = i ^ j;
                if (p > i) {
                    const long long x = d[i], y = d[p];
                    if ((x > y) == ((i & k) == 0)) {
                        d[i] = y;
                        d[p] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    const long long q1 = d[(nact - 1) / 4], med = d[(nact - 1) / 2], q3 = d[(size_t)3 * (nact - 1) / 4];
    const double thr = (double)tol * ((double)(q3 - q1) / 1.349);
    uint8_t *row = tab + (size_t)blockIdx.x * nact;
    for (int a = threadIdx.x; a < nact; a += 256)
        row[a] = (double)((long long)rfichan_diff(S, a, L, nact) - med) > thr ? 1 : 0;
}

// cnt: [2][nact] recv, cast, then nflag.  phase 0: a thread per (lag, channel); phase 1: a thread per channel.
__global__ __launch_bounds__(256) void k_rfichan_vote(const uint8_t *__restrict__ tab, const int32_t *__restrict__ lags,
                                                      int32_t *__restrict__ cnt, uint8_t *__restrict__ mask, int nact,
                                                      int nlag, int phase)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (phase == 0) {
        if (i >= nlag * nact) return;
        const int l = i / nact, a = i - l * nact;
        if (tab[i]) {
            atomicAdd(&cnt[a], 1);
            atomicAdd(&cnt[nact + min(max(a - lags[l], 0), nact - 1)], 1);
        }
        return;
    }
    if (i >= nact) return;
    const int recv = cnt[i];
    bool f = false;
    for (int l = 0; l < nlag; ++l)
        f |= tab[(size_t)l * nact + i] && cnt[nact + min(max(i - lags[l], 0), nact - 1)] <= recv;
    mask[i] = f ? 1 : 0;
    if (f) atomicAdd(&cnt[2 * nact], 1);
}

__global__ __launch_bounds__(256) void k_rfichan_fill(uint8_t *__restrict__ xt, const int32_t *__restrict__ chans,
                                                      const uint8_t *__restrict__ mask, const uint8_t *__restrict__ fill,
                                                      int nsamp, size_t tpitch)
{
    const int a = blockIdx.x;
    if (!mask[a]) return;                                           // (no barrier in this kernel)
    uint8_t *row = xt + (size_t)chans[a] * tpitch;
    const uint32_t b = 0x01010101u * (uint32_t)fill[a];
    const uint32_t w[4] = {b, b, b, b};
    for (int td = 16 * threadIdx.x; td < nsamp; td += 16 * 256) stream_store16(row, td, 0, nsamp, w);
}

void search_rfichan_free(pb_search *s)
{
    search_release({s->chan.d_lags, s->chan.d_mom, s->chan.d_fill, s->chan.d_mask, s->chan.d_tab, s->chan.d_cnt}, nullptr,
                   s->chan.ev, 3);
    s->chan = {};
}

// the signed lags of a radius: +l, -l for l = 1, then max(l * 3 / 2, l + 1), while l <= radius
static std::vector<int32_t> rfichan_lags(int radius)
{
    std::vector<int32_t> lags;
    for (long long l = 1; l <= radius; l = std::max(l * 3 / 2, l + 1)) {
        lags.push_back((int32_t)l);
        lags.push_back((int32_t)-l);
    }
    return lags;
}

extern "C" int pb_search_set_rfi_chan(pb_search *s, int radius, float tol)
{
    const char *fn = "pb_search_set_rfi_chan";
    if (!(tol >= 0) || !std::isfinite(tol)) return search_fail(s, fn, "tol must be >= 0 and finite");
    if (radius < 0) return search_fail(s, fn, "radius must be in 0..nact");
    if (!s) return search_fail(s, fn, "no search handle");
    if (radius > s->nact) return search_fail(s, fn, "radius must be in 0..nact");
    if (tol > 0 && (s->max_samples > RFICHAN_MAX_SAMPLES || s->nact > RFICHAN_MAX_NACT))
        return search_fail(s, fn, "max_samples above 8388608 or more than 8192 unzapped channels");
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    search_rfichan_free(s);
    if (!(tol > 0)) return PB_OK;
    const int nact = s->nact;
    const std::vector<int32_t> lags = rfichan_lags(radius > 0 ? radius : std::max(1, nact / 10));
    const int nlag = (int)lags.size();                             // >= 2 and <= RFICHAN_MAX_LAGS (radius <= 8192)
    hipError_t e = hipMalloc((void **)&s->chan.d_lags, (size_t)nlag * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(s->chan.d_lags, lags.data(), (size_t)nlag * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->chan.d_mom, (size_t)2 * nact * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->chan.d_fill, (size_t)nact);
    if (e == hipSuccess) e = hipMalloc((void **)&s->chan.d_mask, (size_t)nact);
    if (e == hipSuccess) e = hipMalloc((void **)&s->chan.d_tab, (size_t)nlag * nact);
    if (e == hipSuccess) e = hipMalloc((void **)&s->chan.d_cnt, (size_t)(2 * nact + 1) * sizeof(int32_t));
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&s->chan.ev[i]);
    if (e != hipSuccess) {
        search_rfichan_free(s);
        s->err = std::string(fn) + ": " + hipGetErrorString(e);
        return PB_EHIP;
    }
    s->chan.radius = radius;
    s->chan.tol = tol;
    s->chan.nlag = nlag;
    s->chan.npad = 1;
    while (s->chan.npad < nact) s->chan.npad <<= 1;
    return PB_OK;
}

// the stage on the nsamp samples of d_xt, between chan.ev[0] and chan.ev[1]
int search_rfichan_launch(pb_search *s, int nsamp)
{
    const int nact = s->nact, nlag = s->chan.nlag;
    int64_t *S = s->chan.d_mom + nact;
    SCHK(s, hipEventRecord(s->chan.ev[0], s->stream));
    SCHK(s, hipMemsetAsync(s->chan.d_cnt, 0, (size_t)(2 * nact + 1) * sizeof(int32_t), s->stream));
    k_rfichan_moments<<<nact, 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->chan.d_mom, s->chan.d_fill, nact, nsamp, s->tpitch);
    k_rfichan_lag<<<nlag, 256, (size_t)s->chan.npad * sizeof(long long), s->stream>>>(S, s->chan.d_lags, s->chan.d_tab, nact,
                                                                                     s->chan.npad, s->chan.tol);
    k_rfichan_vote<<<(nlag * nact + 255) / 256, 256, 0, s->stream>>>(s->chan.d_tab, s->chan.d_lags, s->chan.d_cnt,
                                                                      s->chan.d_mask, nact, nlag, 0);
    k_rfichan_vote<<<(nact + 255) / 256, 256, 0, s->stream>>>(s->chan.d_tab, s->chan.d_lags, s->chan.d_cnt, s->chan.d_mask,
                                                               nact, nlag, 1);
    k_rfichan_fill<<<nact, 256, 0, s->stream>>>(s->d_xt, s->d_chans, s->chan.d_mask, s->chan.d_fill, nsamp, s->tpitch);
    SCHK(s, hipEventRecord(s->chan.ev[1], s->stream));
    s->chan.have = 1;
    return PB_OK;
}

// a per-channel array of the stage (a < nact) -> file channel numbering, 0 for the zapped channels
template <typename T>
static int rfichan_scatter(pb_search *s, const T *dev, const std::vector<int32_t> &chans, T *out)
{
    std::vector<T> h(chans.size());
    SCHK(s, hipMemcpy(h.data(), dev, h.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (size_t a = 0; a < chans.size(); ++a) out[chans[a]] = h[a];
    return PB_OK;
}

extern "C" int pb_search_rfi_chan_info(pb_search *s, int *nflag, uint8_t *mask, int64_t *sum, int64_t *stat, int32_t *recv,
                                       int32_t *cast, uint8_t *fill, float *ms)
{
    if (!s) return search_fail(s, "pb_search_rfi_chan_info", "no search handle");
    const size_t nchan = (size_t)s->nchan;
    if (nflag) *nflag = 0;
    if (ms) *ms = 0.f;
    if (mask) memset(mask, 0, nchan);
    if (fill) memset(fill, 0, nchan);
    if (sum) memset(sum, 0, nchan * sizeof(int64_t));
    if (stat) memset(stat, 0, nchan * sizeof(int64_t));
    if (recv) memset(recv, 0, nchan * sizeof(int32_t));
    if (cast) memset(cast, 0, nchan * sizeof(int32_t));
    if (!s->chan.ran) return PB_OK;
    const int nact = s->nact;
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    std::vector<int32_t> chans(nact);
    SCHK(s, hipMemcpy(chans.data(), s->d_chans, chans.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    int rc = PB_OK;
    if (nflag) SCHK(s, hipMemcpy(nflag, s->chan.d_cnt + 2 * nact, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (mask && !rc) rc = rfichan_scatter(s, s->chan.d_mask, chans, mask);
    if (fill && !rc) rc = rfichan_scatter(s, s->chan.d_fill, chans, fill);
    if (sum && !rc) rc = rfichan_scatter(s, s->chan.d_mom, chans, sum);
    if (stat && !rc) rc = rfichan_scatter(s, s->chan.d_mom + nact, chans, stat);
    if (recv && !rc) rc = rfichan_scatter(s, s->chan.d_cnt, chans, recv);
    if (cast && !rc) rc = rfichan_scatter(s, s->chan.d_cnt + nact, chans, cast);
    if (ms && !rc) *ms = search_ms(s->chan.ev[0], s->chan.ev[1]);
    return rc;
}
