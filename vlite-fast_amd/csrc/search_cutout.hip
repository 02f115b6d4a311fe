// Per-candidate cutouts of the block and of the dedispersed series that a run leaves on the device (definition:
// include/pb_hip.h, pb_search_set_cutouts / pb_search_cutouts): k_cutout_ft, k_cutout_dt and their host side.
#include "search_internal.h"
#include "search_dev.h"

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
// bytes come through the byte gather of search_dev.h with NDW = 4 (one 16-byte and one 4-byte load); the valid byte
// range [lo, hi) of the unit -- inside [0, nsamp) of the row and inside the span -- is computed per unit and only a unit
// that is cut by it is masked.  A unit with no valid byte loads nothing; one with a valid byte has its first byte at or
// below nsamp - 1, and may begin before the row: the guarded load.
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
                gather_load_guarded<4>(xt, (long long)chans[kk] * (long long)tpitch + (long long)(s0 & ~3), w[q]);
            }
#pragma unroll
            for (int q = 0; q < CUT_CU; ++q) {
                uint32_t a[4];
                gather_shift<4>(w[q], sh[q], a);
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
                const gather_u32x4 v = *(const gather_u32x4 *)(x + t);
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

void search_cutout_ft_launch(pb_search *s, const uint8_t *plane, int n, uint32_t *ft, uint32_t *fth)
{
    k_cutout_ft<<<dim3(s->cut.nsub, n), 256, (size_t)s->cut.nt * sizeof(uint32_t), s->stream>>>(
        plane, s->d_chans, s->d_delay, s->cut.d_req, s->cut.d_sub, ft, fth, s->nact, s->last_nsamp, s->cut.nt, s->tpitch);
}

#define CUT_MAX_NT 8192          // the bins of a frequency-time cutout live in LDS (4 bytes each)

// One call's staging buffer, in 32-bit words: ft, ft_hits [n][nsub][nt], dt, dt_hits [n][ndmrow][nt], back to back;
// the page-locked copy holds the same and then the [n][3] requests.  nf, nd: words of one ft / dt array.
struct cut_layout {
    size_t nf, nd, ft, fth, dt, dth, req, total;
};

static cut_layout cut_layout_of(const pb_search *s, size_t n)
{
    const size_t nf = n * s->cut.nsub * s->cut.nt, nd = n * s->cut.ndmrow * s->cut.nt;
    return {nf, nd, 0, nf, 2 * nf, 2 * nf + nd, 2 * (nf + nd), 2 * (nf + nd) + 3 * n};
}

int search_sub_runs(pb_search *s, int nsub, std::vector<int32_t> &run)
{
    std::vector<int32_t> chans(s->nact);
    run.assign(2 * (size_t)nsub, 0);
    SCHK(s, hipMemcpy(chans.data(), s->d_chans, chans.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int per = s->nchan / nsub;
    int k = 0;
    for (int b = 0; b < nsub; ++b) {
        run[2 * b] = k;
        while (k < s->nact && chans[k] < (b + 1) * per) ++k;
        run[2 * b + 1] = k;
    }
    return PB_OK;
}

void search_cutouts_free(pb_search *s)
{
    search_release({s->cut.d_req, s->cut.d_sub, s->cut.d_out}, s->cut.h_out, s->cut.ev, 3);
    s->cut = {};
}

extern "C" int pb_search_set_cutouts(pb_search *s, int nsub, int nt, int ndmrow, int max_cands)
{
    const char *fn = "pb_search_set_cutouts";
    if (!s) return search_fail(s, fn, "no search handle");
    if (max_cands < 0) return search_fail(s, fn, "max_cands must be >= 0");
    if (max_cands > 0) {
        if (nsub < 1 || s->nchan % nsub) return search_fail(s, fn, "nsub must divide the number of channels");
        if (nt < 2 || (nt & 1) || ndmrow < 2 || (ndmrow & 1)) return search_fail(s, fn, "nt and ndmrow must be positive and even");
        if ((long long)nt * 64 > (long long)s->max_samples || nt > CUT_MAX_NT)
            return search_fail(s, fn, "nt * 64 must not exceed max_samples (and nt 8192)");
        if ((long long)max_cands * ((long long)nsub + ndmrow) * nt > (1ll << 28))
            return search_fail(s, fn, "max_cands cutouts of this geometry exceed 2 GiB");
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    search_cutouts_free(s);
    if (max_cands == 0) return PB_OK;
    std::vector<int32_t> run;
    if (int rc = search_sub_runs(s, nsub, run)) return rc;
    s->cut.nsub = nsub;
    s->cut.nt = nt;
    s->cut.ndmrow = ndmrow;
    const cut_layout M = cut_layout_of(s, (size_t)max_cands);
    hipError_t e = hipMalloc((void **)&s->cut.d_req, (size_t)max_cands * 3 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->cut.d_sub, run.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(s->cut.d_sub, run.data(), run.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&s->cut.d_out, M.req * sizeof(uint32_t));
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->cut.h_out, M.total * sizeof(uint32_t), hipHostMallocDefault);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&s->cut.ev[i]);
    if (e != hipSuccess) {
        search_cutouts_free(s);
        s->err = std::string("pb_search_set_cutouts: ") + hipGetErrorString(e);
        return PB_EHIP;
    }
    s->cut.max = max_cands;                 // (last: the stage is on only once everything exists)
    return PB_OK;
}

extern "C" int pb_search_cutouts(pb_search *s, const int32_t *cands3, int n, uint32_t *ft, uint32_t *ft_hits, uint32_t *dt,
                                 uint32_t *dt_hits)
{
    const char *fn = "pb_search_cutouts";
    if (int rc = search_enter(s, fn, s && s->cut.max, "cutouts are not switched on (pb_search_set_cutouts)",
                              s && s->last_nsamp, "no block searched yet"))
        return rc;
    if (!cands3 || n < 0 || n > s->cut.max) return search_fail(s, fn, "no request list, or more requests than max_cands");
    for (int i = 0; i < n; ++i) {
        const int dmi = cands3[3 * i], t = cands3[3 * i + 1], ts = cands3[3 * i + 2];
        if (dmi < 0 || dmi >= s->ndm || t < 0 || t >= s->last_tout || ts < 1 || ts > 64 || (ts & (ts - 1)))
            return search_fail(s, fn, "request " + std::to_string(i) + " out of range (DM index in [0, ndm), peak sample in "
                                      "[0, tout) of the last run, tscr a power of two in 1..64)");
    }
    if (n == 0) return PB_OK;
    const int nt = s->cut.nt, nrow = s->cut.ndmrow;
    const cut_layout L = cut_layout_of(s, (size_t)n);
    uint32_t *d = s->cut.d_out, *h = s->cut.h_out;
    int32_t *h_req = (int32_t *)(h + cut_layout_of(s, (size_t)s->cut.max).req);
    SCHK(s, hipSetDevice(s->device));
    for (int i = 0; i < 3 * n; ++i) h_req[i] = cands3[i];
    SCHK(s, hipMemcpyAsync(s->cut.d_req, h_req, (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    SCHK(s, hipEventRecord(s->cut.ev[0], s->stream));
    search_cutout_ft_launch(s, s->d_xt, n, d + L.ft, d + L.fth);
    k_cutout_dt<<<dim3(nrow, n), 256, 0, s->stream>>>(s->d_D, s->cut.d_req, d + L.dt, d + L.dth, s->ndm, s->last_tout, nt, s->tpitch);
    SCHK(s, hipEventRecord(s->cut.ev[1], s->stream));
    SCHK(s, hipMemcpyAsync(h, d, L.req * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipEventRecord(s->cut.ev[2], s->stream));
    SCHK(s, hipGetLastError());
    SCHK(s, hipEventSynchronize(s->cut.ev[2]));
    for (int i = 0; i < 2; ++i) s->cut.ms[i] = search_ms(s->cut.ev[0], s->cut.ev[i + 1]);
    if (ft) memcpy(ft, h + L.ft, L.nf * sizeof(uint32_t));
    if (ft_hits) memcpy(ft_hits, h + L.fth, L.nf * sizeof(uint32_t));
    if (dt) memcpy(dt, h + L.dt, L.nd * sizeof(uint32_t));
    if (dt_hits) memcpy(dt_hits, h + L.dth, L.nd * sizeof(uint32_t));
    return PB_OK;
}

extern "C" int pb_search_cutout_timers(const pb_search *s, float *ms2) { return search_get_ms(s, s ? s->cut.ms : nullptr, 2, ms2); }
