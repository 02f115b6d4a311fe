// Polarisation of a candidate (definition: include/pb_hip.h, pb_search_set_pol / pb_search_pol): the search reads the
// four-product filterbank [nsamp][4][nchan] (AA, BB, CR, CI), searches the rounded mean of AA and BB exactly as it
// searches a 1-IF block, and keeps the four products channel-major on the device beside the search plane.  From them, for
// the candidates of the block: the four frequency-time images (k_cutout_ft of search_cutout.hip, once per plane), the
// on- and off-pulse spectra, and an RM synthesis over a grid of trial rotation measures.
//
//   k_transpose_pol<WIDE>  per block: a workgroup takes 64 samples x 64 channels of all four products -- dword loads along
//                          the channel axis (WIDE: source address and nchan multiples of 4; else single bytes) into LDS as
//                          [sample][product][channel], then per (channel, 16 samples) sixteen LDS bytes of each product
//                          make one 16-byte store along time into each of the five planes.
//   k_pol_spectra          grid (16 unzapped channels, request), four channels per wave, one after another: the on
//                          window and the two off windows of the four planes in 16-byte units through the byte gather
//                          of search_dev.h, exact i32 sums.
//   k_pol_stokes           a workgroup per request: q, u and lambda^2 of every unzapped channel in double, the weights;
//                          lane 0 adds W, lambda0^2 and the means of i and v in ascending channel order (from LDS).
//   k_pol_rm               grid (128 trials, request): a lane takes one trial RM and walks the channels in ascending
//                          order, q, u and lambda^2 - lambda0^2 staged in LDS 256 channels at a time.
//   k_pol_best             a workgroup per request: the first trial with the largest |F|^2.
//
// What a lane may touch.  k_transpose_pol loads codes[(t * 4 + k) * nchan + c ..] with t < nsamp and c (+ 4) <= nchan only,
// and stores samples [0, nsamp) of rows c < nchan (stream_store16).  k_pol_spectra clips every window to [0, nsamp) of the
// row BEFORE it is cut into units: a unit's first byte s0 satisfies 0 <= s0 <= nsamp - 1, which is what the gather's
// statement of reads asks for (search_dev.h); the planes are allocated like d_xt, pitch tpitch and 64 bytes of pad, and a
// byte at or beyond the window's end is masked before it is summed.
#include "search_internal.h"
#include "search_dev.h"

#define POL_TP 69               // LDS pitch of a tile's sample in dwords: 4 products x 17, + 1 (16 samples = 16 banks on)
#define POL_KP 17               // and of a product within it (64 channels + a pad dword)
#define POL_CT 16               // k_pol_spectra: unzapped channels of a workgroup, four per wave
#define POL_RT 128              // k_pol_rm: trials of a workgroup
#define POL_CH 256              // k_pol_rm, k_pol_stokes: channels staged in LDS at a time
#define POL_SQRT2 1.4142135623730951

// codes: [nsamp][4][nchan] u8 -> xa, xb, xcr, xci [c][t] and xt[c][t] = (aa + bb + 1) >> 1
template <bool WIDE>
__global__ __launch_bounds__(256) void k_transpose_pol(const uint8_t *__restrict__ codes, uint8_t *__restrict__ xa,
                                                       uint8_t *__restrict__ xb, uint8_t *__restrict__ xcr,
                                                       uint8_t *__restrict__ xci, uint8_t *__restrict__ xt, int nsamp,
                                                       int nchan, size_t tpitch)
{
    __shared__ uint32_t tile[64 * POL_TP];
    const int t0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const size_t rowb = 4 * (size_t)nchan;
    if (WIDE) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = j * 256 + threadIdx.x;
            const int dw = i & 15, k = (i >> 4) & 3, tt = i >> 6;       // 16 lanes read the 64 channels of one product
            const int t = t0 + tt, c = c0 + 4 * dw;
            uint32_t v = 0u;
            if (t < nsamp && c + 4 <= nchan) v = *(const uint32_t *)(codes + (size_t)t * rowb + (size_t)k * nchan + c);
            tile[tt * POL_TP + k * POL_KP + dw] = v;
        }
    } else {
        uint8_t *tb = (uint8_t *)tile;
        for (int i = threadIdx.x; i < 64 * 4 * 64; i += 256) {
            const int cc = i & 63, k = (i >> 6) & 3, tt = i >> 8;
            const int t = t0 + tt, c = c0 + cc;
            uint8_t v = 0;
            if (t < nsamp && c < nchan) v = codes[(size_t)t * rowb + (size_t)k * nchan + c];
            tb[4 * (tt * POL_TP + k * POL_KP) + cc] = v;
        }
    }
    __syncthreads();
    const int cc = threadIdx.x >> 2, g = threadIdx.x & 3;               // four neighbouring lanes write one 64-byte line
    const int c = c0 + cc;
    if (c >= nchan) return;                                             // (no barrier below)
    const uint8_t *tb = (const uint8_t *)tile;
    uint32_t w[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            w[k][q] = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) w[k][q] |= (uint32_t)tb[4 * ((16 * g + 4 * q + b) * POL_TP + k * POL_KP) + cc] << (8 * b);
        }
    }
    uint32_t m[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)         // per byte (a + b + 1) >> 1 = (a | b) - ((a ^ b) >> 1): no carry leaves a byte
        m[q] = (w[0][q] | w[1][q]) - (((w[0][q] ^ w[1][q]) >> 1) & 0x7f7f7f7fu);
    const size_t ro = (size_t)c * tpitch;
    const int td = t0 + 16 * g;
    stream_store16(xa + ro, td, 0, nsamp, w[0]);
    stream_store16(xb + ro, td, 0, nsamp, w[1]);
    stream_store16(xcr + ro, td, 0, nsamp, w[2]);
    stream_store16(xci + ro, td, 0, nsamp, w[3]);
    stream_store16(xt + ro, td, 0, nsamp, m);
}

// the bytes [lo, hi) (0 <= lo < hi <= nsamp) of one row of each of the four planes, a wave's lanes over its 16-byte units
__device__ __forceinline__ void pol_window(const uint8_t *const (&pl)[4], size_t ro, int lo, int hi, uint32_t (&acc)[4])
{
    for (int s0 = lo + 16 * (int)(threadIdx.x & 63); s0 < hi; s0 += 16 * 64) {
        const int h = min(16, hi - s0);
        const unsigned sh = (unsigned)(s0 & 3);
        uint32_t wd[4][5];
#pragma unroll
        for (int k = 0; k < 4; ++k) gather_load<4>((const uint32_t *)(pl[k] + ro + (size_t)(s0 & ~3)), wd[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t a[4];
            gather_shift<4>(wd[k], sh, a);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int hj = min(max(h - 4 * i, 0), 4);
                const uint32_t mk = hj == 4 ? 0xffffffffu : (1u << (8 * hj)) - 1u;
                acc[k] = __builtin_amdgcn_sad_u8(a[i] & mk, 0u, acc[k]);
            }
        }
    }
}

// req: [n][3] = DM index, peak sample, on-window length (checked on the host); on, off: [n][4][nchan]; non, noff:
// [n][nchan] (zeroed before the launch: the rows of zapped channels stay 0)
__global__ __launch_bounds__(256) void k_pol_spectra(const uint8_t *__restrict__ xa, const uint8_t *__restrict__ xb,
                                                     const uint8_t *__restrict__ xcr, const uint8_t *__restrict__ xci,
                                                     const int32_t *__restrict__ chans, const int32_t *__restrict__ delay,
                                                     const int32_t *__restrict__ req, int32_t *__restrict__ on,
                                                     int32_t *__restrict__ non, int32_t *__restrict__ off,
                                                     int32_t *__restrict__ noff, int nact, int nchan, int nsamp, int L,
                                                     int guard, size_t tpitch)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, cand = blockIdx.y;
    const int dmi = req[3 * cand], tpk = req[3 * cand + 1], w = req[3 * cand + 2];
    const int32_t *dl = delay + (size_t)dmi * nact;
    const uint8_t *const pl[4] = {xa, xb, xcr, xci};
    for (int i = 0; i < POL_CT / 4; ++i) {
        const int kk = blockIdx.x * POL_CT + wave * (POL_CT / 4) + i;   // the same in every lane of the wave
        if (kk >= nact) break;
        const int d = dl[kk], c = chans[kk];
        const size_t ro = (size_t)c * tpitch;
        uint32_t a_on[4] = {0u, 0u, 0u, 0u}, a_off[4] = {0u, 0u, 0u, 0u};
        int n_on = 0, n_off = 0;
        {
            const int lo = max(tpk + d, 0), hi = min(tpk + w + d, nsamp);
            if (hi > lo) {
                n_on = hi - lo;
                pol_window(pl, ro, lo, hi, a_on);
            }
        }
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int a = side ? tpk + w + guard : tpk - guard - L;
            const int lo = max(a + d, 0), hi = min(a + L + d, nsamp);
            if (hi > lo) {
                n_off += hi - lo;
                pol_window(pl, ro, lo, hi, a_off);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            for (int o = 32; o >= 1; o >>= 1) {
                a_on[k] += __shfl_down(a_on[k], o);
                a_off[k] += __shfl_down(a_off[k], o);
            }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                on[((size_t)cand * 4 + k) * nchan + c] = (int32_t)a_on[k];
                off[((size_t)cand * 4 + k) * nchan + c] = (int32_t)a_off[k];
            }
            non[(size_t)cand * nchan + c] = n_on;
            noff[(size_t)cand * nchan + c] = n_off;
        }
    }
}

// st: [n][3][nact] = q, u, lambda^2 - lambda0^2 (q = u = 0 where the weight is 0: such a channel adds an exact 0 to F);
// summary: [n][6], entries 0..3 = W, lambda0^2, mean i, mean v (NaN for W = 0)
__global__ __launch_bounds__(256) void k_pol_stokes(const int32_t *__restrict__ chans, const int32_t *__restrict__ on,
                                                    const int32_t *__restrict__ non, const int32_t *__restrict__ off,
                                                    const int32_t *__restrict__ noff, double *__restrict__ st,
                                                    double *__restrict__ summary, int nact, int nchan, double fch1,
                                                    double foff)
{
    __shared__ double sh[4][POL_CH];
    __shared__ double sh_l0;
    const int cand = blockIdx.x;
    double *sq = st + (size_t)cand * 3 * nact, *su = sq + nact, *sl = su + nact;
    double W = 0, SL = 0, SI = 0, SV = 0;                               // lane 0's running sums, ascending channel order
    for (int base = 0; base < nact; base += POL_CH) {
        const int kk = base + threadIdx.x;
        double wgt = 0, l2 = 0, iv = 0, vv = 0;
        if (kk < nact) {
            const int c = chans[kk];
            const double f = fch1 + (double)c * foff;
            const double r = 299.792458 / f;
            l2 = r * r;
            const int no = non[(size_t)cand * nchan + c], nf = noff[(size_t)cand * nchan + c];
            double q = 0, u = 0;
            if (no > 0 && nf > 0) {
                double m[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double a = (double)on[((size_t)cand * 4 + k) * nchan + c] / (double)no;
                    const double b = (double)off[((size_t)cand * 4 + k) * nchan + c] / (double)nf;
                    m[k] = a - b;
                }
                wgt = 1;
                iv = m[0] + m[1];
                q = m[0] - m[1];
                u = POL_SQRT2 * m[2];
                vv = POL_SQRT2 * m[3];
            }
            sq[kk] = q;
            su[kk] = u;
            sl[kk] = l2;
        }
        sh[0][threadIdx.x] = wgt;
        sh[1][threadIdx.x] = l2;
        sh[2][threadIdx.x] = iv;
        sh[3][threadIdx.x] = vv;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int nj = min(POL_CH, nact - base);
            for (int j = 0; j < nj; ++j) {
                if (sh[0][j] != 0) {
                    W += 1;
                    SL += sh[1][j];
                    SI += sh[2][j];
                    SV += sh[3][j];
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const double l0 = W > 0 ? SL / W : nan;
        summary[6 * cand + 0] = W;
        summary[6 * cand + 1] = l0;
        summary[6 * cand + 2] = W > 0 ? SI / W : nan;
        summary[6 * cand + 3] = W > 0 ? SV / W : nan;
        sh_l0 = l0;
    }
    __syncthreads();
    const double l0 = sh_l0;
    for (int kk = threadIdx.x; kk < nact; kk += POL_CH) sl[kk] = sl[kk] - l0;      // (each lane rewrites what it wrote)
}

// F: [n][nrm][2] = (1/W) sum over the channels, ascending, of (q + i u) exp(-2 i phi (lambda^2 - lambda0^2))
__global__ __launch_bounds__(POL_RT) void k_pol_rm(const double *__restrict__ st, const double *__restrict__ summary,
                                                   double *__restrict__ F, int nact, int nrm, double rm_lo, double rm_step)
{
    __shared__ double cq[POL_CH], cu[POL_CH], cl[POL_CH];
    const int cand = blockIdx.y, k = blockIdx.x * POL_RT + threadIdx.x;
    const double *sq = st + (size_t)cand * 3 * nact, *su = sq + nact, *sl = su + nact;
    const double phi = rm_lo + (double)k * rm_step;
    const double two_phi = 2.0 * phi;
    double re = 0, im = 0;
    for (int base = 0; base < nact; base += POL_CH) {
        const int nj = min(POL_CH, nact - base);
        for (int j = threadIdx.x; j < nj; j += POL_RT) {
            cq[j] = sq[base + j];
            cu[j] = su[base + j];
            cl[j] = sl[base + j];
        }
        __syncthreads();
        for (int j = 0; j < nj; ++j) {
            const double th = two_phi * cl[j];
            double sn, cs;
            sincos(th, &sn, &cs);
            const double q = cq[j], u = cu[j];
            re += q * cs + u * sn;
            im += u * cs - q * sn;
        }
        __syncthreads();
    }
    if (k < nrm) {
        const double W = summary[6 * cand];
        F[((size_t)cand * nrm + k) * 2] = re / W;
        F[((size_t)cand * nrm + k) * 2 + 1] = im / W;
    }
}

// kbest: [n] the first trial with the largest re^2 + im^2 (-1 for W = 0); summary entries 4, 5 = sqrt of that, its RM
__global__ __launch_bounds__(256) void k_pol_best(const double *__restrict__ F, double *__restrict__ summary,
                                                  int32_t *__restrict__ kbest, int nrm, double rm_lo, double rm_step)
{
    __shared__ unsigned long long sh[4];
    const int cand = blockIdx.x;
    const double *f = F + (size_t)cand * nrm * 2;
    // a non-negative double orders as its bit pattern; + 1 keeps 0 for "nothing" (a NaN)
    unsigned long long best = 0ull;
    for (int k = threadIdx.x; k < nrm; k += 256) {
        const double p = f[2 * k] * f[2 * k] + f[2 * k + 1] * f[2 * k + 1];
        if (p >= 0) best = max(best, (unsigned long long)__double_as_longlong(p) + 1ull);
    }
    const unsigned long long top = block_max(best, sh);
    unsigned long long first = 0ull;                                    // ~k of the smallest k that reaches it
    if (top)
        for (int k = threadIdx.x; k < nrm; k += 256) {
            const double p = f[2 * k] * f[2 * k] + f[2 * k + 1] * f[2 * k + 1];
            if (p >= 0 && (unsigned long long)__double_as_longlong(p) + 1ull == top) {
                first = ~(unsigned long long)k;
                break;
            }
        }
    first = block_max(first, sh);
    if (threadIdx.x == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const bool ok = summary[6 * cand] > 0 && top != 0ull;
        const int kb = ok ? (int)~first : -1;
        kbest[cand] = kb;
        summary[6 * cand + 4] = ok ? sqrt(__longlong_as_double((long long)(top - 1ull))) : nan;
        summary[6 * cand + 5] = ok ? rm_lo + (double)kb * rm_step : nan;
    }
}

// One call's staging buffer in bytes: F [n][nrm][2] and summary [n][6] doubles, then on, off [n][4][nchan], non, noff
// [n][nchan] and kbest [n] i32, back to back; the page-locked copy holds the same and then the [n][3] requests.
struct pol_layout {
    size_t F, summary, on, off, non, noff, kbest, req, total;
};

static pol_layout pol_layout_of(const pb_search *s, size_t n)
{
    pol_layout L;
    L.F = 0;
    L.summary = L.F + n * s->pol.nrm * 2 * sizeof(double);
    L.on = L.summary + n * 6 * sizeof(double);
    L.off = L.on + n * 4 * s->nchan * sizeof(int32_t);
    L.non = L.off + n * 4 * s->nchan * sizeof(int32_t);
    L.noff = L.non + n * s->nchan * sizeof(int32_t);
    L.kbest = L.noff + n * s->nchan * sizeof(int32_t);
    L.req = L.kbest + n * sizeof(int32_t);
    L.total = L.req + n * 3 * sizeof(int32_t);
    return L;
}

void search_pol_free(pb_search *s)
{
    search_release({s->pol.d_codes, s->pol.d_plane[0], s->pol.d_plane[1], s->pol.d_plane[2], s->pol.d_plane[3], s->pol.d_req,
                    s->pol.d_st, s->pol.d_out, s->pol.d_cut}, s->pol.h_out, s->pol.ev, 3);
    if (s->pol.h_cut) (void)hipHostFree(s->pol.h_cut);
    s->pol = {};
}

extern "C" int pb_search_set_pol(pb_search *s, int off_len, int guard, int nrm, double rm_lo, double rm_step, int max_cands)
{
    const char *fn = "pb_search_set_pol";
    if (!s) return search_fail(s, fn, "no search handle");
    if (max_cands < 0) return search_fail(s, fn, "max_cands must be >= 0");
    const size_t plane = s->tpitch * s->nchan + 64, stage = 4 * (size_t)s->max_samples * s->nchan;
    if (max_cands > 0) {
        if (off_len < 1 || off_len > 1024 || guard < 0 || guard > 1024)
            return search_fail(s, fn, "off_len must be in 1..1024 and guard in 0..1024");
        if (nrm < 1 || nrm > 8192 || !std::isfinite(rm_lo) || !std::isfinite(rm_step))
            return search_fail(s, fn, "nrm must be in 1..8192, rm_lo and rm_step finite");
        if (s->gp.keep_max > 0) return search_fail(s, fn, "streaming is switched on (pb_search_set_gulp): four-product blocks are not streamed");
        const size_t out = (size_t)max_cands * ((size_t)nrm * 16 + 48 + 10 * (size_t)s->nchan * 4 + 16) +
                           (size_t)max_cands * 3 * s->nact * sizeof(double);
        if (4 * plane + stage + out > ((size_t)1 << 31)) return search_fail(s, fn, "the planes and buffers of this geometry exceed 2 GiB");
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    search_pol_free(s);
    if (max_cands == 0) return PB_OK;
    s->pol.off_len = off_len;
    s->pol.guard = guard;
    s->pol.nrm = nrm;
    s->pol.rm_lo = rm_lo;
    s->pol.rm_step = rm_step;
    const pol_layout M = pol_layout_of(s, (size_t)max_cands);
    hipError_t e = hipMalloc((void **)&s->pol.d_codes, stage);
    for (int k = 0; k < 4 && e == hipSuccess; ++k) {
        // + 64: the pad that the byte gather may read into past the last row, as d_xt's (search_dev.h)
        e = hipMalloc((void **)&s->pol.d_plane[k], plane);
        if (e == hipSuccess) e = hipMemset(s->pol.d_plane[k], 0, plane);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&s->pol.d_req, (size_t)max_cands * 3 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->pol.d_st, (size_t)max_cands * 3 * s->nact * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&s->pol.d_out, M.req);
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->pol.h_out, M.total, hipHostMallocDefault);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&s->pol.ev[i]);
    if (e != hipSuccess) {
        search_pol_free(s);
        s->err = std::string(fn) + ": " + hipGetErrorString(e);
        return PB_EHIP;
    }
    s->pol.max = max_cands;                 // (last: the stage is on only once everything exists)
    return PB_OK;
}

int search_pol_transpose(pb_search *s, const uint8_t *codes, int nsamp)
{
    dim3 gt((nsamp + 63) / 64, (s->nchan + 63) / 64);
    uint8_t *const *p = s->pol.d_plane;
    if (((uintptr_t)codes & 3) == 0 && s->nchan % 4 == 0)
        k_transpose_pol<true><<<gt, 256, 0, s->stream>>>(codes, p[0], p[1], p[2], p[3], s->d_xt, nsamp, s->nchan, s->tpitch);
    else
        k_transpose_pol<false><<<gt, 256, 0, s->stream>>>(codes, p[0], p[1], p[2], p[3], s->d_xt, nsamp, s->nchan, s->tpitch);
    s->pol.have = 1;
    return PB_OK;
}

static const char *const POL_OFF = "polarisation is not switched on (pb_search_set_pol)";

extern "C" int pb_search_pol(pb_search *s, const int32_t *req3, int n, int32_t *on, int32_t *non, int32_t *off, int32_t *noff,
                             double *F, int32_t *kbest, double *summary)
{
    const char *fn = "pb_search_pol";
    if (int rc = search_enter(s, fn, s && s->pol.max, POL_OFF, s && s->pol.have && s->last_nsamp, "no block searched yet"))
        return rc;
    if (!req3 || n < 0 || n > s->pol.max) return search_fail(s, fn, "no request list, or more requests than max_cands");
    for (int i = 0; i < n; ++i) {
        const int dmi = req3[3 * i], t = req3[3 * i + 1], w = req3[3 * i + 2];
        if (dmi < 0 || dmi >= s->ndm || t < 0 || t >= s->last_tout || w < 1 || w > 64)
            return search_fail(s, fn, "request " + std::to_string(i) + " out of range (DM index in [0, ndm), peak sample in "
                                      "[0, tout) of the last run, w in 1..64)");
    }
    if (n == 0) return PB_OK;
    const int nrm = s->pol.nrm, nchan = s->nchan, nact = s->nact;
    const pol_layout L = pol_layout_of(s, (size_t)n);
    uint8_t *d = s->pol.d_out, *h = s->pol.h_out;
    int32_t *h_req = (int32_t *)(h + pol_layout_of(s, (size_t)s->pol.max).req);
    SCHK(s, hipSetDevice(s->device));
    for (int i = 0; i < 3 * n; ++i) h_req[i] = req3[i];
    SCHK(s, hipMemcpyAsync(s->pol.d_req, h_req, (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    SCHK(s, hipEventRecord(s->pol.ev[0], s->stream));
    SCHK(s, hipMemsetAsync(d + L.on, 0, L.kbest - L.on, s->stream));    // the rows of zapped channels are 0
    int32_t *d_on = (int32_t *)(d + L.on), *d_off = (int32_t *)(d + L.off), *d_non = (int32_t *)(d + L.non),
            *d_noff = (int32_t *)(d + L.noff);
    double *d_F = (double *)(d + L.F), *d_sum = (double *)(d + L.summary);
    uint8_t *const *p = s->pol.d_plane;
    k_pol_spectra<<<dim3((nact + POL_CT - 1) / POL_CT, n), 256, 0, s->stream>>>(
        p[0], p[1], p[2], p[3], s->d_chans, s->d_delay, s->pol.d_req, d_on, d_non, d_off, d_noff, nact, nchan, s->last_nsamp,
        s->pol.off_len, s->pol.guard, s->tpitch);
    k_pol_stokes<<<n, 256, 0, s->stream>>>(s->d_chans, d_on, d_non, d_off, d_noff, s->pol.d_st, d_sum, nact, nchan,
                                           (double)s->fch1, (double)s->foff);
    k_pol_rm<<<dim3((nrm + POL_RT - 1) / POL_RT, n), POL_RT, 0, s->stream>>>(s->pol.d_st, d_sum, d_F, nact, nrm, s->pol.rm_lo,
                                                                            s->pol.rm_step);
    k_pol_best<<<n, 256, 0, s->stream>>>(d_F, d_sum, (int32_t *)(d + L.kbest), nrm, s->pol.rm_lo, s->pol.rm_step);
    SCHK(s, hipEventRecord(s->pol.ev[1], s->stream));
    SCHK(s, hipMemcpyAsync(h, d, L.req, hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipEventRecord(s->pol.ev[2], s->stream));
    SCHK(s, hipGetLastError());
    SCHK(s, hipEventSynchronize(s->pol.ev[2]));
    for (int i = 0; i < 2; ++i) s->pol.ms[i] = search_ms(s->pol.ev[0], s->pol.ev[i + 1]);
    if (on) memcpy(on, h + L.on, L.off - L.on);
    if (off) memcpy(off, h + L.off, L.non - L.off);
    if (non) memcpy(non, h + L.non, L.noff - L.non);
    if (noff) memcpy(noff, h + L.noff, L.kbest - L.noff);
    if (F) memcpy(F, h + L.F, L.summary - L.F);
    if (summary) memcpy(summary, h + L.summary, L.on - L.summary);
    if (kbest) memcpy(kbest, h + L.kbest, L.req - L.kbest);
    return PB_OK;
}

extern "C" int pb_search_pol_cutouts(pb_search *s, const int32_t *cands3, int n, uint32_t *pft, uint32_t *pft_hits)
{
    const char *fn = "pb_search_pol_cutouts";
    if (int rc = search_enter(s, fn, s && s->pol.max && s->cut.max, "polarisation and cutouts must both be switched on "
                              "(pb_search_set_pol, pb_search_set_cutouts)", s && s->pol.have && s->last_nsamp, "no block searched yet"))
        return rc;
    const int cap = std::min(s->pol.max, s->cut.max);
    if (!cands3 || n < 0 || n > cap) return search_fail(s, fn, "no request list, or more requests than max_cands");
    for (int i = 0; i < n; ++i) {
        const int dmi = cands3[3 * i], t = cands3[3 * i + 1], ts = cands3[3 * i + 2];
        if (dmi < 0 || dmi >= s->ndm || t < 0 || t >= s->last_tout || ts < 1 || ts > 64 || (ts & (ts - 1)))
            return search_fail(s, fn, "request " + std::to_string(i) + " out of range (DM index in [0, ndm), peak sample in "
                                      "[0, tout) of the last run, tscr a power of two in 1..64)");
    }
    if (n == 0) return PB_OK;
    SCHK(s, hipSetDevice(s->device));
    const int nsub = s->cut.nsub, nt = s->cut.nt;
    const size_t one = (size_t)nsub * nt;                               // words of one image
    const int sig[4] = {nsub, nt, s->cut.max, s->pol.max};
    if (memcmp(sig, s->pol.cut_sig, sizeof sig)) {
        // either set call has changed since the buffers were made (or they never were): remake them
        SCHK(s, hipStreamSynchronize(s->stream));
        if (s->pol.d_cut) (void)hipFree(s->pol.d_cut);
        if (s->pol.h_cut) (void)hipHostFree(s->pol.h_cut);
        s->pol.d_cut = s->pol.h_cut = nullptr;
        memset(s->pol.cut_sig, 0, sizeof sig);
        SCHK(s, hipMalloc((void **)&s->pol.d_cut, (size_t)cap * 5 * one * sizeof(uint32_t)));
        SCHK(s, hipHostMalloc((void **)&s->pol.h_cut, ((size_t)cap * 5 * one + 3 * (size_t)cap) * sizeof(uint32_t), hipHostMallocDefault));
        memcpy(s->pol.cut_sig, sig, sizeof sig);
    }
    uint32_t *d = s->pol.d_cut, *h = s->pol.h_cut;
    int32_t *h_req = (int32_t *)(h + (size_t)cap * 5 * one);
    for (int i = 0; i < 3 * n; ++i) h_req[i] = cands3[i];
    SCHK(s, hipMemcpyAsync(s->cut.d_req, h_req, (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    // staging: [4][n] images, then [n] hit counts (the same for all four: the last launch's stay)
    for (int k = 0; k < 4; ++k) search_cutout_ft_launch(s, s->pol.d_plane[k], n, d + (size_t)k * n * one, d + (size_t)4 * n * one);
    SCHK(s, hipMemcpyAsync(h, d, (size_t)5 * n * one * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipGetLastError());
    SCHK(s, hipStreamSynchronize(s->stream));
    if (pft)
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 4; ++k) memcpy(pft + ((size_t)i * 4 + k) * one, h + ((size_t)k * n + i) * one, one * sizeof(uint32_t));
    if (pft_hits) memcpy(pft_hits, h + (size_t)4 * n * one, (size_t)n * one * sizeof(uint32_t));
    return PB_OK;
}

extern "C" int pb_search_pol_fetch(pb_search *s, int which, uint8_t *out, size_t nbytes)
{
    const char *fn = "pb_search_pol_fetch";
    if (int rc = search_enter(s, fn, s && s->pol.max, POL_OFF, s && s->pol.have && s->last_nsamp, "no block searched yet"))
        return rc;
    const size_t n = s->last_nsamp;
    if (which < 0 || which > 3 || !out || nbytes < n * s->nchan)
        return search_fail(s, fn, "which must be in 0..3 and the buffer hold nchan x nsamp bytes");
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    SCHK(s, hipMemcpy2D(out, n, s->pol.d_plane[which], s->tpitch, n, s->nchan, hipMemcpyDeviceToHost));
    return PB_OK;
}

extern "C" int pb_search_pol_timers(const pb_search *s, float *ms3)
{
    if (!s || !ms3) return PB_EINVAL;
    ms3[0] = s->pol.have ? s->ms[1] : 0.f;             // the transposition is the run's transpose stage
    ms3[1] = s->pol.ms[0];
    ms3[2] = s->pol.ms[1];
    return PB_OK;
}
