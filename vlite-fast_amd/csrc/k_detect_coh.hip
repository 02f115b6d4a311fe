// Coherence output (pb_config.coherence): detect / normalise / scrunch / requantise of AA, BB, CR and CI from the
// complex in-band spectra that k_coh_chan / k_coh_chan_kur store (k_channelize.hip).  AA and BB follow
//   detect_and_normalize2 / 3, tscrunch(_weights), sel_and_dig_*   (src/pb_kernels.cu:393-735)
// operation for operation, so they are the bytes of npol = 2; CR and CI are defined in include/pb_hip.h.
//
// One 192-thread workgroup = 32 channels x both pols of one stream, chunks of T rows, one barrier per step:
//   A  (wave 0, lane = (pol, channel)): the running-bandpass recurrence on x*x + y*y (over the row weight on the
//      excised stream, +inf for weight 0: the convention of k_detect2.hip) for chunk k; leaves the bandpass after
//      every row in LDS.  The chunk's spectra were requested one step earlier.
//   B  (waves 1, 2; lane = (8-row group, channel), both pols): chunk k-1 -- its spectra requested one step earlier,
//      the bandpass from LDS -- recomputes the power with the same operations, normalises, forms the cross products,
//      scrunches the 8 rows and quantises the four products.
// The spectra are read twice (A and B), the second time mostly from L2.  HBM traffic per stream: 8 B per row,
// channel and pol; outputs 1/32 of it.
#include "pb_internal.h"

struct DetectCohArgs {
    const float2 *X[2];      // per stream [A][S][2][R][4096] complex spectra
    const float *wrow;       // [A][S*R] row weights after apply_kurtosis
    float *bp;               // [A][2][2][4096]
    uint8_t *codes;          // [A][2][S][trim]
    float *ave;              // [A][2][S][ave_per_seg] or nullptr
    size_t trim, ave_per_seg;
    int S, R, nseg;
    float scale, oms, tscale;
};

#define DC_THREADS 192

namespace {

// LDS operations of this wave done, then the workgroup barrier (not __syncthreads(), whose fence would also drain
// the spectra requested for the next step)
__device__ __forceinline__ void dc_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int NBIT> __device__ __forceinline__ unsigned dc_quantise(float acc)
{
    if (NBIT == 8) {
        const float tmp = (float)((double)acc / 0.02957 + 127.5);
        return tmp <= 0 ? 0u : (tmp >= 255 ? 255u : (unsigned)(uint8_t)tmp);
    } else if (NBIT == 4) {
        const float tmp = (float)((double)acc / 0.3188 + 7.5);
        return tmp <= 0 ? 0u : (tmp >= 15 ? 15u : (unsigned)(uint8_t)tmp);
    } else {
        const double t = (double)acc;
        return t < -0.6109 ? 0u : (t < 0.3970 ? 1u : (t < 1.4050 ? 2u : 3u));
    }
}

// the power of one sample as the channeliser puts it in the npol = 2 planes: x*x + y*y, over the row weight on the
// excised stream (+inf for weight 0)
template <bool KUR> __device__ __forceinline__ float dc_power(float2 v, float w)
{
    const float xx = v.x * v.x;
    const float yy = v.y * v.y;
    const float pw = xx + yy;
    if (!KUR) return pw;
    return w == 0.f ? __builtin_inff() : pw / w;
}

}  // namespace

template <int T, bool KUR, int NBIT>
__device__ __forceinline__ void detect_coh_body(const DetectCohArgs &a, float4 (*s_u)[T / 4][64], float (*s_u0)[64])
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int cg = blockIdx.x, ant = blockIdx.z;
    constexpr int stream = KUR ? 1 : 0;
    constexpr int NG = T / PB_NSCRUNCH;
    const int R = a.R, cps = R / T, nchunk = a.nseg * cps;
    const int ntime = R / PB_NSCRUNCH;
    const float *wrow = a.wrow + (size_t)ant * a.S * R;
    const size_t pol_stride = (size_t)R * PB_NCHANOUT, seg_stride = 2 * pol_stride;
    const float2 *Xant = a.X[stream] + (size_t)ant * a.S * seg_stride;
    // chunk c -> its first row in the plane (segment c / cps, rows (c % cps) T ..)
    auto chunk_base = [&](int c) { return (size_t)(c / cps) * seg_stride + (size_t)(c % cps) * T * PB_NCHANOUT; };

    if (wave == 0) {
        // ---- A: the recurrence.  lane -> (pol, channel)
        const int pol = lane >> 5, c = cg * 32 + (lane & 31);
        const float2 *in = Xant + (size_t)pol * pol_stride + c;
        float *bpp = a.bp + (((size_t)ant * 2 + stream) * 2 + pol) * PB_NCHANOUT + c;
        float bp = *bpp;
        const float scale = a.scale, oms = a.oms;
        float2 cur[T], nxt[T];
        float wcur = 1.f, wnxt = 1.f;       // lane j < T: weight of row j of the chunk
        auto request = [&](int k, float2 (&x)[T], float &w) {
            const float2 *p = in + chunk_base(k);
#pragma unroll
            for (int j = 0; j < T; ++j) x[j] = p[(size_t)j * PB_NCHANOUT];
            if (KUR && lane < T) w = wrow[(size_t)(k / cps) * R + (k % cps) * T + lane];
        };
        if (nchunk > 0) request(0, nxt, wnxt);
        dc_barrier();
        for (int k = 0; k <= nchunk; ++k) {
            if (k < nchunk) {
#pragma unroll
                for (int j = 0; j < T; ++j) cur[j] = nxt[j];
                wcur = wnxt;
                if (k + 1 < nchunk) request(k + 1, nxt, wnxt);
                const int seg = k / cps, rb = k % cps, buf = k & 1;
                if (rb == 0 && bp == 0.f) {
                    // initialise the bandpass from this segment's mean (:406-411, :444-461)
                    const float2 *p = in + (size_t)seg * seg_stride;
                    if (!KUR) {
                        for (int t = 0; t < R; ++t) bp += dc_power<false>(p[(size_t)t * PB_NCHANOUT], 1.f);
                        bp /= (float)R;
                    } else {
                        int good = 0;
                        for (int t = 0; t < R; ++t) {
                            const float w = wrow[(size_t)seg * R + t];
                            if (w == 0.f) continue;
                            good++;
                            bp += dc_power<true>(p[(size_t)t * PB_NCHANOUT], w);
                        }
                        if (good == 0) bp = 1.f;
                        else bp /= (float)good;
                    }
                }
                s_u0[buf][lane] = bp;
                float u[T];
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    const float w = KUR ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wcur), j)) : 1.f;
                    const float p = dc_power<KUR>(cur[j], w);
                    const float t2 = oms * bp;
                    const float t1 = scale * p;
                    const float bpn = t1 + t2;
                    if (KUR) {
                        const float lim = bp * 11.f;
                        bp = p > lim ? bp : bpn;       // :490-491
                    } else {
                        bp = bpn;                       // :419
                    }
                    u[j] = bp;
                }
#pragma unroll
                for (int q = 0; q < T / 4; ++q) s_u[buf][q][lane] = make_float4(u[4 * q], u[4 * q + 1], u[4 * q + 2], u[4 * q + 3]);
            }
            dc_barrier();
        }
        *bpp = bp;
    } else {
        // ---- B.  lane task -> (8-row group g, channel ch), both pols; tasks beyond the chunk's groups repeat the
        // last group and store nothing, so that the whole wave takes part in the quantiser's lane shuffles
        const int idx = (wave - 1) * 64 + lane;
        const int gt = idx >> 5, ch = idx & 31;
        const bool active = gt < NG;
        const int g = active ? gt : NG - 1;
        const int c = cg * 32 + ch;
        uint8_t *codes = a.codes + ((size_t)ant * 2 + stream) * a.S * a.trim;
        float *ave = a.ave ? a.ave + ((size_t)ant * 2 + stream) * a.S * a.ave_per_seg : nullptr;
        const float2 *in = Xant + (size_t)g * PB_NSCRUNCH * PB_NCHANOUT + c;
        float2 cur[2][8], nxt[2][8];
        auto request = [&](int k) {
            const float2 *p = in + chunk_base(k);
#pragma unroll
            for (int pol = 0; pol < 2; ++pol)
#pragma unroll
                for (int j = 0; j < 8; ++j) nxt[pol][j] = p[(size_t)pol * pol_stride + (size_t)j * PB_NCHANOUT];
        };
        if (nchunk > 0) request(0);
        dc_barrier();
        for (int k = 0; k <= nchunk; ++k) {
            if (k >= 1) {
                // chunk k - 1: its bandpass was left by A in the previous step
                const int c1 = k - 1, buf = c1 & 1;
                const int seg = c1 / cps, rb = c1 % cps;
#pragma unroll
                for (int pol = 0; pol < 2; ++pol)
#pragma unroll
                    for (int j = 0; j < 8; ++j) cur[pol][j] = nxt[pol][j];
                if (k < nchunk) request(k);
                float un[2][8], ub[2][8];
#pragma unroll
                for (int pol = 0; pol < 2; ++pol) {
                    const float4 u0 = s_u[buf][2 * g][pol * 32 + ch], u1 = s_u[buf][2 * g + 1][pol * 32 + ch];
                    un[pol][0] = u0.x; un[pol][1] = u0.y; un[pol][2] = u0.z; un[pol][3] = u0.w;
                    un[pol][4] = u1.x; un[pol][5] = u1.y; un[pol][6] = u1.z; un[pol][7] = u1.w;
                    ub[pol][0] = g == 0 ? s_u0[buf][pol * 32 + ch] : s_u[buf][2 * g - 1][pol * 32 + ch].w;
#pragma unroll
                    for (int j = 1; j < 8; ++j) ub[pol][j] = un[pol][j - 1];
                }
                const size_t wbase = (size_t)seg * R + (size_t)rb * T + g * PB_NSCRUNCH;
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
                float wt_sumf = 0.f;
                int wt_sum = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float w = KUR ? wrow[wbase + j] : 1.f;
                    float v[2];
                    bool clip[2];
#pragma unroll
                    for (int pol = 0; pol < 2; ++pol) {
                        const float p = dc_power<KUR>(cur[pol][j], w);
                        float x = p / un[pol][j] - 1.f;
                        clip[pol] = false;
                        if (KUR) {
                            clip[pol] = p > ub[pol][j] * 11.f;
                            x = clip[pol] ? 10.f : x;
                            x = w == 0.f ? 0.f : x;
                        }
                        v[pol] = x;
                    }
                    // cross products (include/pb_hip.h)
                    const float ax = cur[0][j].x, ay = cur[0][j].y, bx = cur[1][j].x, by = cur[1][j].y;
                    const float rxx = ax * bx, ryy = ay * by;
                    const float re = rxx + ryy;
                    const float iyx = ay * bx, ixy = ax * by;
                    const float im = iyx - ixy;
                    float n;
                    if (KUR) {
                        const float na = un[0][j] * w, nb = un[1][j] * w;
                        n = na * nb;
                    } else {
                        n = un[0][j] * un[1][j];
                    }
                    const float d = sqrtf(n);
                    const float qr = re / d, qi = im / d;
                    float cr = qr * 1.41421356f, ci = qi * 1.41421356f;
                    if (KUR) {
                        const bool zero = w == 0.f || clip[0] || clip[1];
                        cr = zero ? 0.f : cr;
                        ci = zero ? 0.f : ci;
                    }
                    if (!KUR) {
                        acc[0] += v[0];
                        acc[1] += v[1];
                        acc[2] += cr;
                        acc[3] += ci;
                    } else if (!(w < 0.2f)) {
                        // (double)w >= 0.2 <=> w >= 0.2f; both pols share the row weight, and
                        // (float)(0.5 * (wA + wB)) of two equal weights is that weight
                        const float wx = (float)(0.5 * (double)(w + w));
                        wt_sum++;
                        wt_sumf += w;
                        const float p0 = w * v[0], p1 = w * v[1], p2 = wx * cr, p3 = wx * ci;
                        acc[0] = p0 + acc[0];
                        acc[1] = p1 + acc[1];
                        acc[2] = p2 + acc[2];
                        acc[3] = p3 + acc[3];
                    }
                }
                if (!KUR) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] *= a.tscale;
                } else {
                    const bool ok = (wt_sumf / PB_NSCRUNCH) >= 0.2f;
                    const float dd = sqrtf((float)wt_sum);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float q = acc[i] / dd;
                        acc[i] = ok ? q : 0.f;
                    }
                }
                const int trow = rb * NG + g;
                uint8_t *cseg = codes + (size_t)seg * a.trim;
                float *aseg = ave ? ave + (size_t)seg * a.ave_per_seg : nullptr;
#pragma unroll
                for (int pr = 0; pr < 4; ++pr) {
                    const size_t n = ((size_t)trow * 4 + pr) * PB_NCHANOUT + c;
                    if (aseg && active) aseg[((size_t)pr * ntime + trow) * PB_NCHANOUT + c] = acc[pr];
                    const unsigned q = dc_quantise<NBIT>(acc[pr]);
                    if (NBIT == 8) {
                        if (active) cseg[n] = (uint8_t)q;
                    } else if (NBIT == 4) {
                        const unsigned hi = __shfl_down(q, 1);
                        if (active && !(lane & 1)) cseg[n >> 1] = (uint8_t)(q | (hi << 4));
                    } else {
                        const unsigned q1 = __shfl_down(q, 1);
                        const unsigned q2 = __shfl_down(q, 2);
                        const unsigned q3 = __shfl_down(q, 3);
                        if (active && !(lane & 3)) cseg[n >> 2] = (uint8_t)(q | (q1 << 2) | (q2 << 4) | (q3 << 6));
                    }
                }
            }
            dc_barrier();
        }
    }
}

// MODE = rfi_mode: 0 raw stream only, 1 excised only, 2 both (blockIdx.y picks the stream)
template <int T, int NBIT, int MODE>
__global__ __launch_bounds__(DC_THREADS) void k_detect_coh(DetectCohArgs a)
{
    __shared__ __attribute__((aligned(16))) float4 s_u[2][T / 4][64];   // bp after each row, four rows to an entry
    __shared__ float s_u0[2][64];                                        // bp before the chunk
    if (MODE == 0 || (MODE == 2 && blockIdx.y == 0)) detect_coh_body<T, false, NBIT>(a, s_u, s_u0);
    else detect_coh_body<T, true, NBIT>(a, s_u, s_u0);
}

template <int T, int NBIT>
static void launch_coh_mode(const DetectCohArgs &a, int mode, dim3 grid, hipStream_t st)
{
    if (mode == 0) k_detect_coh<T, NBIT, 0><<<grid, DC_THREADS, 0, st>>>(a);
    else if (mode == 1) k_detect_coh<T, NBIT, 1><<<grid, DC_THREADS, 0, st>>>(a);
    else k_detect_coh<T, NBIT, 2><<<grid, DC_THREADS, 0, st>>>(a);
}

template <int T>
static void launch_coh_all(const DetectCohArgs &a, int mode, int nbit, dim3 grid, hipStream_t st)
{
    if (nbit == 8) launch_coh_mode<T, 8>(a, mode, grid, st);
    else if (nbit == 4) launch_coh_mode<T, 4>(a, mode, grid, st);
    else launch_coh_mode<T, 2>(a, mode, grid, st);
}

hipError_t launch_detect_coh(pb_handle *h, int nseg)
{
    const pb_handle::BufSet &b = h->set();
    DetectCohArgs a;
    a.X[0] = (const float2 *)b.d_Praw.p;
    a.X[1] = (const float2 *)b.d_Pkur.p;
    a.wrow = b.d_wrow.p;
    a.bp = h->d_bp.p;
    a.codes = b.d_codes.p;
    a.ave = h->cfg.keep_ave ? b.d_ave.p : nullptr;
    a.trim = h->trim;
    a.ave_per_seg = h->ave_per_seg;
    a.S = h->S;
    a.R = h->R;
    a.nseg = nseg;
    const double tsamp = (double)PB_NFFT / 128000000 * PB_NSCRUNCH;  // src/process_baseband.cu:739-741
    a.scale = (float)(tsamp / 1.0);
    a.oms = 1 - a.scale;
    a.tscale = (float)sqrt(1. / PB_NSCRUNCH);
    dim3 grid(PB_NCHANOUT / 32, h->cfg.rfi_mode == 2 ? 2 : 1, h->A);
    if (h->R % 32 == 0) launch_coh_all<32>(a, h->cfg.rfi_mode, h->cfg.nbit, grid, h->stream);
    else launch_coh_all<8>(a, h->cfg.rfi_mode, h->cfg.nbit, grid, h->stream);
    return hipGetLastError();
}
