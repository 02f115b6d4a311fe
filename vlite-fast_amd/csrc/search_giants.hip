// The S/N planes that a run leaves on the device turned into giants and clusters of giants, one candidate per cluster
// (definition: include/pb_hip.h, pb_search_set_giants / pb_search_giants): k_giant_count, k_giant_scan, k_giant_write,
// then k_giant_hook / k_giant_jump until no label changes, k_giant_reduce, k_giant_cands, and their host side.
#include "search_internal.h"
#include "search_dev.h"

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
    int run = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < n ? cnt[i] : 0;
        const int inc = wave_inclusive_sum(v);
        int woff;
        const int tot = block_wave_offsets(inc, wsum, woff);
        if (i < n) off[i] = run + woff + inc - v;
        run += tot;
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
    int rank;
    const int roots = block_count(live && lab[live ? a : 0] == a, nroot, rank);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = roots;
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
    const int a = blockIdx.x * 256 + threadIdx.x;
    const bool root = a < G && lab[a < G ? a : 0] == a;
    int rank;
    block_count(root, nroot, rank);
    if (!root) return;
    const int idx = tile_off[blockIdx.x] + rank;
    if (idx >= cap) return;
    const int w = (int)(0xffffffffu - (uint32_t)best[a]);                // (a root is a member of its own cluster: best[a] is set)
    if (w < 0 || w >= G) return;
    const int32_t *g = giants + (size_t)w * GI_W;
    const int32_t *c = acc + 4 * (size_t)a;
    int4 *o = (int4 *)(cands + (size_t)idx * GI_W);
    o[0] = make_int4(g[5], g[4], g[6], g[0]);
    o[1] = make_int4(c[0], c[1], 0x7fffffff - c[2], c[3]);
}

#define GI_MAX_GIANTS (1 << 22)

void search_giants_free(pb_search *s)
{
    search_release({s->gi.d_cnt, s->gi.d_row, s->gi.d_giants, s->gi.d_lab, s->gi.d_best, s->gi.d_acc, s->gi.d_tile, s->gi.d_out},
                   s->gi.h_out, s->gi.ev, 4);
    s->gi = {};
}

extern "C" int pb_search_set_giants(pb_search *s, int sep_time, int sep_dm, int sep_filter, int max_giants)
{
    const char *fn = "pb_search_set_giants";
    if (!s) return search_fail(s, fn, "no search handle");
    if (max_giants < 0 || max_giants > GI_MAX_GIANTS) return search_fail(s, fn, "max_giants must be in 0..4194304");
    if (max_giants > 0) {
        if (sep_time < 1 || sep_time > 64)
            return search_fail(s, fn, "sep_time must be in 1..64 (a chunk of 64 samples looks one chunk back)");
        if (sep_dm < 0 || sep_filter < 0) return search_fail(s, fn, "sep_dm and sep_filter must be >= 0");
        if ((long long)s->ndm * (long long)s->max_samples >= (1ll << 31))
            return search_fail(s, fn, "ndm x max_samples must stay below 2^31 (32-bit counts)");
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    search_giants_free(s);
    if (max_giants == 0) return PB_OK;
    const size_t cap = (size_t)max_giants, ntile = (cap + 255) / 256;
    hipError_t e = hipMalloc((void **)&s->gi.d_cnt, (size_t)s->ndm * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->gi.d_row, ((size_t)s->ndm + 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->gi.d_giants, cap * GI_W * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->gi.d_lab, cap * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->gi.d_best, cap * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&s->gi.d_acc, cap * 4 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->gi.d_tile, (2 * ntile + 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->gi.d_out, (16 + cap * GI_W) * sizeof(int32_t));
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->gi.h_out, (16 + cap * GI_W) * sizeof(int32_t), hipHostMallocDefault);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&s->gi.ev[i]);
    if (e != hipSuccess) {
        search_giants_free(s);
        s->err = std::string("pb_search_set_giants: ") + hipGetErrorString(e);
        return PB_EHIP;
    }
    s->gi.sep_time = sep_time;
    s->gi.sep_dm = sep_dm;
    s->gi.sep_filter = sep_filter;
    s->gi.max = max_giants;
    return PB_OK;
}

extern "C" int pb_search_set_planes(pb_search *s, const float *snr, const uint8_t *width_log2, int tout)
{
    if (!s) return search_fail(s, "pb_search_set_planes", "no search handle");
    if (!snr || !width_log2 || tout < 1 || tout > s->max_samples)
        return search_fail(s, "pb_search_set_planes", "no planes, or tout outside 1..max_samples");
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    SCHK(s, hipMemcpy2D(s->d_snr, s->tpitch * sizeof(float), snr, (size_t)tout * sizeof(float), (size_t)tout * sizeof(float),
                        s->ndm, hipMemcpyHostToDevice));
    SCHK(s, hipMemcpy2D(s->d_wid, s->tpitch, width_log2, (size_t)tout, (size_t)tout, s->ndm, hipMemcpyHostToDevice));
    s->plane_tout = tout;
    return PB_OK;
}

extern "C" int pb_search_giants(pb_search *s, float thresh, int t_lo, int t_hi, int32_t *cands, int max_out, int *ncands,
                                int *ngiants, int *overflow)
{
    if (int rc = search_enter(s, "pb_search_giants", s && s->gi.max, "the stage is not switched on (pb_search_set_giants)",
                              s && s->plane_tout, "no block searched and no planes set yet"))
        return rc;
    if (t_lo < 0 || t_lo >= t_hi || t_hi > s->plane_tout)
        return search_fail(s, "pb_search_giants", "the sample range must satisfy 0 <= t_lo < t_hi <= tout of the planes");
    if (thresh != thresh || max_out < 0 || (max_out > 0 && !cands) || !ncands || !ngiants || !overflow)
        return search_fail(s, "pb_search_giants", "NaN threshold, or an output is missing");
    const int cap = s->gi.max, ndm = s->ndm, sep = s->gi.sep_time;
    int32_t *ctl = s->gi.d_out, *d_cands = s->gi.d_out + 16;
    s->gi.last = 0;
    s->gi.sweeps = 0;
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipMemsetAsync(s->gi.d_cnt, 0, (size_t)ndm * sizeof(int32_t), s->stream));
    SCHK(s, hipMemsetAsync(ctl, 0, 16 * sizeof(int32_t), s->stream));
    SCHK(s, hipEventRecord(s->gi.ev[0], s->stream));
    const int nchunk = ((t_hi + 63) >> 6) - (t_lo >> 6);
    k_giant_count<<<dim3((nchunk + 4 * GI_SEG - 1) / (4 * GI_SEG), ndm), 256, 0, s->stream>>>(s->d_snr, s->gi.d_cnt, t_lo, t_hi,
                                                                                               thresh, sep, s->tpitch);
    k_giant_scan<<<1, 256, 0, s->stream>>>(s->gi.d_cnt, s->gi.d_row, ndm, ctl, ctl + 1, cap);
    // G decides every grid that follows: the one word the host waits for before the end
    SCHK(s, hipMemcpyAsync(s->gi.h_out, ctl, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipStreamSynchronize(s->stream));
    const int G = s->gi.h_out[0], over = s->gi.h_out[1];
    const bool work = !over && G > 0;
    if (work)
        k_giant_write<<<(ndm + 3) / 4, 256, 0, s->stream>>>(s->d_snr, s->d_wid, s->gi.d_row, ctl, s->gi.d_giants, s->gi.d_lab, ndm, t_lo,
                                                            t_hi, thresh, sep, cap, s->tpitch);
    SCHK(s, hipEventRecord(s->gi.ev[1], s->stream));
    if (work) {
        // every sweep that changes a label takes a root away, so G + 1 sweeps are the most there can be
        for (int sweep = 0;; ++sweep) {
            if (sweep > G + 1) {
                s->err = "pb_search_giants: the labelling did not settle";
                return PB_ESTATE;
            }
            SCHK(s, hipMemsetAsync(ctl + 3, 0, sizeof(int32_t), s->stream));
            k_giant_hook<<<(G + 3) / 4, 256, 0, s->stream>>>(s->gi.d_giants, s->gi.d_row, s->gi.d_lab, ctl, G, sep, s->gi.sep_dm,
                                                             s->gi.sep_filter);
            k_giant_jump<<<(G + 255) / 256, 256, 0, s->stream>>>(s->gi.d_lab, G);
            SCHK(s, hipMemcpyAsync(s->gi.h_out + 3, ctl + 3, sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
            SCHK(s, hipStreamSynchronize(s->stream));
            s->gi.sweeps = sweep + 1;
            if (!s->gi.h_out[3]) break;
        }
        const int ntile = (G + 255) / 256;
        int32_t *tile_cnt = s->gi.d_tile, *tile_off = s->gi.d_tile + (cap + 255) / 256;
        SCHK(s, hipMemsetAsync(s->gi.d_best, 0, (size_t)G * sizeof(unsigned long long), s->stream));
        SCHK(s, hipMemsetAsync(s->gi.d_acc, 0, (size_t)G * 4 * sizeof(int32_t), s->stream));
        k_giant_reduce<<<ntile, 256, 0, s->stream>>>(s->gi.d_giants, s->gi.d_lab, s->gi.d_best, s->gi.d_acc, tile_cnt, G);
        k_giant_scan<<<1, 256, 0, s->stream>>>(tile_cnt, tile_off, ntile, ctl + 2, nullptr, 0);
        k_giant_cands<<<ntile, 256, 0, s->stream>>>(s->gi.d_giants, s->gi.d_lab, s->gi.d_best, s->gi.d_acc, tile_off, d_cands, G, cap);
    }
    SCHK(s, hipEventRecord(s->gi.ev[2], s->stream));
    // one copy: the control words and the candidate table (a cluster holds a giant or more, so G rows are enough)
    const int nrow = work ? std::min(G, max_out) : 0;
    SCHK(s, hipMemcpyAsync(s->gi.h_out, s->gi.d_out, (16 + (size_t)nrow * GI_W) * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipEventRecord(s->gi.ev[3], s->stream));
    SCHK(s, hipGetLastError());
    SCHK(s, hipEventSynchronize(s->gi.ev[3]));
    for (int i = 0; i < 3; ++i) s->gi.ms[i] = search_ms(s->gi.ev[i == 2 ? 0 : i], s->gi.ev[i == 2 ? 3 : i + 1]);
    const int nc = work ? s->gi.h_out[2] : 0;
    if (nc > 0 && max_out > 0) memcpy(cands, s->gi.h_out + 16, (size_t)std::min(nc, max_out) * GI_W * sizeof(int32_t));
    s->gi.last = work ? G : 0;
    *ncands = nc;
    *ngiants = G;
    *overflow = over;
    return PB_OK;
}

extern "C" int pb_search_giant_list(pb_search *s, int32_t *out, int max_out, int *n)
{
    if (!s) return search_fail(s, "pb_search_giant_list", "no search handle");
    if (s->gi.max == 0 || !n || max_out < 0 || (max_out > 0 && !out))
        return search_fail(s, "pb_search_giant_list", "the stage is not switched on, or an output is missing");
    const int k = std::min(s->gi.last, max_out);
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    if (k > 0) SCHK(s, hipMemcpy(out, s->gi.d_giants, (size_t)k * GI_W * sizeof(int32_t), hipMemcpyDeviceToHost));
    *n = s->gi.last;
    return PB_OK;
}

extern "C" int pb_search_giant_timers(const pb_search *s, float *ms3, int *nsweeps)
{
    const int rc = search_get_ms(s, s ? s->gi.ms : nullptr, 3, ms3);
    if (rc == PB_OK && nsweeps) *nsweeps = s->gi.sweeps;
    return rc;
}
