// Device-only helpers of the search's kernels: the packed-byte gather of the channel-major block, and the reductions and
// scans of a 256-thread workgroup (four waves of 64).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// ---- the byte gather ----
// A lane wants 4 NDW consecutive samples of one channel's row from sample s0 = t + delay on, where s0 is any byte
// offset.  It loads the NDW + 1 aligned dwords from s0 & ~3 (gather_load), shifts them into place with v_alignbyte by
// s0 & 3 (gather_align, gather_shift); k_dedisperse and k_refine_series then sum the bytes as packed 16-bit pairs, each
// in its own registers (a shared accumulator cost k_refine_series 13 VGPRs).  The two invariants every user relies on:
//
// Reads.  The last byte loaded is (s0 & ~3) + 4 NDW + 3 <= s0 + 4 NDW + 3: 11 bytes past s0 for NDW = 2, 19 for
// NDW = 4.  A lane only loads when s0 <= nsamp - 1 (each kernel says why its s0 is), so it reads below nsamp + 19.  A
// row's pitch is a multiple of 64 and at least max_samples >= nsamp: bytes past nsamp are the rest of the row's pitch,
// the start of the next row or, after the last row, the 64-byte pad that the allocation ends with (search_create) --
// all readable, and no kernel lets a byte at or beyond nsamp reach an output.  Below the row the same holds for the
// previous row, except below the very first: gather_load_guarded leaves the dwords before the allocation unloaded.
//
// 16 bits.  A channel puts one byte (<= 255) into each 16-bit half; the kernel flushes into its 32-bit sums once
// GATHER_FLUSH = 240 channels have gone in since the last flush, counting in steps of at most 8 (DDM_CU, RF_CU), and
// adds at most 7 tail channels after the last check: never more than 254 x 255 = 64770 < 2^16 (257 is the limit).
#define GATHER_FLUSH 240

typedef uint32_t gather_u32x4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes at a 4-byte aligned address

template <int NDW>
__device__ __forceinline__ void gather_load(const uint32_t *p, uint32_t (&w)[NDW + 1])
{
#pragma unroll
    for (int i = 0; i + 4 <= NDW + 1; i += 4) {
        const gather_u32x4 v = *(const gather_u32x4 *)(p + i);
        w[i] = v.x;
        w[i + 1] = v.y;
        w[i + 2] = v.z;
        w[i + 3] = v.w;
    }
#pragma unroll
    for (int i = (NDW + 1) & ~3; i <= NDW; ++i) w[i] = p[i];
}

// the same from byte offset `off` (a multiple of 4, possibly negative) of the block: a dword before the block keeps
// what w[] held (the callers' 0)
template <int NDW>
__device__ __forceinline__ void gather_load_guarded(const uint8_t *xt, long long off, uint32_t (&w)[NDW + 1])
{
    if (off >= 0) {
        gather_load<NDW>((const uint32_t *)(xt + off), w);
    } else {
#pragma unroll
        for (int i = 0; i <= NDW; ++i)
            if (off + 4 * i >= 0) w[i] = *(const uint32_t *)(xt + off + 4 * i);
    }
}

// bytes sh .. sh + 3 (sh in 0 .. 3) of the 8 bytes w1:w0
__device__ __forceinline__ uint32_t gather_align(uint32_t w0, uint32_t w1, unsigned sh) { return __builtin_amdgcn_alignbyte(w1, w0, sh); }

// a[i] = bytes sh .. sh + 3 of w[i + 1]:w[i]
template <int NDW>
__device__ __forceinline__ void gather_shift(const uint32_t (&w)[NDW + 1], unsigned sh, uint32_t (&a)[NDW])
{
#pragma unroll
    for (int i = 0; i < NDW; ++i) a[i] = gather_align(w[i], w[i + 1], sh);
}

// ---- the append of the streaming stage (search_stream.hip: codes; search_plane.hip: an fp32 plane) ----
// Both tile the DESTINATION: a tile is SA_T block samples from a multiple of SA_T on, staged in LDS as [sample][channel]
// and stored along time, sixteen samples of one channel at a time.
#define SA_T 64                 // destination samples of a tile
#define SA_B 64                 // fast path of the codes: packed source bytes of a tile's row
#define SA_PITCH 84             // fast path of the codes: LDS pitch of a tile row in bytes; 16 rows = 336 dwords = 16 banks on:
                                // the four 16-sample groups that a wave reads together fall into different banks
#define SA_BPITCH 68            // 64 unpacked channels: the same (16 rows = 272 dwords = 16 banks on)

// w = 16 samples of one channel from sample td (a multiple of 16) on; [lo, hi) = the samples that this push owns
__device__ __forceinline__ void stream_store16(uint8_t *__restrict__ row, int td, int lo, int hi, const uint32_t (&w)[4])
{
    if (td >= lo && td + 16 <= hi) {
        *(uint4 *)(row + td) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int tq = td + 4 * q;
        if (tq >= lo && tq + 4 <= hi) {
            *(uint32_t *)(row + tq) = w[q];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (tq + k >= lo && tq + k < hi) row[tq + k] = (uint8_t)(w[q] >> (8 * k));
        }
    }
}

// ---- a workgroup of 256 threads ----

// op over the workgroup's values, the same in every thread; sh: 4 words of LDS.  The order is fixed (k_series_stats'
// pinned statistics depend on it for double): the __shfl_down tree 32 .. 1 inside a wave, lane 0 to LDS, then every
// thread folds the four waves' results onto `zero` in ascending wave order.  The leading barrier lets back-to-back
// calls share sh.
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T *sh, T zero, Op op)
{
    for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_down(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = zero;
#pragma unroll
    for (int i = 0; i < 4; ++i) r = op(r, sh[i]);
    return r;
}

template <typename T>
__device__ __forceinline__ T block_sum(T v, T *sh)
{
    return block_reduce(v, sh, (T)0, [](T a, T b) { return a + b; });
}

__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long *sh)
{
    return block_reduce(v, sh, 0ull, [](unsigned long long a, unsigned long long b) { return b > a ? b : a; });
}

// inclusive sums over the lanes of a wave
template <typename T>
__device__ __forceinline__ T wave_inclusive_sum(T v)
{
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(v, o);
        if (lane >= o) v += y;
    }
    return v;
}

// wave_total (what lane 63 holds) of the four waves -> before: the total of the waves below this thread's; returns the
// workgroup's total.  sh: 4 words of LDS, reusable by the next call (leading barrier).
__device__ __forceinline__ int block_wave_offsets(int wave_total, int *sh, int &before)
{
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 63) sh[wave] = wave_total;
    __syncthreads();
    int tot = 0;
    before = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += sh[w];
        tot += sh[w];
    }
    return tot;
}

// threads of the workgroup whose flag is set; rank: how many of them stand before this thread
__device__ __forceinline__ int block_count(bool flag, int *sh, int &rank)
{
    const uint64_t m = __ballot(flag);
    int before;
    const int tot = block_wave_offsets(__popcll(m), sh, before);
    rank = before + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
    return tot;
}
