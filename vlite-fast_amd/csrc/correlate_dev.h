// What the correlator's two files share (pb_correlate.hip: k_correlate; pb_correlate_track.hip: k_correlate_track): the
// kernels' arguments, the baseline index, the tile's rows in flight, the loader's walk over a window, one term of the
// definition, and the prefix kernel's launch.
#pragma once
#include "pb_job.h"

struct CorrArgs {
    const float2 *X;       // one stream's spectra [A][S][2][R][4096]
    const int32_t *row0;   // [ngate][4096] first row of the gate per channel
    const int32_t *pref;   // [nbl][T + 1] rows before t with both weights > 0; nullptr on the raw stream
    float2 *vis;           // [ngate][nbl][4][4096]
    int32_t *used;         // [ngate][nbl][4096]
    int A, S, R, T, nrows;
    int i0, j0;            // first antenna of the tile's rows and columns
};

__host__ __device__ inline int corr_bl(int A, int i, int j) { return i * A - i * (i - 1) / 2 + (j - i); }

// rows in flight per buffer: about 32 8-byte loads per lane and buffer
constexpr int corr_rows_in_flight(int nl) { return nl == 1 ? 16 : nl == 2 ? 8 : nl == 3 ? 5 : nl == 4 ? 4 : 2; }

// the loader's position: row k of a lane's window, as (row within its segment, offset of that row in an antenna's plane)
struct CorrWalk {
    int k, row;
    size_t off;
    __device__ __forceinline__ CorrWalk(int r0, int R, size_t seg_stride) : k(0), row(r0 % R), off((size_t)(r0 / R) * seg_stride + (size_t)row * PB_NCHANOUT) {}
    // one row on; rows past the window's end repeat its last row (loaded, never added): no address leaves the window
    __device__ __forceinline__ void step(int nrows, int R, size_t seg_stride, size_t pol_stride)
    {
        if (k < nrows - 1) {
            ++k;
            ++row;
            off += PB_NCHANOUT;
            if (row == R) {
                row = 0;
                off += seg_stride - pol_stride;
            }
        }
    }
};

// one term (include/pb_hip.h): the lines of the coherence definition, acc = acc + term
__device__ __forceinline__ void corr_term(float2 &acc, const float2 A, const float2 B)
{
    const float rxx = A.x * B.x, ryy = A.y * B.y;
    const float re = rxx + ryy;
    const float iyx = A.y * B.x, ixy = A.x * B.y;
    const float im = iyx - ixy;
    acc.x = acc.x + re;
    acc.y = acc.y + im;
}

// a tile's outputs: the accumulators of baseline bl of gate g and, where asked for, its rows_used
__device__ __forceinline__ void corr_store(const CorrArgs &a, int g, int c, int r0, int bl, const float2 (&acc)[4])
{
    const int nbl = a.A * (a.A + 1) / 2;
    const size_t o = (size_t)g * nbl + bl;
    if (a.vis) {
#pragma unroll
        for (int pr = 0; pr < 4; ++pr) a.vis[(o * 4 + pr) * PB_NCHANOUT + c] = acc[pr];
    }
    if (a.used) {
        int n = a.nrows;
        if (a.pref) {
            const int32_t *P = a.pref + (size_t)bl * (a.T + 1);
            n = P[r0 + a.nrows] - P[r0];
        }
        a.used[o * PB_NCHANOUT + c] = n;
    }
}

// pb_correlate.hip: k_corr_prefix on stream st -- pref[bl][t] = the number of rows before t whose weight is > 0 for
// both antennas of baseline bl, t = 0 .. T
PB_LOCAL void corr_prefix_launch(const float *wrow, int A, size_t ant_stride, int T, int32_t *pref, hipStream_t st);
