// The fp32 entry of the streaming stage (definition: include/pb_hip.h, pb_search_push_f32): a piece of an fp32 plane
// [time][nchan] -- pb_output_dev's `ave` at npol = 1, a coadder's d_sum -- is quantised with the reference's 8-bit rule
// (sel_and_dig_8b, src/pb_kernels.cu:711-735) and appended to the channel-major block d_xt, where pb_search_push
// appends code bytes.  The search then sees 8-bit depth whatever depth the files and rings are written at.
//
//   k_plane_append<true>     the fast path: source 16-byte aligned and nchan a multiple of 4.  A workgroup takes 64
//                            destination samples x 64 channels: one float4 load per lane along the channel axis, four
//                            times over; the four bytes quantised in registers go to the LDS tile as one dword; then
//                            per (channel, 16 samples) sixteen LDS bytes become one 16-byte store along time.
//   k_plane_append<false>    any other 4-byte aligned source: single float loads, the same tile, the same stores.
// Both tile the DESTINATION as k_stream_append_bytes does (search_dev.h: SA_T, SA_BPITCH, stream_store16).
//
// What a lane may touch.  Source: the float (or the four floats) at t * nchan + c with 0 <= t < nsamp and c (c + 3) <
// nchan, i.e. inside [plane, plane + nsamp * nchan).  Destination: stream_store16 stores samples of [fill, fill + nsamp)
// only, rows c < nchan only; fill + nsamp <= max_samples <= tpitch.
// LDS: the tile's pitch of 17 dwords puts the 32 dword writes of half a wave (two samples x 16 channel quads) on 31
// banks and the byte reads of the store stage where k_stream_append_bytes has them.
#include "search_internal.h"
#include "search_dev.h"

// One sample, operation by operation as include/pb_hip.h states it (-ffp-contract=off: no operation is fused): a
// binary32 product, a binary64 quotient and sum rounded to binary32, a select that sends NaN to 0, a truncating cast.
__device__ __forceinline__ uint32_t plane_quantise8(float x, float scale)
{
    const float v = x * scale;
    const float tmp = (float)((double)v / 0.02957 + 127.5);
    return tmp > 0 ? (tmp >= 255 ? 255u : (uint32_t)(uint8_t)tmp) : 0u;
}

// plane: [nsamp][nchan] fp32 -> xt[c][fill + t]
template <bool VEC>
__global__ __launch_bounds__(256) void k_plane_append(const float *__restrict__ plane, float scale, uint8_t *__restrict__ xt,
                                                      int fill, int nsamp, int nchan, size_t tpitch)
{
    __shared__ uint32_t tile[SA_T][SA_BPITCH / 4];
    const int td0 = (fill & ~(SA_T - 1)) + blockIdx.x * SA_T, c0 = blockIdx.y * 64;
    if (VEC) {
        const int seg = threadIdx.x & 15;
        const int c = c0 + 4 * seg;
#pragma unroll
        for (int tt = threadIdx.x >> 4; tt < SA_T; tt += 16) {
            const int t = td0 + tt - fill;
            uint32_t w = 0u;
            if (t >= 0 && t < nsamp && c < nchan) {                 // nchan % 4 == 0: c + 3 < nchan as well
                const float4 v = *(const float4 *)(plane + (size_t)t * nchan + c);
                w = plane_quantise8(v.x, scale) | plane_quantise8(v.y, scale) << 8 | plane_quantise8(v.z, scale) << 16 |
                    plane_quantise8(v.w, scale) << 24;
            }
            tile[tt][seg] = w;
        }
    } else {
        uint8_t *tb = (uint8_t *)&tile[0][0];
        for (int i = threadIdx.x; i < SA_T * 64; i += 256) {
            const int tt = i >> 6, cc = i & 63;
            const int t = td0 + tt - fill, c = c0 + cc;
            uint32_t q = 0u;
            if (t >= 0 && t < nsamp && c < nchan) q = plane_quantise8(plane[(size_t)t * nchan + c], scale);
            tb[tt * SA_BPITCH + cc] = (uint8_t)q;
        }
    }
    __syncthreads();
    const uint8_t *tb = (const uint8_t *)&tile[0][0];
    const int cc = threadIdx.x >> 2, g = threadIdx.x & 3;
    const int c = c0 + cc;
    if (c >= nchan) return;
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        w[q] = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[q] |= (uint32_t)tb[(16 * g + 4 * q + k) * SA_BPITCH + cc] << (8 * k);
    }
    stream_store16(xt + (size_t)c * tpitch, td0 + 16 * g, fill, fill + nsamp, w);
}

extern "C" int pb_search_push_f32(pb_search *s, const float *plane, int plane_on_device, int nsamp, float scale, int *fill)
{
    const char *fn = "pb_search_push_f32";
    int rc = search_enter(s, fn, s && s->gp.keep_max > 0, "streaming is not switched on (pb_search_set_gulp)", true, "");
    if (rc) return rc;
    if (nsamp < 0 || (nsamp > 0 && !plane)) return search_fail(s, fn, "no plane, or a negative number of samples");
    if ((long long)s->gp.fill + nsamp > s->max_samples)
        return search_fail(s, fn, "the accumulated block would exceed max_samples");
    if (!(scale > 0.f) || !std::isfinite(scale)) return search_fail(s, fn, "scale must be finite and greater than 0");
    if (plane_on_device && (uintptr_t)plane % 4) return search_fail(s, fn, "a device plane must lie at a multiple of 4 bytes");
    if (s->gp.cleaned && nsamp > 0)
        return search_fail(s, fn, "the block was cleaned in place by a gulp call: pb_search_gulp_advance comes before the next push");
    if (nsamp > 0) {
        SCHK(s, hipSetDevice(s->device));
        // a host plane goes through the staging buffer of the block entry points (max_samples * nchan bytes) in slices of
        // max_samples / 4 >= 16 samples; a device plane is one slice, read where it lies
        const int per = plane_on_device ? nsamp : s->max_samples / 4;
        float ms_copy = 0.f, ms_append = 0.f;
        for (int off = 0; off < nsamp; off += per) {
            const int n = std::min(per, nsamp - off), f = s->gp.fill + off;
            const float *src = plane + (size_t)off * s->nchan;
            SCHK(s, hipEventRecord(s->gp.ev[0], s->stream));
            if (!plane_on_device) {
                SCHK(s, hipMemcpyAsync(s->d_codes, src, (size_t)n * s->nchan * sizeof(float), hipMemcpyHostToDevice, s->stream));
                src = (const float *)s->d_codes;
            }
            SCHK(s, hipEventRecord(s->gp.ev[1], s->stream));
            dim3 g((unsigned)((f + n + SA_T - 1) / SA_T - f / SA_T), (unsigned)((s->nchan + 63) / 64));
            if (s->nchan % 4 == 0 && (uintptr_t)src % 16 == 0)
                k_plane_append<true><<<g, 256, 0, s->stream>>>(src, scale, s->d_xt, f, n, s->nchan, s->tpitch);
            else
                k_plane_append<false><<<g, 256, 0, s->stream>>>(src, scale, s->d_xt, f, n, s->nchan, s->tpitch);
            SCHK(s, hipEventRecord(s->gp.ev[2], s->stream));
            SCHK(s, hipGetLastError());
            SCHK(s, hipStreamSynchronize(s->stream));   // the staging buffer, and in the end `plane`, may be reused from here on
            ms_copy += search_ms(s->gp.ev[0], s->gp.ev[1]);
            ms_append += search_ms(s->gp.ev[1], s->gp.ev[2]);
        }
        s->gp.ms[0] = ms_copy;
        s->gp.ms[1] = ms_append;
        s->gp.fill += nsamp;
        s->gp.tail_n = 0;
    }
    if (fill) *fill = s->gp.fill;
    return PB_OK;
}
