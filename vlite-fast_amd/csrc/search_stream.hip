// The streaming stage of the search (definition: include/pb_hip.h, pb_search_set_gulp): filterbank samples arrive in
// pieces of any length (a second of pb_process output, say), are unpacked and transposed into the channel-major block
// d_xt as they arrive, and a gulp is searched where it has accumulated -- the search enters at search_block
// (search_run.hip), after the transpose that the block entry points do.  The dispersion tail that a gulp hands on to the
// next stays on the device: pb_search_gulp_advance moves it to the front of the block.
//
//   k_stream_append<NBIT>    the fast path: source and row length multiples of 16 bytes.  A workgroup takes 64 destination
//                            samples x 64 packed source bytes (64 / 128 / 256 channels at 8 / 4 / 2 bits): one 16-byte
//                            load per lane along the channel axis into LDS as it lies, then per (channel, 16 samples)
//                            sixteen LDS bytes are unpacked into one 16-byte store along time.
//   k_stream_append_bytes    any other source: single-byte loads as in k_transpose_codes, the same stores.
// Both tile the DESTINATION: a tile's first sample is a multiple of 64 in the block, whatever `fill` is, so every store
// inside [fill, fill + nsamp) is an aligned 16-byte one except in the first and last 16 samples of a row, which fall
// back to aligned dwords and then single bytes (stream_store16).
//
// What a lane may touch.  Source: the fast path loads 16 bytes at t * rowb + b with 0 <= t < nsamp and b + 16 <= rowb,
// the byte path the byte (t * nchan + c) / per with 0 <= t < nsamp and c < nchan, which is below nsamp * nchan * nbit / 8
// because a piece ends on a byte (pb_search_push refuses one that does not).  Destination: stream_store16 stores
// samples of [fill, fill + nsamp) only, rows c < nchan only; fill + nsamp <= max_samples <= tpitch.
//
// The tail needs no kernel: it is two 2-D device copies through the side buffer d_tail, [nchan][keep_max].
#include "search_internal.h"
#include "search_dev.h"         // the tile constants SA_* and stream_store16, shared with search_plane.hip

// codes: [nsamp][rowb] packed bytes, 16-byte aligned, rowb = nchan * NBIT / 8 a multiple of 16 -> xt[c][fill + t]
template <int NBIT>
__global__ __launch_bounds__(256) void k_stream_append(const uint8_t *__restrict__ codes, uint8_t *__restrict__ xt, int fill,
                                                       int nsamp, int nchan, int rowb, size_t tpitch)
{
    constexpr int PER = 8 / NBIT, CT = SA_B * PER, MASK = (1 << NBIT) - 1;
    __shared__ uint32_t tile[SA_T][SA_PITCH / 4];
    const int td0 = (fill & ~(SA_T - 1)) + blockIdx.x * SA_T;       // the tile's first destination sample
    const int b0 = blockIdx.y * SA_B;
    {
        const int tt = threadIdx.x >> 2, seg = threadIdx.x & 3;
        const int t = td0 + tt - fill, b = b0 + 16 * seg;           // source sample, byte of its row
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (t >= 0 && t < nsamp && b + 16 <= rowb) v = *(const uint4 *)(codes + (size_t)t * rowb + b);
        uint32_t *p = &tile[tt][4 * seg];
        p[0] = v.x;
        p[1] = v.y;
        p[2] = v.z;
        p[3] = v.w;
    }
    __syncthreads();
    const uint8_t *tb = (const uint8_t *)&tile[0][0];
    const int c0 = b0 * PER;
#pragma unroll
    for (int j0 = 0; j0 < CT * 4; j0 += 256) {
        const int j = j0 + threadIdx.x;
        const int cc = j >> 2, g = j & 3;                           // four neighbouring lanes write one 64-byte line
        const int c = c0 + cc;
        if (c >= nchan) continue;                                   // (no barrier below)
        const int cb = cc / PER, sh = (cc % PER) * NBIT;
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            w[q] = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[q] |= (((uint32_t)tb[(16 * g + 4 * q + k) * SA_PITCH + cb] >> sh) & MASK) << (8 * k);
        }
        stream_store16(xt + (size_t)c * tpitch, td0 + 16 * g, fill, fill + nsamp, w);
    }
}

// the same for any source address and row length: sample n = t * nchan + c lies in byte n / per, low bits first
__global__ __launch_bounds__(256) void k_stream_append_bytes(const uint8_t *__restrict__ codes, uint8_t *__restrict__ xt,
                                                             int fill, int nsamp, int nchan, int nbit, size_t tpitch)
{
    __shared__ uint8_t tile[SA_T][SA_BPITCH];
    const int td0 = (fill & ~(SA_T - 1)) + blockIdx.x * SA_T, c0 = blockIdx.y * 64;
    const int per = 8 / nbit, maskv = (1 << nbit) - 1;
    for (int i = threadIdx.x; i < SA_T * 64; i += 256) {
        const int tt = i >> 6, cc = i & 63;
        const int t = td0 + tt - fill, c = c0 + cc;
        uint8_t v = 0;
        if (t >= 0 && t < nsamp && c < nchan) {
            const size_t n = (size_t)t * nchan + c;
            v = (codes[n / per] >> (nbit * (n % per))) & maskv;
        }
        tile[tt][cc] = v;
    }
    __syncthreads();
    const int cc = threadIdx.x >> 2, g = threadIdx.x & 3;
    const int c = c0 + cc;
    if (c >= nchan) return;
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        w[q] = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[q] |= (uint32_t)tile[16 * g + 4 * q + k][cc] << (8 * k);
    }
    stream_store16(xt + (size_t)c * tpitch, td0 + 16 * g, fill, fill + nsamp, w);
}

void search_gulp_free(pb_search *s)
{
    search_release({s->gp.d_tail}, nullptr, s->gp.ev, 5);
    s->gp = {};
}

static const char *const GULP_OFF = "streaming is not switched on (pb_search_set_gulp)";

extern "C" int pb_search_set_gulp(pb_search *s, int keep_max)
{
    const char *fn = "pb_search_set_gulp";
    if (!s) return search_fail(s, fn, "no search handle");
    if (keep_max < 0 || keep_max > s->max_samples) return search_fail(s, fn, "keep_max must be in 0..max_samples");
    if (keep_max > 0 && s->pol.max > 0) return search_fail(s, fn, "polarisation is switched on (pb_search_set_pol): four-product blocks are not streamed");
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    search_gulp_free(s);
    if (keep_max == 0) return PB_OK;
    const size_t kpitch = ((size_t)keep_max + 63) / 64 * 64;
    hipError_t e = hipMalloc((void **)&s->gp.d_tail, kpitch * s->nchan);
    for (int i = 0; i < 5 && e == hipSuccess; ++i) e = hipEventCreate(&s->gp.ev[i]);
    if (e != hipSuccess) {
        search_gulp_free(s);
        s->err = std::string(fn) + ": " + hipGetErrorString(e);
        return PB_EHIP;
    }
    s->gp.kpitch = kpitch;
    s->gp.keep_max = keep_max;
    return PB_OK;
}

extern "C" int pb_search_push(pb_search *s, const void *codes, int codes_on_device, int nsamp, int nbit, int *fill)
{
    const char *fn = "pb_search_push";
    int rc = search_enter(s, fn, s && s->gp.keep_max > 0, GULP_OFF, true, "");
    if (rc) return rc;
    if (!(nbit == 8 || nbit == 4 || nbit == 2)) return search_fail(s, fn, "nbit must be 8, 4 or 2");
    if (nsamp < 0 || (nsamp > 0 && !codes)) return search_fail(s, fn, "no codes, or a negative number of samples");
    if ((long long)s->gp.fill + nsamp > s->max_samples)
        return search_fail(s, fn, "the accumulated block would exceed max_samples");
    if (((long long)nsamp * s->nchan * nbit) % 8) return search_fail(s, fn, "a piece must end on a byte");
    if (s->gp.cleaned && nsamp > 0)
        return search_fail(s, fn, "the block was cleaned in place by a gulp call: pb_search_gulp_advance comes before the next push");
    if (nsamp > 0) {
        SCHK(s, hipSetDevice(s->device));
        const size_t nbytes = (size_t)nsamp * s->nchan * nbit / 8;
        const uint8_t *src = (const uint8_t *)codes;
        SCHK(s, hipEventRecord(s->gp.ev[0], s->stream));
        if (!codes_on_device) {
            SCHK(s, hipMemcpyAsync(s->d_codes, codes, nbytes, hipMemcpyHostToDevice, s->stream));
            src = s->d_codes;
        }
        SCHK(s, hipEventRecord(s->gp.ev[1], s->stream));
        const int f = s->gp.fill;
        const unsigned ntile = (unsigned)((f + nsamp + SA_T - 1) / SA_T - f / SA_T);
        const long long rowbits = (long long)s->nchan * nbit;
        if (rowbits % 128 == 0 && (uintptr_t)src % 16 == 0) {
            const int rowb = (int)(rowbits / 8);
            dim3 g(ntile, (rowb + SA_B - 1) / SA_B);
            if (nbit == 8) k_stream_append<8><<<g, 256, 0, s->stream>>>(src, s->d_xt, f, nsamp, s->nchan, rowb, s->tpitch);
            else if (nbit == 4) k_stream_append<4><<<g, 256, 0, s->stream>>>(src, s->d_xt, f, nsamp, s->nchan, rowb, s->tpitch);
            else k_stream_append<2><<<g, 256, 0, s->stream>>>(src, s->d_xt, f, nsamp, s->nchan, rowb, s->tpitch);
        } else {
            dim3 g(ntile, (s->nchan + 63) / 64);
            k_stream_append_bytes<<<g, 256, 0, s->stream>>>(src, s->d_xt, f, nsamp, s->nchan, nbit, s->tpitch);
        }
        SCHK(s, hipEventRecord(s->gp.ev[2], s->stream));
        SCHK(s, hipGetLastError());
        SCHK(s, hipStreamSynchronize(s->stream));       // the caller may reuse `codes` from here on
        s->gp.ms[0] = search_ms(s->gp.ev[0], s->gp.ev[1]);
        s->gp.ms[1] = search_ms(s->gp.ev[1], s->gp.ev[2]);
        s->gp.fill = f + nsamp;
        s->gp.tail_n = 0;
    }
    if (fill) *fill = s->gp.fill;
    return PB_OK;
}

// rows [first, first + n) of the block -> d_tail[.][0, n)
static int gulp_save(pb_search *s, int first, int n)
{
    SCHK(s, hipMemcpy2DAsync(s->gp.d_tail, s->gp.kpitch, s->d_xt + first, s->tpitch, (size_t)n, (size_t)s->nchan,
                             hipMemcpyDeviceToDevice, s->stream));
    s->gp.tail_n = n;
    return PB_OK;
}

// the opening of both gulp searches: the refusals of the block entry points, the raw tail put aside where the cleaning is
// about to overwrite it, the events that the block entry points record around their copy and transpose
static int gulp_search(pb_search *s, const char *fn, float thresh, bool want_peaks)
{
    int rc = search_enter(s, fn, s && s->gp.keep_max > 0, GULP_OFF, true, "");
    if (rc) return rc;
    const int fill = s->gp.fill;
    if (fill - s->max_delay < 64) return search_fail(s, fn, "block shorter than the largest dispersion delay");
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipEventRecord(s->ev[0], s->stream));
    SCHK(s, hipEventRecord(s->ev[1], s->stream));
    const bool clean = s->rfi.narrow || s->rfi.broad || s->chan.tol > 0;
    if (clean && !s->gp.cleaned) {
        rc = gulp_save(s, fill - std::min(s->gp.keep_max, fill), std::min(s->gp.keep_max, fill));
        if (rc) return rc;
    }
    SCHK(s, hipEventRecord(s->ev[2], s->stream));
    rc = search_block(s, fill, thresh, want_peaks, s->gp.cleaned != 0);
    if (rc) return rc;
    if (clean) s->gp.cleaned = 1;
    return PB_OK;
}

extern "C" int pb_search_gulp_peaks(pb_search *s, float threshold, int32_t *peaks, int max_out, int *npeaks, int *tout)
{
    const char *fn = "pb_search_gulp_peaks";
    if (!s) return search_fail(s, fn, "no search handle");
    if (!peaks || !npeaks || max_out < 1) return search_fail(s, fn, "no room for the peaks");
    const int rc = gulp_search(s, fn, threshold, true);
    return rc ? rc : search_peaks_out(s, peaks, max_out, npeaks, tout);
}

extern "C" int pb_search_gulp_run(pb_search *s, float *snr, uint8_t *width_log2, uint32_t *series, float *stats, int *tout)
{
    const int rc = gulp_search(s, "pb_search_gulp_run", 0.f, false);
    return rc ? rc : search_run_out(s, snr, width_log2, series, stats, tout);
}

extern "C" int pb_search_gulp_advance(pb_search *s, int keep)
{
    const char *fn = "pb_search_gulp_advance";
    int rc = search_enter(s, fn, s && s->gp.keep_max > 0, GULP_OFF, true, "");
    if (rc) return rc;
    const int fill = s->gp.fill;
    if (keep < 0 || keep > fill) return search_fail(s, fn, "keep must be in 0..fill");
    if (keep > s->gp.keep_max) return search_fail(s, fn, "keep exceeds keep_max");
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipEventRecord(s->gp.ev[3], s->stream));
    const bool raw = !s->gp.cleaned;
    if (keep == 0 || (raw && keep == fill)) {
        // nothing to move: the block is emptied, or stays where it is
    } else if (raw && 2 * (long long)keep <= fill) {
        // raw where it lies, and source and destination apart: one copy
        SCHK(s, hipMemcpy2DAsync(s->d_xt, s->tpitch, s->d_xt + (fill - keep), s->tpitch, (size_t)keep, (size_t)s->nchan,
                                 hipMemcpyDeviceToDevice, s->stream));
    } else {
        // through the side buffer.  After a cleaned gulp it already holds the raw samples [fill - tail_n, fill), tail_n =
        // min(keep_max, fill) >= keep; on a raw block the two ranges overlap, and the buffer keeps the move exact whatever
        // order a copy moves its bytes in.
        if (raw) {
            rc = gulp_save(s, fill - keep, keep);
            if (rc) return rc;
        }
        SCHK(s, hipMemcpy2DAsync(s->d_xt, s->tpitch, s->gp.d_tail + (s->gp.tail_n - keep), s->gp.kpitch, (size_t)keep,
                                 (size_t)s->nchan, hipMemcpyDeviceToDevice, s->stream));
    }
    SCHK(s, hipEventRecord(s->gp.ev[4], s->stream));
    SCHK(s, hipStreamSynchronize(s->stream));
    s->gp.ms[2] = search_ms(s->gp.ev[3], s->gp.ev[4]);
    s->gp.fill = keep;
    s->gp.cleaned = 0;
    s->gp.tail_n = 0;
    return PB_OK;
}

extern "C" int pb_search_gulp_fetch(pb_search *s, uint8_t *xt, size_t nbytes, int *fill)
{
    const char *fn = "pb_search_gulp_fetch";
    int rc = search_enter(s, fn, s && s->gp.keep_max > 0, GULP_OFF, true, "");
    if (rc) return rc;
    const size_t n = (size_t)s->gp.fill;
    if (s->gp.cleaned)
        return search_fail(s, fn, "the block was cleaned in place by a gulp call (pb_search_fetch_clean reads it); the raw tail comes back with pb_search_gulp_advance");
    if (n > 0 && (!xt || nbytes < n * s->nchan)) return search_fail(s, fn, "the buffer is smaller than nchan x fill");
    if (n > 0) {
        SCHK(s, hipSetDevice(s->device));
        SCHK(s, hipStreamSynchronize(s->stream));
        SCHK(s, hipMemcpy2D(xt, n, s->d_xt, s->tpitch, n, s->nchan, hipMemcpyDeviceToHost));
    }
    if (fill) *fill = (int)n;
    return PB_OK;
}

extern "C" int pb_search_gulp_timers(const pb_search *s, float *ms3)
{
    return search_get_ms(s, s ? s->gp.ms : nullptr, 3, ms3);
}
