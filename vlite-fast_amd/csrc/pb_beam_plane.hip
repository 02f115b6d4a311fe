// Beams as filterbank planes on the device (include/pb_hip.h: pb_beam_planes): the four-product block and the row counts
// that pb_beamform / pb_beamform_proj would copy to the host stay in HBM, and per (beam, output sample, channel) AA + BB,
// rescaled to a full window's rows, becomes one value of a zero-mean, unit-variance fp32 plane [nbeam][nout][4096] -- what
// pb_search_push_f32 quantises where it lies.  The level that is divided out is the plane's own mean per (beam, channel),
// or one the caller hands in (a running level over batches).
//
// k_beam_plane<SUM, WRITE>: a lane owns one channel of one beam and walks one chunk of PLANE_CHUNK = 32 consecutive output
//   samples (the definition's chunk) in ascending order; neighbouring lanes own neighbouring channels, so every load and
//   store is a coalesced dword per lane.  It reads AA, BB and the row count -- never CR and CI --, PLANE_UNROLL samples'
//   loads in flight.  SUM adds the chunk's (double)J in binary64 and counts its samples with rows, into
//   psum / pcnt [nbeam][nchunk][4096]; WRITE divides by the level and stores the plane.
//     level_in given:  <true, true>, one pass over the block (12 bytes read, 4 written per value);
//     no level_in:     <true, false>, k_beam_level, then <false, true>: the level needs all of a (beam, channel)'s samples
//                      before the first plane value.  The second pass walks the grid backwards, so that it starts on what
//                      the first pass touched last.
//   The grid is channel blocks x chunks x beams, ceil(nout / 32) independent pieces per (beam, channel): four beams of one
//   second (nout = 1280) are 2560 workgroups of 256 lanes.
// k_beam_level: a lane adds its (beam, channel)'s chunk sums in ascending chunk order in binary64 and divides by the count.
// All three are bound by memory traffic: per value two or three coalesced loads, one store, a correctly rounded division or
// two.  No LDS, no atomics, no scratch; the order of every sum is the definition's and depends on neither nbeam nor the
// launch.
// Host side: pb_plane_state holds the buffers this call adds (planes, levels, chunk sums); the beams come from beam_check
// and beam_queue of pb_beamform.hip on that call's own state (h->beam, or h->beamproj with matrices), whose timers are put
// back as they were.
#include "pb_beam.h"

#define PLANE_CHUNK 32      // output samples of a chunk: the definition's
#define PLANE_UNROLL 8      // samples whose loads are in flight
#define PLANE_LANES 256

struct PlaneArgs {
    const float *beams;     // [nbeam][nout][4][4096]
    const int32_t *used;    // [nbeam][nout][4096]
    const float *level;     // WRITE: the effective level [nbeam][4096]
    double *psum;           // SUM: [nbeam][nchunk][4096] chunk sums
    int32_t *pcnt;          // SUM: [nbeam][nchunk][4096] samples with rows
    float *plane;           // WRITE: [nbeam][nout][4096]
    int nout;
    float ftscr, g;         // (float)tscr; sqrtf((float)(2 * tscr))
};

template <bool SUM, bool WRITE>
__global__ __launch_bounds__(PLANE_LANES) void k_beam_plane(PlaneArgs a)
{
    // the second pass (WRITE alone) takes the grid from its end
    const int bx = SUM ? blockIdx.x : gridDim.x - 1 - blockIdx.x, ch = SUM ? blockIdx.y : gridDim.y - 1 - blockIdx.y;
    const int b = SUM ? blockIdx.z : gridDim.z - 1 - blockIdx.z;
    const int c = bx * PLANE_LANES + threadIdx.x, nchunk = gridDim.y;
    const int s0 = ch * PLANE_CHUNK, ns = a.nout - s0 < PLANE_CHUNK ? a.nout - s0 : PLANE_CHUNK;
    const size_t o0 = (size_t)b * a.nout + s0;
    const float *x = a.beams + o0 * 4 * PB_NCHANOUT + c;
    const int32_t *u = a.used + o0 * PB_NCHANOUT + c;
    float *out = WRITE ? a.plane + o0 * PB_NCHANOUT + c : nullptr;
    const float le = WRITE ? a.level[(size_t)b * PB_NCHANOUT + c] : 0.f;
    double sum = 0.0;
    int n = 0;
    for (int s = 0; s < ns; s += PLANE_UNROLL) {
        float aa[PLANE_UNROLL], bb[PLANE_UNROLL];
        int32_t us[PLANE_UNROLL];
#pragma unroll
        for (int i = 0; i < PLANE_UNROLL; ++i) {
            // samples past the chunk's end repeat its last one (loaded, never used): no address leaves the chunk
            const size_t k = s + i < ns ? s + i : ns - 1;
            aa[i] = x[k * 4 * PB_NCHANOUT];
            bb[i] = x[(k * 4 + 1) * PB_NCHANOUT];
            us[i] = u[k * PB_NCHANOUT];
        }
#pragma unroll
        for (int i = 0; i < PLANE_UNROLL; ++i) {
            if (s + i < ns) {
                // the definition's lines, one binary32 operation each
                const float I = aa[i] + bb[i];
                const float ratio = a.ftscr / (float)us[i];
                const float J = I * ratio;
                if (SUM && us[i] > 0) {
                    sum = sum + (double)J;
                    ++n;
                }
                if (WRITE) {
                    const float q = J / le;
                    const float d = q - 1.0f;
                    const float v = d * a.g;
                    out[(size_t)(s + i) * PB_NCHANOUT] = (us[i] > 0 && le > 0.f) ? v : 0.f;
                }
            }
        }
    }
    if (SUM) {
        const size_t o = ((size_t)b * nchunk + ch) * PB_NCHANOUT + c;
        a.psum[o] = sum;
        a.pcnt[o] = n;
    }
}

__global__ __launch_bounds__(PLANE_LANES) void k_beam_level(const double *psum, const int32_t *pcnt, int nchunk, float *level)
{
    const int c = blockIdx.x * PLANE_LANES + threadIdx.x, b = blockIdx.y;
    const size_t o = (size_t)b * nchunk * PB_NCHANOUT + c;
    double sum = 0.0;
    int n = 0;
    for (int ch = 0; ch < nchunk; ++ch) {
        sum = sum + psum[o + (size_t)ch * PB_NCHANOUT];
        n += pcnt[o + (size_t)ch * PB_NCHANOUT];
    }
    level[(size_t)b * PB_NCHANOUT + c] = n > 0 ? (float)(sum / (double)n) : 0.f;
}

struct PB_LOCAL pb_plane_state {
    DevBuf<float> planes;        // [nbeam][nout][4096]
    DevBuf<float> level;         // [nbeam][4096] the planes' own level L
    DevBuf<float> level_in;      // [nbeam][4096] the caller's
    DevBuf<double> psum;         // [nbeam][nchunk][4096]
    DevBuf<int32_t> pcnt;
    Event ev;                    // the level and plane kernels end here
    float ms[4] = {};
};

void pb_beam_plane_free(pb_handle *h)
{
    delete h->plane;      // (every call has returned with its stream drained)
    h->plane = nullptr;
}

extern "C" int pb_beam_planes(pb_handle *h, int stream, int nseg, int nbeam, const double *delay, const double *psi,
                              const float *gain, const float *proj, const int32_t *shift, int tscr, int nout,
                              const float *level_in, float *level_out, float *planes, const float **d_planes)
{
    if (!h) return PB_EINVAL;
    const std::string w = "pb_beam_planes";
    BeamCall c = {stream, nseg, nbeam, delay, psi, gain, proj, shift, tscr, nout, 0, 0, 0, 0};
    if (int rc = beam_check(h, w, proj != nullptr, c)) return rc;
    const size_t nlev = (size_t)nbeam * PB_NCHANOUT;
    if (level_in)
        for (size_t k = 0; k < nlev; ++k)
            if (!std::isfinite(level_in[k]) || level_in[k] < 0.f) return fail(h, PB_EINVAL, w + ": a level_in value is not finite or is negative");

    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->plane) h->plane = new pb_plane_state;
    pb_plane_state *ps = h->plane;
    HIPCHK(h, ps->ev.create(hipEventDefault));      // (timed)
    const int nchunk = (nout + PLANE_CHUNK - 1) / PLANE_CHUNK;
    HIPCHK(h, ps->planes.grow(h, c.nused));
    HIPCHK(h, ps->level.grow(h, nlev));
    if (level_in) HIPCHK(h, ps->level_in.grow(h, nlev));
    HIPCHK(h, ps->psum.grow(h, nlev * nchunk));
    HIPCHK(h, ps->pcnt.grow(h, nlev * nchunk));

    // the beams and the row counts, on the device: the call's own state, whose timers stay those of its own last call
    pb_beam_state *&bs = proj ? h->beamproj : h->beam;
    float kept[3] = {};
    if (bs) for (int k = 0; k < 3; ++k) kept[k] = bs->ms[k];
    const BeamUpload up = {ps->level_in.p, level_in, nlev};
    if (int rc = beam_queue(h, bs, c, true, true, level_in ? &up : nullptr)) return rc;

    PlaneArgs a;
    a.beams = bs->beams.p;
    a.used = bs->used.p;
    a.level = level_in ? ps->level_in.p : ps->level.p;
    a.psum = ps->psum.p;
    a.pcnt = ps->pcnt.p;
    a.plane = ps->planes.p;
    a.nout = nout;
    a.ftscr = (float)tscr;
    a.g = sqrtf((float)(2 * tscr));
    const dim3 grid(PB_NCHANOUT / PLANE_LANES, nchunk, nbeam);      // nbeam nout <= 32768 (the 2 GiB limit): nchunk <= 1024
    if (level_in) k_beam_plane<true, true><<<grid, PLANE_LANES, 0, bs->st>>>(a);
    else k_beam_plane<true, false><<<grid, PLANE_LANES, 0, bs->st>>>(a);
    k_beam_level<<<dim3(PB_NCHANOUT / PLANE_LANES, nbeam), PLANE_LANES, 0, bs->st>>>(ps->psum.p, ps->pcnt.p, nchunk, ps->level.p);
    if (!level_in) k_beam_plane<false, true><<<grid, PLANE_LANES, 0, bs->st>>>(a);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(ps->ev.e, bs->st));
    HIPCHK(h, ps->level.to_host(level_out, nlev, bs->st));
    HIPCHK(h, ps->planes.to_host(planes, c.nused, bs->st));
    HIPCHK(h, bs->finish());
    ps->ms[0] = bs->ms[0];
    ps->ms[1] = bs->ms[1];
    HIPCHK(h, hipEventElapsedTime(&ps->ms[2], bs->ev[2], ps->ev.e));
    HIPCHK(h, hipEventElapsedTime(&ps->ms[3], ps->ev.e, bs->ev[3]));
    for (int k = 0; k < 3; ++k) bs->ms[k] = kept[k];
    if (d_planes) *d_planes = ps->planes.p;
    return PB_OK;
}

extern "C" int pb_beam_planes_timers(const pb_handle *h, float *ms4)
{
    if (!h || !ms4) return PB_EINVAL;
    for (int k = 0; k < 4; ++k) ms4[k] = h->plane ? h->plane->ms[k] : 0.f;
    return PB_OK;
}
