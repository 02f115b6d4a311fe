// The beamformer (include/pb_hip.h: pb_beamform, pb_beamform_proj): per beam a weighted, phase-rotated sum of a handle's
// antennas per (pol, row, channel), detected into the four coherence products and added over windows of tscr rows --
// from the complex in-band spectra that the coherence channeliser leaves in HBM (BufSet::d_Praw / d_Pkur, float2
// [A][S][2][R][4096]).  The sum over a window's rows is in row order, so a lane walks its channel's rows alone and the
// parallelism is channels x runs of output samples x beam tiles.  pb_beamform's weight is the beam's steering weight
// s[b][a][c], the same for both pols; pb_beamform_proj's is free per (beam, pol, antenna, channel): s put through a
// complex matrix proj[p][c] per (pol, channel), w'[b][p][j][c] = sum over a of s[b][a][c] proj[p][c][a][j], so that the
// beam voltage is s^T (P x) -- per-channel spatial nulls (vlite-fast_amd/nulling.py makes P = I - v v^H from the
// correlator's matrices) or per-pol calibration, then the beam.
//
// beam_steer: the steering weight gain * (cr, sr), the header's binary64 phase and binary32 rotation polynomial.
// k_beam_weights (plain): W[b][a][c] = s; once per call, one lane per value.
// k_beamproj_weights<NA> (projecting): W'[b][p][j][c], once per call; a lane owns one (b, c), forms the NA steering
//   weights once and keeps them in registers, then walks the 2 NA columns.  proj lies on the device as float2
//   [2][NA][NA][4096] (pol, row a, column j, channel): the host checks it, transposes it into pinned memory and uploads it
//   from there, and every read is coalesced over the channels.
// k_beam_prefix: the running count of rows whose weight is > 0 for every antenna that counts (one wave, ballots), so that
//   rows_used of the excised stream is a difference of two entries.  Plain: per beam, the antennas of non-zero gain.
//   Projecting: one count for the whole call over EVERY antenna of the handle (a matrix mixes the antennas, so no gain
//   takes one out of the count).
// beam_walk<NA, NPW>, the body of k_beamform<NA> (NPW = 1: one set of weights) and k_beamform_proj<NA> (NPW = 2: pol p
//   uses w'[b][p]): one 64-lane workgroup = 64 channels, a run of output samples (about BEAM_CHUNK_ROWS rows) and a tile
//   of BEAM_TILE beams; a lane owns one channel and keeps the tile's weights (2 NPW NA BEAM_TILE floats) and its
//   4 BEAM_TILE accumulators in registers, as pairs of beams: the definition's lines are written once on two-element
//   vectors (beams 2j and 2j + 1), which the compiler turns into packed binary32 multiplies and adds without keeping a
//   weight twice.  Every spectrum value is loaded once per workgroup and serves all beams of the tile; the lane holds U
//   rows and reloads a row's slot as soon as the row is added, so U - 1 rows' loads are in flight.  The windows of a run
//   follow one another without a gap, so the lane walks one stretch of rows and stores and clears its accumulators every
//   tscr rows.  A channel's stretch differs from its neighbours' only in its first row (shift): the addresses are
//   coalesced over the channels whenever neighbouring shifts are equal and correct when they are not.  The tile stays
//   four beams at every antenna count: with both pols' weights a tile of two above four antennas compiled to fewer
//   registers but read the spectra twice as often and was slower wherever it was measured (eight antennas: 1.35 against
//   1.08 ms for four beams, 3.95 against 2.75 ms for sixteen).  k_beamform_proj asks for two waves per SIMD
//   (amdgpu_waves_per_eu), which at eight antennas makes the compiler fit 250 VGPRs where it otherwise took 256 and 4
//   AGPRs and one wave (sixteen beams: 3.42 ms).  No LDS, no atomics, no scratch.
// Host side: pb_beam_state is a job of csrc/pb_job.h (stream, stage events and times, owned buffers that grow, teardown);
// a handle keeps one for each of the two calls, and beam_call is the host path of both: beam_check (the refusals) and
// beam_queue (uploads, weights, row counts, beam kernel), which pb_beam_planes (pb_beam_plane.hip) runs too, then the
// copies to the host.  What the call refuses about the handle, the stream and the batch is that header's spectra_check_*.
#include "pb_beam.h"      // the call's state, the kernels' arguments, and what pb_beam_plane.hip shares of the host path
#include "rotation_dev.h"

#include <vector>

#define BEAM_TILE 4             // beams of a workgroup
#define BEAM_CHUNK_ROWS 32      // rows of a workgroup's run: max(1, BEAM_CHUNK_ROWS / tscr) output samples

typedef float beam_pair __attribute__((ext_vector_type(2)));      // one value for each of two beams

namespace {

// rows of the lane's buffer: about 32 8-byte loads per lane
constexpr int beam_rows_in_flight(int na) { return na == 1 ? 16 : na == 2 ? 8 : na == 3 ? 5 : na == 4 ? 4 : na <= 6 ? 3 : 2; }

}  // namespace

// the steering weight of channel c: the phase (include/pb_hip.h) in binary64, every operation rounded once
__device__ __forceinline__ float2 beam_steer(int c, double q, double psi, float g)
{
    const double k = (double)(PB_CHANMIN + c);
    const double kq = k * q;
    const double t = psi + kq;
    const double r64 = t - rint(t);
    float cr, sr;
    img_rotation((float)r64, cr, sr);
    return make_float2(g * cr, g * sr);
}

__global__ __launch_bounds__(64) void k_beam_weights(const double *q, const double *psi, const float *gain, float2 *W)
{
    const int c = blockIdx.x * 64 + threadIdx.x, ba = blockIdx.y;
    W[(size_t)ba * PB_NCHANOUT + c] = beam_steer(c, q[ba], psi[ba], gain[ba]);
}

template <int NA>
__global__ __launch_bounds__(64) void k_beamproj_weights(const double *q, const double *psi, const float *gain,
                                                         const float2 *proj, float2 *W)
{
    const int c = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    float sr[NA], si[NA];
#pragma unroll
    for (int l = 0; l < NA; ++l) {
        const float2 s = beam_steer(c, q[b * NA + l], psi[b * NA + l], gain[b * NA + l]);
        sr[l] = s.x;
        si[l] = s.y;
    }
    // w' = s^T P per pol: rows of P ascending, one operation per line
#pragma unroll
    for (int p = 0; p < 2; ++p)
        for (int j = 0; j < NA; ++j) {
            float ur = 0.f, ui = 0.f;
#pragma unroll
            for (int l = 0; l < NA; ++l) {
                const float2 P = proj[((size_t)(p * NA + l) * NA + j) * PB_NCHANOUT + c];
                const float rr = sr[l] * P.x, ii = si[l] * P.y;
                const float tr = rr - ii;
                const float ir = si[l] * P.x, ri = sr[l] * P.y;
                const float ti = ir + ri;
                ur = ur + tr;
                ui = ui + ti;
            }
            W[((size_t)(b * 2 + p) * NA + j) * PB_NCHANOUT + c] = make_float2(ur, ui);
        }
}

// pref[b][t] = the number of rows before t whose weight is > 0 for every antenna with gain[b][a] != 0 (gain = nullptr:
// for every antenna), t = 0 .. T
__global__ __launch_bounds__(64) void k_beam_prefix(const float *wrow, const float *gain, int A, size_t ant_stride, int T,
                                                    int32_t *pref)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const float *g = gain ? gain + (size_t)b * A : nullptr;
    int32_t *P = pref + (size_t)b * (T + 1);
    int total = 0;
    if (lane == 0) P[0] = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        bool ok = t < T;
        if (ok)
            for (int a = 0; a < A; ++a)
                if ((!g || g[a] != 0.f) && !(wrow[(size_t)a * ant_stride + t] > 0.f)) ok = false;
        const unsigned long long m = __ballot(ok);
        if (t < T) P[t + 1] = total + __popcll(m & (~0ull >> (63 - lane)));
        total += __popcll(m);
    }
}

// NPW: the pols that have weights of their own, 1 (pb_beamform) or 2 (pb_beamform_proj)
template <int NA, int NPW>
__device__ __forceinline__ void beam_walk(const BeamArgs &a)
{
    constexpr int U = beam_rows_in_flight(NA);
    // the beam tiles of one run of rows are neighbours in blockIdx.y: they run at about the same time, 64 workgroups
    // apart (so on the same XCD), and all but the first can find the run's spectra in the L2
    const int ntile = (a.nbeam + BEAM_TILE - 1) / BEAM_TILE;
    const int c = blockIdx.x * 64 + threadIdx.x, s0 = (blockIdx.y / ntile) * a.spc, b0 = (blockIdx.y % ntile) * BEAM_TILE;
    const int ns = a.nout - s0 < a.spc ? a.nout - s0 : a.spc;
    const int R = a.R, tscr = a.tscr, nrows = ns * tscr;
    const size_t pol_stride = (size_t)R * PB_NCHANOUT, seg_stride = 2 * pol_stride, ant_stride = (size_t)a.S * seg_stride;
    const int r0 = a.shift[c] + s0 * tscr;

    // The tile's weights, held as pairs of beams (wr of beams 2j and 2j + 1, wi likewise): the arithmetic below is
    // elementwise on such pairs.  A tile's beams past nbeam repeat the last beam (computed, never stored): no address
    // leaves the table.
    beam_pair wr[BEAM_TILE / 2][NPW][NA], wi[BEAM_TILE / 2][NPW][NA];
#pragma unroll
    for (int j = 0; j < BEAM_TILE / 2; ++j) {
        const int last = a.nbeam - 1;
        const int be = b0 + 2 * j < last ? b0 + 2 * j : last, bo = b0 + 2 * j + 1 < last ? b0 + 2 * j + 1 : last;
#pragma unroll
        for (int p = 0; p < NPW; ++p)
#pragma unroll
            for (int l = 0; l < NA; ++l) {
                const float2 we = a.W[((size_t)(be * NPW + p) * NA + l) * PB_NCHANOUT + c];
                const float2 wo = a.W[((size_t)(bo * NPW + p) * NA + l) * PB_NCHANOUT + c];
                wr[j][p][l] = beam_pair{we.x, wo.x};
                wi[j][p][l] = beam_pair{we.y, wo.y};
            }
    }

    const float2 *xp = a.X + c;
    // the loader's position: row k of the run, as (row within its segment, offset of that row in an antenna's plane)
    int kload = 0, row = r0 % R;
    size_t off = (size_t)(r0 / R) * seg_stride + (size_t)row * PB_NCHANOUT;

    // one buffer of U rows: a slot is reloaded with the row U further on as soon as its row has been added, so the loads
    // of the other U - 1 rows are in flight while one row is added
    float2 buf[U][NA][2];
    auto request = [&](int u) {
#pragma unroll
        for (int l = 0; l < NA; ++l) {
            buf[u][l][0] = xp[(size_t)l * ant_stride + off];
            buf[u][l][1] = xp[(size_t)l * ant_stride + off + pol_stride];
        }
        // rows past the run's end repeat its last row (loaded, never added): no address leaves the windows
        if (kload < nrows - 1) {
            ++kload;
            ++row;
            off += PB_NCHANOUT;
            if (row == R) {
                row = 0;
                off += seg_stride - pol_stride;
            }
        }
    };

    beam_pair acc[BEAM_TILE / 2][4];
#pragma unroll
    for (int j = 0; j < BEAM_TILE / 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[j][q] = beam_pair{0.f, 0.f};
    int kin = 0, s = s0;          // rows added to the current output sample; the sample

#pragma unroll
    for (int u = 0; u < U; ++u) request(u);
    for (int kb = 0; kb < nrows; kb += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kb + u < nrows) {
#pragma unroll
                for (int j = 0; j < BEAM_TILE / 2; ++j) {
                    // the beam voltage of both pols (include/pb_hip.h) for two beams at once, pol p with its own weights
                    // where it has them: antennas ascending, one operation per line and element
                    beam_pair yr[2], yi[2];
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
                        const int pw = NPW == 2 ? p : 0;
                        yr[p] = beam_pair{0.f, 0.f};
                        yi[p] = beam_pair{0.f, 0.f};
#pragma unroll
                        for (int l = 0; l < NA; ++l) {
                            const beam_pair xr = buf[u][l][p].x, xi = buf[u][l][p].y;      // both beams see the same value
                            const beam_pair rr = xr * wr[j][pw][l], ii = xi * wi[j][pw][l];
                            const beam_pair tr = rr - ii;
                            const beam_pair ir = xi * wr[j][pw][l], ri = xr * wi[j][pw][l];
                            const beam_pair ti = ir + ri;
                            yr[p] = yr[p] + tr;
                            yi[p] = yi[p] + ti;
                        }
                    }
                    // detection: the correlator's term lines, AA BB CR CI
                    const beam_pair ar = yr[0], ai = yi[0], br = yr[1], bi = yi[1];
                    const beam_pair arar = ar * ar, aiai = ai * ai;
                    const beam_pair aa = arar + aiai;
                    const beam_pair brbr = br * br, bibi = bi * bi;
                    const beam_pair bb = brbr + bibi;
                    const beam_pair arbr = ar * br, aibi = ai * bi;
                    const beam_pair cr = arbr + aibi;
                    const beam_pair aibr = ai * br, arbi = ar * bi;
                    const beam_pair ci = aibr - arbi;
                    acc[j][0] = acc[j][0] + aa;
                    acc[j][1] = acc[j][1] + bb;
                    acc[j][2] = acc[j][2] + cr;
                    acc[j][3] = acc[j][3] + ci;
                }
                if (++kin == tscr) {
                    // the window is complete (the same row in every lane): store the sample and start the next.  Its
                    // rows that count: per beam with one set of weights, one figure for the call with two
                    const int rs = r0 + (s - s0) * tscr;
                    int nwin = tscr;
                    if constexpr (NPW == 2) {
                        if (a.used && a.pref) nwin = a.pref[rs + tscr] - a.pref[rs];
                    }
#pragma unroll
                    for (int i = 0; i < BEAM_TILE; ++i) {
                        if (b0 + i < a.nbeam) {
                            const size_t o = (size_t)(b0 + i) * a.nout + s;
                            if (a.beams) {
#pragma unroll
                                for (int q = 0; q < 4; ++q) a.beams[(o * 4 + q) * PB_NCHANOUT + c] = (i & 1) ? acc[i / 2][q].y : acc[i / 2][q].x;
                            }
                            if (a.used) {
                                int n = nwin;
                                if constexpr (NPW == 1) {
                                    if (a.pref) {
                                        const int32_t *P = a.pref + (size_t)(b0 + i) * (a.T + 1);
                                        n = P[rs + tscr] - P[rs];
                                    }
                                }
                                a.used[o * PB_NCHANOUT + c] = n;
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < BEAM_TILE / 2; ++j)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[j][q] = beam_pair{0.f, 0.f};
                    kin = 0;
                    ++s;
                }
                if (kb + u + U < nrows) request(u);
            }
        }
    }
}

template <int NA>
__global__ __launch_bounds__(64) void k_beamform(BeamArgs a) { beam_walk<NA, 1>(a); }

template <int NA>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_beamform_proj(BeamArgs a) { beam_walk<NA, 2>(a); }

template <int NA> static void beam_launch(bool proj, const BeamArgs &a, hipStream_t st)
{
    const int nchunk = (a.nout + a.spc - 1) / a.spc, ntile = (a.nbeam + BEAM_TILE - 1) / BEAM_TILE;
    const dim3 grid(PB_NCHANOUT / 64, nchunk * ntile);      // at most 32768 rows of workgroups (the 2 GiB limit: nbeam nout <= 32768)
    if (proj) k_beamform_proj<NA><<<grid, 64, 0, st>>>(a);
    else k_beamform<NA><<<grid, 64, 0, st>>>(a);
}

template <int NA> static void beamproj_weights_launch(int nbeam, const double *par, const float *gain, const float2 *proj, float2 *W,
                                                      hipStream_t st)
{
    k_beamproj_weights<NA><<<dim3(PB_NCHANOUT / 64, nbeam), 64, 0, st>>>(par, par + nbeam * NA, gain, proj, W);
}

// the instantiation for the handle's antennas
#define BEAM_ANY(A, fn, ...)                   \
    switch (A) {                               \
    case 1: fn<1>(__VA_ARGS__); break;         \
    case 2: fn<2>(__VA_ARGS__); break;         \
    case 3: fn<3>(__VA_ARGS__); break;         \
    case 4: fn<4>(__VA_ARGS__); break;         \
    case 5: fn<5>(__VA_ARGS__); break;         \
    case 6: fn<6>(__VA_ARGS__); break;         \
    case 7: fn<7>(__VA_ARGS__); break;         \
    default: fn<8>(__VA_ARGS__); break;        \
    }

void pb_beamform_free(pb_handle *h)
{
    job_free(h->beam);
    job_free(h->beamproj);
}

// What both calls refuse, under the name w: everything refused is refused here, on the host, before anything is queued.
// The plain call has no matrices to check; past the refusals, c.proj != nullptr is the projecting call.
int beam_check(pb_handle *h, const std::string &w, bool projecting, BeamCall &c)
{
    if (int rc = spectra_check_config(h, w, c.stream, c.nseg)) return rc;
    if (c.tscr < 1 || c.nout < 1) return fail(h, PB_EINVAL, w + ": tscr and nout must be positive");
    if (c.nbeam < 1 || c.nbeam > BEAM_MAX_BEAMS) return fail(h, PB_EINVAL, w + ": nbeam must be 1..64");
    c.nused = (size_t)c.nbeam * c.nout * PB_NCHANOUT;
    c.nval = c.nused * 4;
    if (!job_output_fits(c.nval * sizeof(float))) return fail(h, PB_EINVAL, w + ": outputs beyond 2 GiB; use fewer beams or samples per call");
    if (!c.delay) return fail(h, PB_EINVAL, w + ": delay is null");
    if (projecting && !c.proj) return fail(h, PB_EINVAL, w + ": proj is null");
    const int A = h->A, n = c.nbeam * A;
    for (int k = 0; k < n; ++k) {
        if (!delay_ok(c.delay[k])) return fail(h, PB_EINVAL, w + ": a delay is not finite or beyond 2^24 samples");
        if (c.psi && !std::isfinite(c.psi[k])) return fail(h, PB_EINVAL, w + ": a psi is not finite");
        if (c.gain && !std::isfinite(c.gain[k])) return fail(h, PB_EINVAL, w + ": a gain is not finite");
    }
    int max_shift = 0;
    if (c.shift)
        for (int k = 0; k < PB_NCHANOUT; ++k) {
            if (c.shift[k] < 0) return fail(h, PB_EINVAL, w + ": a shift is negative");
            if (c.shift[k] > max_shift) max_shift = c.shift[k];
        }
    c.nproj = c.proj ? (size_t)2 * A * A * PB_NCHANOUT : 0;
    for (size_t k = 0; k < 2 * c.nproj; ++k)
        if (!std::isfinite(c.proj[k])) return fail(h, PB_EINVAL, w + ": a proj value is not finite");
    if (int rc = spectra_check_batch(h, w, c.nseg)) return rc;
    c.T = c.nseg * h->R;
    if ((int64_t)max_shift + (int64_t)c.nout * c.tscr > c.T) return fail(h, PB_EINVAL, w + ": a window leaves the batch's rows");
    return PB_OK;
}

// The first part of a checked call, on the call's own state bs: stage, upload, weights, row counts and the beam kernel.
// The plain call has no matrices to stage or upload, one set of weights per beam and a row count per beam.
int beam_queue(pb_handle *h, pb_beam_state *&bs, const BeamCall &c, bool want_beams, bool want_used, const BeamUpload *more)
{
    const int A = h->A, nbeam = c.nbeam, n = nbeam * A, T = c.T;
    const float *proj = c.proj;
    const size_t nproj = c.nproj;
    if (!bs) bs = new pb_beam_state;
    bs->h_par.resize(2 * (size_t)n);
    bs->h_gain.resize(n);
    for (int k = 0; k < n; ++k) {
        bs->h_par[k] = delay_slope(c.delay[k]);
        bs->h_par[n + k] = c.psi ? c.psi[k] : 0.0;
        bs->h_gain[k] = c.gain ? c.gain[k] : 1.0f;
    }
    if (c.shift) bs->h_shift.assign(c.shift, c.shift + PB_NCHANOUT);
    else bs->h_shift.assign(PB_NCHANOUT, 0);

    HIPCHK(h, bs->ensure(h->cfg.device));
    if (proj) {
        // proj [2][4096][A][A] (re, im) -> the device's [2][A][A][4096], in pinned memory (the previous call's upload has
        // finished: every call returns with its stream drained)
        HIPCHK(h, bs->h_proj.grow(nproj));
        for (int p = 0; p < 2; ++p)
            for (int k = 0; k < PB_NCHANOUT; ++k) {
                const float *src = proj + ((size_t)p * PB_NCHANOUT + k) * A * A * 2;
                for (int aj = 0; aj < A * A; ++aj)
                    bs->h_proj.p[((size_t)p * A * A + aj) * PB_NCHANOUT + k] = make_float2(src[2 * aj], src[2 * aj + 1]);
            }
    }
    const bool count = c.stream == PB_CORR_KUR && want_used;      // rows_used of the excised stream: from the row counts
    HIPCHK(h, bs->par.grow(h, (size_t)2 * BEAM_MAX_BEAMS * PB_SPECTRA_MAX_ANT));
    HIPCHK(h, bs->gain.grow(h, (size_t)BEAM_MAX_BEAMS * PB_SPECTRA_MAX_ANT));
    HIPCHK(h, bs->shift.grow(h, (size_t)PB_NCHANOUT));
    if (proj) HIPCHK(h, bs->proj.grow(h, nproj));
    HIPCHK(h, bs->W.grow(h, (size_t)(proj ? 2 : 1) * n * PB_NCHANOUT));
    if (want_beams) HIPCHK(h, bs->beams.grow(h, c.nval));
    if (want_used) HIPCHK(h, bs->used.grow(h, c.nused));
    if (count) HIPCHK(h, bs->pref.grow(h, (size_t)(proj ? 1 : nbeam) * (T + 1)));

    const pb_handle::BufSet &b = h->set();
    // behind the set's channeliser and detect (ev_chan): whatever refills the set is queued by a later call, and this
    // one returns only when its own stream has drained
    HIPCHK(h, hipStreamWaitEvent(bs->st, b.ev_chan.e, 0));
    HIPCHK(h, bs->mark(0));
    HIPCHK(h, bs->par.from_host(bs->h_par.data(), 2 * (size_t)n, bs->st));
    HIPCHK(h, bs->gain.from_host(bs->h_gain.data(), (size_t)n, bs->st));
    HIPCHK(h, bs->shift.from_host(bs->h_shift.data(), PB_NCHANOUT, bs->st));
    if (proj) HIPCHK(h, bs->proj.from_host(bs->h_proj.p, nproj, bs->st));
    if (more) HIPCHK(h, hipMemcpyAsync(more->dst, more->src, more->n * sizeof(float), hipMemcpyHostToDevice, bs->st));
    BeamArgs a;
    a.X = (const float2 *)(c.stream == PB_CORR_KUR ? b.d_Pkur.p : b.d_Praw.p);
    a.W = bs->W.p;
    a.shift = bs->shift.p;
    a.pref = count ? bs->pref.p : nullptr;
    a.beams = want_beams ? bs->beams.p : nullptr;
    a.used = want_used ? bs->used.p : nullptr;
    a.S = h->S;
    a.R = h->R;
    a.T = T;
    a.nbeam = nbeam;
    a.tscr = c.tscr;
    a.nout = c.nout;
    a.spc = c.tscr >= BEAM_CHUNK_ROWS ? 1 : BEAM_CHUNK_ROWS / c.tscr;
    // the plain call's weights go before its row counts, the projecting call's after them
    if (!proj) k_beam_weights<<<dim3(PB_NCHANOUT / 64, n), 64, 0, bs->st>>>(bs->par.p, bs->par.p + n, bs->gain.p, bs->W.p);
    if (count)
        k_beam_prefix<<<proj ? 1 : nbeam, 64, 0, bs->st>>>(b.d_wrow.p, proj ? nullptr : bs->gain.p, A, (size_t)h->S * h->R, T, bs->pref.p);
    if (proj) BEAM_ANY(A, beamproj_weights_launch, nbeam, bs->par.p, bs->gain.p, bs->proj.p, bs->W.p, bs->st)
    HIPCHK(h, bs->launched(1));
    if (want_beams || want_used) BEAM_ANY(A, beam_launch, proj != nullptr, a, bs->st)
    HIPCHK(h, bs->launched(2));
    return PB_OK;
}

// Both calls, under the name w, on the call's own state bs: the first part above, then the copies to the host and the
// wait for them.
static int beam_call(pb_handle *h, const std::string &w, pb_beam_state *&bs, bool projecting, int stream, int nseg, int nbeam,
                     const double *delay, const double *psi, const float *gain, const float *proj, const int32_t *shift,
                     int tscr, int nout, float *beams, int32_t *rows_used)
{
    BeamCall c = {stream, nseg, nbeam, delay, psi, gain, proj, shift, tscr, nout, 0, 0, 0, 0};
    if (int rc = beam_check(h, w, projecting, c)) return rc;
    if (int rc = beam_queue(h, bs, c, beams != nullptr, rows_used != nullptr, nullptr)) return rc;
    HIPCHK(h, bs->beams.to_host(beams, c.nval, bs->st));
    HIPCHK(h, bs->used.to_host(rows_used, c.nused, bs->st));
    HIPCHK(h, bs->finish());
    return PB_OK;
}

static int beam_timers(const pb_handle *h, const pb_beam_state *bs, float *ms3)
{
    if (!h || !ms3) return PB_EINVAL;
    for (int k = 0; k < 3; ++k) ms3[k] = bs ? bs->ms[k] : 0.f;
    return PB_OK;
}

extern "C" int pb_beamform(pb_handle *h, int stream, int nseg, int nbeam, const double *delay, const double *psi,
                           const float *gain, const int32_t *shift, int tscr, int nout, float *beams, int32_t *rows_used)
{
    if (!h) return PB_EINVAL;
    return beam_call(h, "pb_beamform", h->beam, false, stream, nseg, nbeam, delay, psi, gain, nullptr, shift, tscr, nout, beams, rows_used);
}

extern "C" int pb_beamform_proj(pb_handle *h, int stream, int nseg, int nbeam, const double *delay, const double *psi,
                                const float *gain, const float *proj, const int32_t *shift, int tscr, int nout, float *beams,
                                int32_t *rows_used)
{
    if (!h) return PB_EINVAL;
    return beam_call(h, "pb_beamform_proj", h->beamproj, true, stream, nseg, nbeam, delay, psi, gain, proj, shift, tscr, nout, beams,
                     rows_used);
}

extern "C" int pb_beamform_timers(const pb_handle *h, float *ms3) { return beam_timers(h, h ? h->beam : nullptr, ms3); }

extern "C" int pb_beamform_proj_timers(const pb_handle *h, float *ms3) { return beam_timers(h, h ? h->beamproj : nullptr, ms3); }
