// The beamformer (include/pb_hip.h: pb_beamform): per beam a weighted, phase-rotated sum of a handle's antennas per
// (pol, row, channel), detected into the four coherence products and added over windows of tscr rows -- from the complex
// in-band spectra that the coherence channeliser leaves in HBM (BufSet::d_Praw / d_Pkur, float2 [A][S][2][R][4096]).
// The sum over a window's rows is in row order, so a lane walks its channel's rows alone and the parallelism is
// channels x runs of output samples x beam tiles.
//
// k_beam_weights: W[b][a][c] = gain * (cr, sr), the header's binary64 phase and binary32 rotation polynomial; once per
//   call, one lane per value.
// k_beam_prefix: per beam the running count of rows whose weight is > 0 for every antenna of non-zero gain (one wave,
//   ballots), so that rows_used of the excised stream is a difference of two entries.
// k_beamform<NA>: one 64-lane workgroup = 64 channels, a run of output samples (about BEAM_CHUNK_ROWS rows) and a tile of
//   BEAM_TILE beams; a lane owns one channel and keeps the tile's weights (2 NA BEAM_TILE floats) and its 4 BEAM_TILE
//   accumulators in registers, as pairs of beams: the definition's lines are written once on two-element vectors (beams
//   2j and 2j + 1), which the compiler turns into packed binary32 multiplies and adds without keeping a weight twice.
//   Every spectrum value is loaded once per workgroup and serves all beams of the tile; the
//   lane holds U rows and reloads a row's slot as soon as the row is added, so U - 1 rows' loads are in flight.  The
//   windows of a run follow one another without a gap, so the lane walks one stretch of rows and stores and clears its
//   accumulators every tscr rows.  A channel's stretch differs from its neighbours' only in its first row (shift): the
//   addresses are coalesced over the channels whenever neighbouring shifts are equal and correct when they are not.
//   No LDS, no atomics, no scratch.
// Host side: pb_beam_state is a job of csrc/pb_job.h (stream, stage events and times, owned buffers that grow, teardown),
// and what the call refuses about the handle, the stream and the batch is that header's spectra_check_*.
#include "pb_job.h"
#include "rotation_dev.h"

#define BEAM_MAX_BEAMS 64
#define BEAM_TILE 4             // beams of a workgroup
#define BEAM_CHUNK_ROWS 32      // rows of a workgroup's run: max(1, BEAM_CHUNK_ROWS / tscr) output samples

struct BeamArgs {
    const float2 *X;       // one stream's spectra [A][S][2][R][4096]
    const float2 *W;       // [nbeam][A][4096] weights
    const int32_t *shift;  // [4096] first row of output sample 0 per channel
    const int32_t *pref;   // [nbeam][T + 1] rows before t that count for the beam; nullptr on the raw stream
    float *beams;          // [nbeam][nout][4][4096]
    int32_t *used;         // [nbeam][nout][4096]
    int S, R, T, nbeam, tscr, nout, spc;   // spc: output samples per workgroup
};

struct PB_LOCAL pb_beam_state : PbJob<3> {      // stages: uploads + weights + row counts, beam kernel, copy to the host
    DevBuf<double> par;                  // [2][BEAM_MAX_BEAMS * PB_SPECTRA_MAX_ANT]: delay / 12500, psi
    DevBuf<float> gain;                  // [BEAM_MAX_BEAMS * PB_SPECTRA_MAX_ANT]
    DevBuf<int32_t> shift;               // [4096]
    DevBuf<float2> W;
    DevBuf<float> beams;
    DevBuf<int32_t> used, pref;
    std::vector<double> h_par;
    std::vector<float> h_gain;
    std::vector<int32_t> h_shift;
};

typedef float beam_pair __attribute__((ext_vector_type(2)));      // one value for each of two beams

namespace {

// rows of the lane's buffer: about 32 8-byte loads per lane
constexpr int beam_rows_in_flight(int na) { return na == 1 ? 16 : na == 2 ? 8 : na == 3 ? 5 : na == 4 ? 4 : na <= 6 ? 3 : 2; }

}  // namespace

__global__ __launch_bounds__(64) void k_beam_weights(const double *q, const double *psi, const float *gain, float2 *W)
{
    const int c = blockIdx.x * 64 + threadIdx.x, ba = blockIdx.y;
    // the phase (include/pb_hip.h): binary64, every operation rounded once
    const double k = (double)(PB_CHANMIN + c);
    const double kq = k * q[ba];
    const double t = psi[ba] + kq;
    const double r64 = t - rint(t);
    float cr, sr;
    img_rotation((float)r64, cr, sr);
    const float g = gain[ba];
    W[(size_t)ba * PB_NCHANOUT + c] = make_float2(g * cr, g * sr);
}

// pref[b][t] = the number of rows before t whose weight is > 0 for every antenna with gain[b][a] != 0, t = 0 .. T
__global__ __launch_bounds__(64) void k_beam_prefix(const float *wrow, const float *gain, int A, size_t ant_stride, int T,
                                                    int32_t *pref)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const float *g = gain + (size_t)b * A;
    int32_t *P = pref + (size_t)b * (T + 1);
    int total = 0;
    if (lane == 0) P[0] = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        bool ok = t < T;
        if (ok)
            for (int a = 0; a < A; ++a)
                if (g[a] != 0.f && !(wrow[(size_t)a * ant_stride + t] > 0.f)) ok = false;
        const unsigned long long m = __ballot(ok);
        if (t < T) P[t + 1] = total + __popcll(m & (~0ull >> (63 - lane)));
        total += __popcll(m);
    }
}

template <int NA>
__global__ __launch_bounds__(64) void k_beamform(BeamArgs a)
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
    beam_pair wr[BEAM_TILE / 2][NA], wi[BEAM_TILE / 2][NA];
#pragma unroll
    for (int j = 0; j < BEAM_TILE / 2; ++j) {
        const int last = a.nbeam - 1;
        const int be = b0 + 2 * j < last ? b0 + 2 * j : last, bo = b0 + 2 * j + 1 < last ? b0 + 2 * j + 1 : last;
#pragma unroll
        for (int l = 0; l < NA; ++l) {
            const float2 we = a.W[((size_t)be * NA + l) * PB_NCHANOUT + c];
            const float2 wo = a.W[((size_t)bo * NA + l) * PB_NCHANOUT + c];
            wr[j][l] = beam_pair{we.x, wo.x};
            wi[j][l] = beam_pair{we.y, wo.y};
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
                    // the beam voltage of both pols (include/pb_hip.h) for two beams at once: antennas ascending, one
                    // operation per line and element
                    beam_pair yr[2], yi[2];
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
                        yr[p] = beam_pair{0.f, 0.f};
                        yi[p] = beam_pair{0.f, 0.f};
#pragma unroll
                        for (int l = 0; l < NA; ++l) {
                            const beam_pair xr = buf[u][l][p].x, xi = buf[u][l][p].y;      // both beams see the same value
                            const beam_pair rr = xr * wr[j][l], ii = xi * wi[j][l];
                            const beam_pair tr = rr - ii;
                            const beam_pair ir = xi * wr[j][l], ri = xr * wi[j][l];
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
                    // the window is complete (the same row in every lane): store the sample and start the next
#pragma unroll
                    for (int i = 0; i < BEAM_TILE; ++i) {
                        if (b0 + i < a.nbeam) {
                            const size_t o = (size_t)(b0 + i) * a.nout + s;
                            if (a.beams) {
#pragma unroll
                                for (int q = 0; q < 4; ++q) a.beams[(o * 4 + q) * PB_NCHANOUT + c] = (i & 1) ? acc[i / 2][q].y : acc[i / 2][q].x;
                            }
                            if (a.used) {
                                int n = tscr;
                                if (a.pref) {
                                    const int32_t *P = a.pref + (size_t)(b0 + i) * (a.T + 1);
                                    const int rs = r0 + (s - s0) * tscr;
                                    n = P[rs + tscr] - P[rs];
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

template <int NA> static void beam_launch(const BeamArgs &a, hipStream_t st)
{
    const int nchunk = (a.nout + a.spc - 1) / a.spc, ntile = (a.nbeam + BEAM_TILE - 1) / BEAM_TILE;
    k_beamform<NA><<<dim3(PB_NCHANOUT / 64, nchunk * ntile), 64, 0, st>>>(a);      // at most 40960 rows of workgroups (the 2 GiB limit)
}

static void beam_launch_any(int A, const BeamArgs &a, hipStream_t st)
{
    switch (A) {
    case 1: beam_launch<1>(a, st); break;
    case 2: beam_launch<2>(a, st); break;
    case 3: beam_launch<3>(a, st); break;
    case 4: beam_launch<4>(a, st); break;
    case 5: beam_launch<5>(a, st); break;
    case 6: beam_launch<6>(a, st); break;
    case 7: beam_launch<7>(a, st); break;
    default: beam_launch<8>(a, st); break;
    }
}

void pb_beamform_free(pb_handle *h) { job_free(h->beam); }

extern "C" int pb_beamform(pb_handle *h, int stream, int nseg, int nbeam, const double *delay, const double *psi,
                           const float *gain, const int32_t *shift, int tscr, int nout, float *beams, int32_t *rows_used)
{
    if (!h) return PB_EINVAL;
    // everything refused is refused here, on the host, before anything is queued
    if (int rc = spectra_check_config(h, "pb_beamform", stream, nseg)) return rc;
    if (tscr < 1 || nout < 1) return fail(h, PB_EINVAL, "pb_beamform: tscr and nout must be positive");
    if (nbeam < 1 || nbeam > BEAM_MAX_BEAMS) return fail(h, PB_EINVAL, "pb_beamform: nbeam must be 1..64");
    const size_t nused = (size_t)nbeam * nout * PB_NCHANOUT, nval = nused * 4;
    if (!job_output_fits(nval * sizeof(float))) return fail(h, PB_EINVAL, "pb_beamform: outputs beyond 2 GiB; use fewer beams or samples per call");
    if (!delay) return fail(h, PB_EINVAL, "pb_beamform: delay is null");
    const int A = h->A, n = nbeam * A;
    for (int k = 0; k < n; ++k) {
        if (!delay_ok(delay[k])) return fail(h, PB_EINVAL, "pb_beamform: a delay is not finite or beyond 2^24 samples");
        if (psi && !std::isfinite(psi[k])) return fail(h, PB_EINVAL, "pb_beamform: a psi is not finite");
        if (gain && !std::isfinite(gain[k])) return fail(h, PB_EINVAL, "pb_beamform: a gain is not finite");
    }
    int max_shift = 0;
    if (shift)
        for (int c = 0; c < PB_NCHANOUT; ++c) {
            if (shift[c] < 0) return fail(h, PB_EINVAL, "pb_beamform: a shift is negative");
            if (shift[c] > max_shift) max_shift = shift[c];
        }
    if (int rc = spectra_check_batch(h, "pb_beamform", nseg)) return rc;
    const int T = nseg * h->R;
    if ((int64_t)max_shift + (int64_t)nout * tscr > T) return fail(h, PB_EINVAL, "pb_beamform: a window leaves the batch's rows");

    if (!h->beam) h->beam = new pb_beam_state;
    pb_beam_state *bs = h->beam;
    bs->h_par.resize(2 * (size_t)n);
    bs->h_gain.resize(n);
    for (int k = 0; k < n; ++k) {
        bs->h_par[k] = delay_slope(delay[k]);
        bs->h_par[n + k] = psi ? psi[k] : 0.0;
        bs->h_gain[k] = gain ? gain[k] : 1.0f;
    }
    if (shift) bs->h_shift.assign(shift, shift + PB_NCHANOUT);
    else bs->h_shift.assign(PB_NCHANOUT, 0);

    HIPCHK(h, bs->ensure(h->cfg.device));
    const bool kur = stream == PB_CORR_KUR;
    HIPCHK(h, bs->par.grow(h, (size_t)2 * BEAM_MAX_BEAMS * PB_SPECTRA_MAX_ANT));
    HIPCHK(h, bs->gain.grow(h, (size_t)BEAM_MAX_BEAMS * PB_SPECTRA_MAX_ANT));
    HIPCHK(h, bs->shift.grow(h, (size_t)PB_NCHANOUT));
    HIPCHK(h, bs->W.grow(h, (size_t)n * PB_NCHANOUT));
    if (beams) HIPCHK(h, bs->beams.grow(h, nval));
    if (rows_used) HIPCHK(h, bs->used.grow(h, nused));
    if (kur && rows_used) HIPCHK(h, bs->pref.grow(h, (size_t)nbeam * (T + 1)));

    const pb_handle::BufSet &b = h->set();
    // behind the set's channeliser and detect (ev_chan): whatever refills the set is queued by a later call, and this
    // one returns only when its own stream has drained
    HIPCHK(h, hipStreamWaitEvent(bs->st, b.ev_chan, 0));
    HIPCHK(h, bs->mark(0));
    HIPCHK(h, bs->par.from_host(bs->h_par.data(), 2 * (size_t)n, bs->st));
    HIPCHK(h, bs->gain.from_host(bs->h_gain.data(), (size_t)n, bs->st));
    HIPCHK(h, bs->shift.from_host(bs->h_shift.data(), PB_NCHANOUT, bs->st));
    k_beam_weights<<<dim3(PB_NCHANOUT / 64, n), 64, 0, bs->st>>>(bs->par.p, bs->par.p + n, bs->gain.p, bs->W.p);
    BeamArgs a;
    a.X = (const float2 *)(kur ? b.d_Pkur : b.d_Praw);
    a.W = bs->W.p;
    a.shift = bs->shift.p;
    a.pref = nullptr;
    a.beams = beams ? bs->beams.p : nullptr;
    a.used = rows_used ? bs->used.p : nullptr;
    a.S = h->S;
    a.R = h->R;
    a.T = T;
    a.nbeam = nbeam;
    a.tscr = tscr;
    a.nout = nout;
    a.spc = tscr >= BEAM_CHUNK_ROWS ? 1 : BEAM_CHUNK_ROWS / tscr;
    if (kur && rows_used) {
        k_beam_prefix<<<nbeam, 64, 0, bs->st>>>(b.d_wrow, bs->gain.p, A, (size_t)h->S * h->R, T, bs->pref.p);
        a.pref = bs->pref.p;
    }
    HIPCHK(h, bs->launched(1));
    if (beams || rows_used) beam_launch_any(A, a, bs->st);
    HIPCHK(h, bs->launched(2));
    HIPCHK(h, bs->beams.to_host(beams, nval, bs->st));
    HIPCHK(h, bs->used.to_host(rows_used, nused, bs->st));
    HIPCHK(h, bs->finish());
    return PB_OK;
}

extern "C" int pb_beamform_timers(const pb_handle *h, float *ms3)
{
    if (!h || !ms3) return PB_EINVAL;
    for (int k = 0; k < 3; ++k) ms3[k] = h->beam ? h->beam->ms[k] : 0.f;
    return PB_OK;
}
