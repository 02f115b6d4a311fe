// The projecting beamformer (include/pb_hip.h: pb_beamform_proj): pb_beamform with a weight that is free per (beam, pol,
// antenna, channel) -- the beam's steering weights s[b][a][c] put through a complex matrix proj[p][c] per (pol, channel),
// w'[b][p][j][c] = sum over a of s[b][a][c] proj[p][c][a][j], so that the beam voltage is s^T (P x): per-channel spatial
// nulls (vlite-fast_amd/nulling.py makes P = I - v v^H from the correlator's matrices) or per-pol calibration, then the
// beam.  Voltage, detection and integration are pb_beamform's lines on the same spectra (BufSet::d_Praw / d_Pkur,
// float2 [A][S][2][R][4096]); pol p uses w'[b][p].
//
// k_beamproj_weights<NA>: W'[b][p][j][c], once per call; a lane owns one (b, c), forms the NA steering weights (the
//   header's binary64 phase, the rotation polynomial, the gain) once and keeps them in registers, then walks the 2 NA
//   columns.  proj lies on the device as float2 [2][NA][NA][4096] (pol, row a, column j, channel): the host checks
//   it, transposes it into pinned memory and uploads it from there, and every read is coalesced over the channels.
// k_beamproj_prefix: the running count of rows whose weight is > 0 for EVERY antenna of the handle (a matrix mixes the
//   antennas, so no gain takes one out of the count): one count for the whole call, one wave, ballots.
// k_beamform_proj<NA>: k_beamform's walk -- a 64-lane workgroup = 64 channels, a run of output samples (about
//   BEAMPROJ_CHUNK_ROWS rows) and a tile of BEAMPROJ_TILE beams, the tile's weights and accumulators in registers as
//   pairs of beams, U rows in flight, every spectrum value loaded once per workgroup -- with the weights of both pols:
//   16 NA floats, twice pb_beamform's.  The tile stays four beams at every antenna count: a tile of two above four
//   antennas compiled to fewer registers but read the spectra twice as often and was slower wherever it was measured
//   (eight antennas: 1.35 against 1.08 ms for four beams, 3.95 against 2.75 ms for sixteen).  The kernel asks for two
//   waves per SIMD (amdgpu_waves_per_eu), which at eight antennas makes the compiler fit 250 VGPRs where it otherwise
//   took 256 and 4 AGPRs and one wave (sixteen beams: 3.42 ms).  No LDS, no atomics, no scratch.
// pb_beamform.hip's list of kernels is pinned by its resource test, and the pieces the two files have in common are a
// few lines each: they are restated here, and that file is as it was.
// Host side: pb_beamproj_state is a job of csrc/pb_job.h, and what the call refuses about the handle, the stream and the
// batch is that header's spectra_check_*.
#include "pb_job.h"
#include "rotation_dev.h"

#include <vector>

#define BEAMPROJ_MAX_BEAMS 64
#define BEAMPROJ_TILE 4             // beams of a workgroup
#define BEAMPROJ_CHUNK_ROWS 32      // rows of a workgroup's run: max(1, BEAMPROJ_CHUNK_ROWS / tscr) output samples

struct BeamProjArgs {
    const float2 *X;       // one stream's spectra [A][S][2][R][4096]
    const float2 *W;       // [nbeam][2][A][4096] projected weights
    const int32_t *shift;  // [4096] first row of output sample 0 per channel
    const int32_t *pref;   // [T + 1] rows before t that count; nullptr on the raw stream
    float *beams;          // [nbeam][nout][4][4096]
    int32_t *used;         // [nbeam][nout][4096]
    int S, R, T, nbeam, tscr, nout, spc;   // spc: output samples per workgroup
};

// pinned host memory that is freed with the struct it is a member of: the matrices go to the device from here, so that
// their upload is a DMA transfer that does not wait for the host
struct PB_LOCAL PinnedProj {
    float2 *p = nullptr;
    size_t cap = 0;      // elements
    PinnedProj() = default;
    PinnedProj(PinnedProj &&) = delete;
    ~PinnedProj() { if (p) (void)hipHostFree(p); }
    hipError_t grow(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc((void **)&p, n * sizeof(float2), hipHostMallocDefault);
        if (e == hipSuccess) cap = n;
        return e;
    }
};

struct PB_LOCAL pb_beamproj_state : PbJob<3> {  // stages: uploads + weights + row counts, beam kernel, copy to the host
    DevBuf<double> par;                  // [2][BEAMPROJ_MAX_BEAMS * PB_SPECTRA_MAX_ANT]: delay / 12500, psi
    DevBuf<float> gain;                  // [BEAMPROJ_MAX_BEAMS * PB_SPECTRA_MAX_ANT]
    DevBuf<int32_t> shift;               // [4096]
    DevBuf<float2> proj;                 // [2][A][A][4096]
    DevBuf<float2> W;
    DevBuf<float> beams;
    DevBuf<int32_t> used, pref;
    std::vector<double> h_par;
    std::vector<float> h_gain;
    std::vector<int32_t> h_shift;
    PinnedProj h_proj;                   // [2][A][A][4096], the device's layout
};

typedef float beamproj_pair __attribute__((ext_vector_type(2)));      // one value for each of two beams

namespace {

// rows of the lane's buffer: about 32 8-byte loads per lane
constexpr int beamproj_rows_in_flight(int na) { return na == 1 ? 16 : na == 2 ? 8 : na == 3 ? 5 : na == 4 ? 4 : na <= 6 ? 3 : 2; }

}  // namespace

template <int NA>
__global__ __launch_bounds__(64) void k_beamproj_weights(const double *q, const double *psi, const float *gain,
                                                         const float2 *proj, float2 *W)
{
    const int c = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    // the steering weights of (b, c): pb_beamform's, the phase in binary64 with every operation rounded once
    float sr[NA], si[NA];
    const double k = (double)(PB_CHANMIN + c);
#pragma unroll
    for (int l = 0; l < NA; ++l) {
        const double kq = k * q[b * NA + l];
        const double t = psi[b * NA + l] + kq;
        const double r64 = t - rint(t);
        float cr, sn;
        img_rotation((float)r64, cr, sn);
        const float g = gain[b * NA + l];
        sr[l] = g * cr;
        si[l] = g * sn;
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

// pref[t] = the number of rows before t whose weight is > 0 for every antenna, t = 0 .. T
__global__ __launch_bounds__(64) void k_beamproj_prefix(const float *wrow, int A, size_t ant_stride, int T, int32_t *pref)
{
    const int lane = threadIdx.x;
    int total = 0;
    if (lane == 0) pref[0] = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        bool ok = t < T;
        if (ok)
            for (int a = 0; a < A; ++a)
                if (!(wrow[(size_t)a * ant_stride + t] > 0.f)) ok = false;
        const unsigned long long m = __ballot(ok);
        if (t < T) pref[t + 1] = total + __popcll(m & (~0ull >> (63 - lane)));
        total += __popcll(m);
    }
}

template <int NA>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_beamform_proj(BeamProjArgs a)
{
    constexpr int TILE = BEAMPROJ_TILE;
    constexpr int U = beamproj_rows_in_flight(NA);
    // the beam tiles of one run of rows are neighbours in blockIdx.y: they run at about the same time, 64 workgroups
    // apart (so on the same XCD), and all but the first can find the run's spectra in the L2
    const int ntile = (a.nbeam + TILE - 1) / TILE;
    const int c = blockIdx.x * 64 + threadIdx.x, s0 = (blockIdx.y / ntile) * a.spc, b0 = (blockIdx.y % ntile) * TILE;
    const int ns = a.nout - s0 < a.spc ? a.nout - s0 : a.spc;
    const int R = a.R, tscr = a.tscr, nrows = ns * tscr;
    const size_t pol_stride = (size_t)R * PB_NCHANOUT, seg_stride = 2 * pol_stride, ant_stride = (size_t)a.S * seg_stride;
    const int r0 = a.shift[c] + s0 * tscr;

    // The tile's weights of both pols, held as pairs of beams (wr of beams 2j and 2j + 1, wi likewise).  A tile's beams
    // past nbeam repeat the last beam (computed, never stored): no address leaves the table.
    beamproj_pair wr[TILE / 2][2][NA], wi[TILE / 2][2][NA];
#pragma unroll
    for (int j = 0; j < TILE / 2; ++j) {
        const int last = a.nbeam - 1;
        const int be = b0 + 2 * j < last ? b0 + 2 * j : last, bo = b0 + 2 * j + 1 < last ? b0 + 2 * j + 1 : last;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int l = 0; l < NA; ++l) {
                const float2 we = a.W[((size_t)(be * 2 + p) * NA + l) * PB_NCHANOUT + c];
                const float2 wo = a.W[((size_t)(bo * 2 + p) * NA + l) * PB_NCHANOUT + c];
                wr[j][p][l] = beamproj_pair{we.x, wo.x};
                wi[j][p][l] = beamproj_pair{we.y, wo.y};
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

    beamproj_pair acc[TILE / 2][4];
#pragma unroll
    for (int j = 0; j < TILE / 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[j][q] = beamproj_pair{0.f, 0.f};
    int kin = 0, s = s0;          // rows added to the current output sample; the sample

#pragma unroll
    for (int u = 0; u < U; ++u) request(u);
    for (int kb = 0; kb < nrows; kb += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kb + u < nrows) {
#pragma unroll
                for (int j = 0; j < TILE / 2; ++j) {
                    // the beam voltage of both pols (include/pb_hip.h) for two beams at once, pol p with its own
                    // weights: antennas ascending, one operation per line and element
                    beamproj_pair yr[2], yi[2];
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
                        yr[p] = beamproj_pair{0.f, 0.f};
                        yi[p] = beamproj_pair{0.f, 0.f};
#pragma unroll
                        for (int l = 0; l < NA; ++l) {
                            const beamproj_pair xr = buf[u][l][p].x, xi = buf[u][l][p].y;      // both beams see the same value
                            const beamproj_pair rr = xr * wr[j][p][l], ii = xi * wi[j][p][l];
                            const beamproj_pair tr = rr - ii;
                            const beamproj_pair ir = xi * wr[j][p][l], ri = xr * wi[j][p][l];
                            const beamproj_pair ti = ir + ri;
                            yr[p] = yr[p] + tr;
                            yi[p] = yi[p] + ti;
                        }
                    }
                    // detection: the correlator's term lines, AA BB CR CI
                    const beamproj_pair ar = yr[0], ai = yi[0], br = yr[1], bi = yi[1];
                    const beamproj_pair arar = ar * ar, aiai = ai * ai;
                    const beamproj_pair aa = arar + aiai;
                    const beamproj_pair brbr = br * br, bibi = bi * bi;
                    const beamproj_pair bb = brbr + bibi;
                    const beamproj_pair arbr = ar * br, aibi = ai * bi;
                    const beamproj_pair cr = arbr + aibi;
                    const beamproj_pair aibr = ai * br, arbi = ar * bi;
                    const beamproj_pair ci = aibr - arbi;
                    acc[j][0] = acc[j][0] + aa;
                    acc[j][1] = acc[j][1] + bb;
                    acc[j][2] = acc[j][2] + cr;
                    acc[j][3] = acc[j][3] + ci;
                }
                if (++kin == tscr) {
                    // the window is complete (the same row in every lane): store the sample and start the next
                    int n = tscr;
                    if (a.used && a.pref) {
                        const int rs = r0 + (s - s0) * tscr;
                        n = a.pref[rs + tscr] - a.pref[rs];
                    }
#pragma unroll
                    for (int i = 0; i < TILE; ++i) {
                        if (b0 + i < a.nbeam) {
                            const size_t o = (size_t)(b0 + i) * a.nout + s;
                            if (a.beams) {
#pragma unroll
                                for (int q = 0; q < 4; ++q) a.beams[(o * 4 + q) * PB_NCHANOUT + c] = (i & 1) ? acc[i / 2][q].y : acc[i / 2][q].x;
                            }
                            if (a.used) a.used[o * PB_NCHANOUT + c] = n;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < TILE / 2; ++j)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[j][q] = beamproj_pair{0.f, 0.f};
                    kin = 0;
                    ++s;
                }
                if (kb + u + U < nrows) request(u);
            }
        }
    }
}

template <int NA> static void beamproj_weights_launch(int nbeam, const double *par, const float *gain, const float2 *proj, float2 *W,
                                                      hipStream_t st)
{
    k_beamproj_weights<NA><<<dim3(PB_NCHANOUT / 64, nbeam), 64, 0, st>>>(par, par + nbeam * NA, gain, proj, W);
}

template <int NA> static void beamproj_launch(const BeamProjArgs &a, hipStream_t st)
{
    constexpr int TILE = BEAMPROJ_TILE;
    const int nchunk = (a.nout + a.spc - 1) / a.spc, ntile = (a.nbeam + TILE - 1) / TILE;
    // at most 32768 rows of workgroups (the 2 GiB limit: nbeam nout <= 32768)
    k_beamform_proj<NA><<<dim3(PB_NCHANOUT / 64, nchunk * ntile), 64, 0, st>>>(a);
}

// the instantiation for the handle's antennas
#define BEAMPROJ_ANY(A, fn, ...)               \
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

void pb_beamproj_free(pb_handle *h) { job_free(h->beamproj); }

extern "C" int pb_beamform_proj(pb_handle *h, int stream, int nseg, int nbeam, const double *delay, const double *psi,
                                const float *gain, const float *proj, const int32_t *shift, int tscr, int nout, float *beams,
                                int32_t *rows_used)
{
    if (!h) return PB_EINVAL;
    // everything refused is refused here, on the host, before anything is queued
    if (int rc = spectra_check_config(h, "pb_beamform_proj", stream, nseg)) return rc;
    if (tscr < 1 || nout < 1) return fail(h, PB_EINVAL, "pb_beamform_proj: tscr and nout must be positive");
    if (nbeam < 1 || nbeam > BEAMPROJ_MAX_BEAMS) return fail(h, PB_EINVAL, "pb_beamform_proj: nbeam must be 1..64");
    const size_t nused = (size_t)nbeam * nout * PB_NCHANOUT, nval = nused * 4;
    if (!job_output_fits(nval * sizeof(float)))
        return fail(h, PB_EINVAL, "pb_beamform_proj: outputs beyond 2 GiB; use fewer beams or samples per call");
    if (!delay) return fail(h, PB_EINVAL, "pb_beamform_proj: delay is null");
    if (!proj) return fail(h, PB_EINVAL, "pb_beamform_proj: proj is null");
    const int A = h->A, n = nbeam * A;
    for (int k = 0; k < n; ++k) {
        if (!delay_ok(delay[k])) return fail(h, PB_EINVAL, "pb_beamform_proj: a delay is not finite or beyond 2^24 samples");
        if (psi && !std::isfinite(psi[k])) return fail(h, PB_EINVAL, "pb_beamform_proj: a psi is not finite");
        if (gain && !std::isfinite(gain[k])) return fail(h, PB_EINVAL, "pb_beamform_proj: a gain is not finite");
    }
    int max_shift = 0;
    if (shift)
        for (int c = 0; c < PB_NCHANOUT; ++c) {
            if (shift[c] < 0) return fail(h, PB_EINVAL, "pb_beamform_proj: a shift is negative");
            if (shift[c] > max_shift) max_shift = shift[c];
        }
    const size_t nproj = (size_t)2 * A * A * PB_NCHANOUT;
    for (size_t k = 0; k < 2 * nproj; ++k)
        if (!std::isfinite(proj[k])) return fail(h, PB_EINVAL, "pb_beamform_proj: a proj value is not finite");
    if (int rc = spectra_check_batch(h, "pb_beamform_proj", nseg)) return rc;
    const int T = nseg * h->R;
    if ((int64_t)max_shift + (int64_t)nout * tscr > T) return fail(h, PB_EINVAL, "pb_beamform_proj: a window leaves the batch's rows");

    if (!h->beamproj) h->beamproj = new pb_beamproj_state;
    pb_beamproj_state *bs = h->beamproj;
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
    // proj [2][4096][A][A] (re, im) -> the device's [2][A][A][4096], in pinned memory (the previous call's upload has
    // finished: every call returns with its stream drained)
    HIPCHK(h, bs->h_proj.grow(nproj));
    for (int p = 0; p < 2; ++p)
        for (int c = 0; c < PB_NCHANOUT; ++c) {
            const float *src = proj + ((size_t)p * PB_NCHANOUT + c) * A * A * 2;
            for (int aj = 0; aj < A * A; ++aj)
                bs->h_proj.p[((size_t)p * A * A + aj) * PB_NCHANOUT + c] = make_float2(src[2 * aj], src[2 * aj + 1]);
        }
    const bool kur = stream == PB_CORR_KUR;
    HIPCHK(h, bs->par.grow(h, (size_t)2 * BEAMPROJ_MAX_BEAMS * PB_SPECTRA_MAX_ANT));
    HIPCHK(h, bs->gain.grow(h, (size_t)BEAMPROJ_MAX_BEAMS * PB_SPECTRA_MAX_ANT));
    HIPCHK(h, bs->shift.grow(h, (size_t)PB_NCHANOUT));
    HIPCHK(h, bs->proj.grow(h, nproj));
    HIPCHK(h, bs->W.grow(h, (size_t)2 * n * PB_NCHANOUT));
    if (beams) HIPCHK(h, bs->beams.grow(h, nval));
    if (rows_used) HIPCHK(h, bs->used.grow(h, nused));
    if (kur && rows_used) HIPCHK(h, bs->pref.grow(h, (size_t)T + 1));

    const pb_handle::BufSet &b = h->set();
    // behind the set's channeliser and detect (ev_chan): whatever refills the set is queued by a later call, and this
    // one returns only when its own stream has drained
    HIPCHK(h, hipStreamWaitEvent(bs->st, b.ev_chan, 0));
    HIPCHK(h, bs->mark(0));
    HIPCHK(h, bs->par.from_host(bs->h_par.data(), 2 * (size_t)n, bs->st));
    HIPCHK(h, bs->gain.from_host(bs->h_gain.data(), (size_t)n, bs->st));
    HIPCHK(h, bs->shift.from_host(bs->h_shift.data(), PB_NCHANOUT, bs->st));
    HIPCHK(h, bs->proj.from_host(bs->h_proj.p, nproj, bs->st));
    BeamProjArgs a;
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
    a.spc = tscr >= BEAMPROJ_CHUNK_ROWS ? 1 : BEAMPROJ_CHUNK_ROWS / tscr;
    if (kur && rows_used) {
        k_beamproj_prefix<<<1, 64, 0, bs->st>>>(b.d_wrow, A, (size_t)h->S * h->R, T, bs->pref.p);
        a.pref = bs->pref.p;
    }
    BEAMPROJ_ANY(A, beamproj_weights_launch, nbeam, bs->par.p, bs->gain.p, bs->proj.p, bs->W.p, bs->st)
    HIPCHK(h, bs->launched(1));
    if (beams || rows_used) BEAMPROJ_ANY(A, beamproj_launch, a, bs->st)
    HIPCHK(h, bs->launched(2));
    HIPCHK(h, bs->beams.to_host(beams, nval, bs->st));
    HIPCHK(h, bs->used.to_host(rows_used, nused, bs->st));
    HIPCHK(h, bs->finish());
    return PB_OK;
}

extern "C" int pb_beamform_proj_timers(const pb_handle *h, float *ms3)
{
    if (!h || !ms3) return PB_EINVAL;
    for (int k = 0; k < 3; ++k) ms3[k] = h->beamproj ? h->beamproj->ms[k] : 0.f;
    return PB_OK;
}
