// The fringe-stopping correlator (include/pb_hip.h: pb_correlate_tracked): pb_correlate_gated on spectra that are turned,
// per antenna, row and channel, by a delay and a phase that change linearly with the row.  The host evaluates the model
// per (antenna, row) in binary64 -- s, the delay's slope in turns per bin, and p, the phase in turns -- and uploads the
// two as one table sp[t][a] = (s, p); the turn per channel is the kernel's.
//
// k_correlate_track: k_correlate's decomposition (correlate_dev.h; pb_correlate.hip) -- one 64-lane workgroup = 64
//   channels of one gate and one antenna tile, a lane owns a channel and the tile's accumulators, the next U rows' loads
//   are in flight while the current U rows are added.  Before a row's products every loaded value of the row is turned
//   in registers, once per (antenna of the tile, row): the rotation serves both pols and all of the tile's baselines, and
//   no turned copy of the spectra exists in memory.  A row's (s, p) are the same for every lane whose window starts at
//   the same row: a workgroup whose 64 first rows are equal (every uniform gate) reads them through a wave-uniform index,
//   i.e. as scalar loads; one whose first rows differ reads them per lane.  The two are the same loop, compiled twice, and
//   the workgroup takes one of them as a whole.  No LDS, no atomics.
//   Tiles: those of k_correlate.
// Host side: pb_track_state is a job of csrc/pb_job.h like pb_corr_state, with the table besides.
#include "correlate_dev.h"
#include "rotation_dev.h"

#include <cstdint>
#include <type_traits>

struct PB_LOCAL pb_track_state : PbJob<3> {      // stages: uploads and the prefix kernel, kernels, copy to the host
    DevBuf<float> vis;
    DevBuf<int32_t> used, row0, pref;
    DevBuf<double> sp;                           // [T][A][2]: s, p
    std::vector<int32_t> h_row0;
    std::vector<double> h_sp;
};

namespace {

// rows in flight per buffer: corr_rows_in_flight, but three rows instead of four for the four-antenna group, whose 80
// accumulators and two buffers leave the rotation's temporaries no room below 256 registers (two waves per SIMD)
constexpr int track_rows_in_flight(int nl) { return nl == 4 ? 3 : corr_rows_in_flight(nl); }

}  // namespace

// x exp(+2 pi i r), w = (cr, sr): the beamformer's voltage lines (include/pb_hip.h), every line one binary32 operation
__device__ __forceinline__ float2 track_turn(const float2 x, float cr, float sr)
{
    const float rc = x.x * cr, is = x.y * sr;
    const float ic = x.y * cr, rs = x.x * sr;
    return make_float2(rc - is, ic + rs);
}

template <int NI, int NJ, bool DIAG>
__global__ __launch_bounds__(64) void k_correlate_track(CorrArgs a, const double2 *sp)
{
    constexpr int NL = DIAG ? NI : NI + NJ;              // antennas the tile reads
    constexpr int NBL = DIAG ? NI * (NI + 1) / 2 : NI * NJ;
    constexpr int U = track_rows_in_flight(NL);
    const int c = blockIdx.x * 64 + threadIdx.x, g = blockIdx.y;
    const int R = a.R, nrows = a.nrows;
    const size_t pol_stride = (size_t)R * PB_NCHANOUT, seg_stride = 2 * pol_stride, ant_stride = (size_t)a.S * seg_stride;
    const int r0 = a.row0[(size_t)g * PB_NCHANOUT + c];
    const double kbin = (double)(PB_CHANMIN + c);

    const float2 *xp[NL];
    int ant[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        ant[l] = (DIAG || l < NI) ? a.i0 + l : a.j0 + (l - NI);
        xp[l] = a.X + (size_t)ant[l] * ant_stride + c;
    }
    CorrWalk w(r0, R, seg_stride);

    float2 cur[U][NL][2], nxt[U][NL][2];
    auto request = [&]() {
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                nxt[u][l][0] = xp[l][w.off];
                nxt[u][l][1] = xp[l][w.off + pol_stride];
            }
            w.step(nrows, R, seg_stride, pol_stride);
        }
    };

    float2 acc[NBL][4];
#pragma unroll
    for (int b = 0; b < NBL; ++b)
#pragma unroll
        for (int pr = 0; pr < 4; ++pr) acc[b][pr] = make_float2(0.f, 0.f);

    // the window's rows from first row t0 on, compiled twice.  t0 the workgroup's (uniform): the U rows' table entries are
    // scalar values, fetched ahead of the wait for the rows' spectra; t0 the lane's: vector loads, one row at a time
    auto rows = [&](auto uniform, const int t0) __attribute__((always_inline)) {
        constexpr bool AHEAD = decltype(uniform)::value;
        request();
        for (int kb = 0; kb < nrows; kb += U) {
            double2 tab[AHEAD ? U : 1][NL];
            if constexpr (AHEAD) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = kb + u < nrows ? kb + u : nrows - 1;      // past the window's end: its last row, unused
#pragma unroll
                    for (int l = 0; l < NL; ++l) tab[u][l] = sp[(size_t)(t0 + k) * a.A + ant[l]];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    cur[u][l][0] = nxt[u][l][0];
                    cur[u][l][1] = nxt[u][l][1];
                }
            if (kb + U < nrows) request();
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (kb + u < nrows) {
#pragma unroll
                    for (int l = 0; l < NL; ++l) {
                        if constexpr (!AHEAD) tab[0][l] = sp[(size_t)(t0 + kb + u) * a.A + ant[l]];
                        // the phase (include/pb_hip.h) in binary64, every operation rounded once
                        const double2 v = tab[AHEAD ? u : 0][l];
                        const double ks = kbin * v.x;
                        const double turn = v.y + ks;
                        const double r64 = turn - rint(turn);
                        float cr, sr;
                        img_rotation((float)r64, cr, sr);
                        cur[u][l][0] = track_turn(cur[u][l][0], cr, sr);
                        cur[u][l][1] = track_turn(cur[u][l][1], cr, sr);
                    }
                    int b = 0;
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int j = DIAG ? i : 0; j < (DIAG ? NI : NJ); ++j) {
                            const int lj = DIAG ? j : NI + j;
#pragma unroll
                            for (int p = 0; p < 2; ++p)
#pragma unroll
                                for (int q = 0; q < 2; ++q) corr_term(acc[b][2 * p + q], cur[u][i][p], cur[u][lj][q]);
                            ++b;
                        }
                }
            }
        }
    };
    const int r0_first = __builtin_amdgcn_readfirstlane(r0);
    if (__all(r0 == r0_first)) rows(std::true_type(), r0_first);
    else rows(std::false_type(), r0);

    int b = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = DIAG ? i : 0; j < (DIAG ? NI : NJ); ++j) {
            corr_store(a, g, c, r0, corr_bl(a.A, a.i0 + i, DIAG ? a.i0 + j : a.j0 + j), acc[b]);
            ++b;
        }
}

template <int NI, int NJ, bool DIAG> static void track_launch(const CorrArgs &a, const double2 *sp, int ngate, hipStream_t st)
{
    k_correlate_track<NI, NJ, DIAG><<<dim3(PB_NCHANOUT / 64, ngate), 64, 0, st>>>(a, sp);
}

static void track_launch_all(CorrArgs a, const double2 *sp, int ngate, hipStream_t st)
{
    for (int i0 = 0; i0 < a.A; i0 += 4) {
        a.i0 = a.j0 = i0;
        switch (a.A - i0 < 4 ? a.A - i0 : 4) {
        case 1: track_launch<1, 1, true>(a, sp, ngate, st); break;
        case 2: track_launch<2, 2, true>(a, sp, ngate, st); break;
        case 3: track_launch<3, 3, true>(a, sp, ngate, st); break;
        default: track_launch<4, 4, true>(a, sp, ngate, st); break;
        }
    }
    a.i0 = 0;
    for (int j0 = 4; j0 < a.A; j0 += 2) {
        a.j0 = j0;
        if (a.A - j0 >= 2) track_launch<4, 2, false>(a, sp, ngate, st);
        else track_launch<4, 1, false>(a, sp, ngate, st);
    }
}

void pb_correlate_track_free(pb_handle *h) { job_free(h->track); }

// the model per (antenna, row) (include/pb_hip.h), every operation rounded once (-ffp-contract=off): false when a delay
// or a phase leaves 2^24 at either end of the batch -- both are linear in the row, so the ends bound them
static bool track_table(const double *model, int A, int T, int64_t row_base, std::vector<double> &sp)
{
    sp.resize((size_t)T * A * 2);
    for (int a = 0; a < A; ++a) {
        const double delay0 = model[4 * a], delay_rate = model[4 * a + 1], psi0 = model[4 * a + 2], psi_rate = model[4 * a + 3];
        for (int t = 0; t < T; ++t) {
            const double tau = (double)(row_base + t);
            const double dr = delay_rate * tau, pr = psi_rate * tau;
            const double d = delay0 + dr, p = psi0 + pr;
            if ((t == 0 || t == T - 1) && !(delay_ok(d) && delay_ok(p))) return false;
            sp[((size_t)t * A + a) * 2] = delay_slope(d);
            sp[((size_t)t * A + a) * 2 + 1] = p;
        }
    }
    return true;
}

extern "C" int pb_correlate_tracked(pb_handle *h, int stream, int nseg, const int32_t *row0, int ngate, int nrows,
                                    const double *model, int64_t row_base, float *vis, int32_t *rows_used)
{
    const char *w = "pb_correlate_tracked";
    if (!h) return PB_EINVAL;
    if (int rc = spectra_check_config(h, w, stream, nseg)) return rc;
    if (int rc = spectra_check_batch(h, w, nseg)) return rc;
    if (ngate <= 0 || nrows <= 0) return fail(h, PB_EINVAL, "pb_correlate_tracked: ngate and nrows must be positive");
    const int A = h->A, T = nseg * h->R;
    const size_t nrow0 = (size_t)ngate * PB_NCHANOUT;
    if (row0) {
        for (size_t k = 0; k < nrow0; ++k)
            if (row0[k] < 0 || row0[k] > T - nrows) return fail(h, PB_EINVAL, "pb_correlate_tracked: a window leaves the batch's rows");
    } else if (T % nrows || ngate != T / nrows)
        return fail(h, PB_EINVAL, "pb_correlate_tracked: without row0, nrows must divide the batch's rows and ngate be their quotient");
    if (!model) return fail(h, PB_EINVAL, "pb_correlate_tracked: model is null");
    for (int k = 0; k < 4 * A; ++k)
        if (!std::isfinite(model[k])) return fail(h, PB_EINVAL, "pb_correlate_tracked: a model entry is not finite");
    if (row_base > INT64_MAX - T) return fail(h, PB_EINVAL, "pb_correlate_tracked: row_base leaves the rows that can be counted");
    const int nbl = A * (A + 1) / 2;
    const size_t nused = nrow0 * nbl, nvis = nused * 8;
    if (!job_output_fits(nvis * sizeof(float))) return fail(h, PB_EINVAL, "pb_correlate_tracked: outputs beyond 2 GiB; use fewer gates per call");
    if (!h->track) h->track = new pb_track_state;
    pb_track_state *ts = h->track;
    if (!track_table(model, A, T, row_base, ts->h_sp))
        return fail(h, PB_EINVAL, "pb_correlate_tracked: a delay or a phase of the model leaves 2^24 within the batch");
    if (row0) ts->h_row0.assign(row0, row0 + nrow0);
    else {
        ts->h_row0.resize(nrow0);
        for (int g = 0; g < ngate; ++g)
            for (int c = 0; c < PB_NCHANOUT; ++c) ts->h_row0[(size_t)g * PB_NCHANOUT + c] = g * nrows;
    }

    const bool kur = stream == PB_CORR_KUR;
    HIPCHK(h, ts->ensure(h->cfg.device));
    if (vis) HIPCHK(h, ts->vis.grow(h, nvis));
    if (rows_used) HIPCHK(h, ts->used.grow(h, nused));
    HIPCHK(h, ts->row0.grow(h, nrow0));
    HIPCHK(h, ts->sp.grow(h, ts->h_sp.size()));
    if (kur && rows_used) HIPCHK(h, ts->pref.grow(h, (size_t)nbl * (T + 1)));

    const pb_handle::BufSet &b = h->set();
    // behind the set's channeliser and detect (ev_chan), as pb_correlate_gated
    HIPCHK(h, hipStreamWaitEvent(ts->st, b.ev_chan.e, 0));
    HIPCHK(h, ts->mark(0));
    HIPCHK(h, ts->row0.from_host(ts->h_row0.data(), nrow0, ts->st));
    HIPCHK(h, ts->sp.from_host(ts->h_sp.data(), ts->h_sp.size(), ts->st));
    CorrArgs a;
    a.X = (const float2 *)(kur ? b.d_Pkur.p : b.d_Praw.p);
    a.row0 = ts->row0.p;
    a.pref = nullptr;
    a.vis = vis ? (float2 *)ts->vis.p : nullptr;
    a.used = rows_used ? ts->used.p : nullptr;
    a.A = A;
    a.S = h->S;
    a.R = h->R;
    a.T = T;
    a.nrows = nrows;
    a.i0 = a.j0 = 0;
    if (kur && rows_used) {
        corr_prefix_launch(b.d_wrow.p, A, (size_t)h->S * h->R, T, ts->pref.p, ts->st);
        a.pref = ts->pref.p;
    }
    HIPCHK(h, ts->launched(1));
    track_launch_all(a, (const double2 *)ts->sp.p, ngate, ts->st);
    HIPCHK(h, ts->launched(2));
    HIPCHK(h, ts->vis.to_host(vis, nvis, ts->st));
    HIPCHK(h, ts->used.to_host(rows_used, nused, ts->st));
    HIPCHK(h, ts->finish());
    return PB_OK;
}

extern "C" int pb_correlate_tracked_timers(const pb_handle *h, float *ms3)
{
    if (!h || !ms3) return PB_EINVAL;
    for (int k = 0; k < 3; ++k) ms3[k] = h->track ? h->track->ms[k] : 0.f;
    return PB_OK;
}
