// The correlator's X step (include/pb_hip.h: pb_correlate*): every antenna pair of a handle's batch, per channel, from
// the complex in-band spectra that the coherence channeliser leaves in HBM (BufSet::d_Praw / d_Pkur, float2
// [A][S][2][R][4096]).  The sum over a gate's rows is in row order, so a lane walks its channel's window alone and the
// parallelism is gates x channels x antenna tiles.
//
// k_correlate: one 64-lane workgroup = 64 channels of one gate and one antenna tile; a lane owns one channel and keeps
//   the tile's accumulators (8 floats per baseline) in registers.  Every spectrum value of the tile is loaded once and
//   serves all of the tile's baselines and products; the loads of the next U rows are in flight while the current U
//   rows are added.  A gate's window differs per channel only in its first row: the addresses are coalesced over the
//   channels whenever neighbouring row0 are equal and correct when they are not.  No LDS, no atomics.
//   Tiles: antennas in groups of four; a group against itself (k_correlate<N, N, true>: N (N + 1) / 2 baselines, 80
//   accumulators at N = 4) and, beyond four antennas, group 0 against two antennas of group 1 at a time
//   (k_correlate<4, N, false>: 4 N baselines).
// k_corr_prefix: per baseline the running count of rows whose weight is > 0 for both antennas (one wave, ballots), so
//   that rows_used of the excised stream is a difference of two entries.
// What the fringe-stopping kernel (pb_correlate_track.hip) shares with these -- the arguments, the loader's walk over a
// window, one term, the stores, the prefix kernel's launch -- is correlate_dev.h.
// Host side: pb_corr_state is a job of csrc/pb_job.h (stream, stage events and times, owned buffers that grow, teardown),
// and what the calls refuse about the handle, the stream and the batch is that header's spectra_check_*.
#include "correlate_dev.h"

struct PB_LOCAL pb_corr_state : PbJob<2> {      // stages: kernels, copy to the host
    DevBuf<float> vis;
    DevBuf<int32_t> used, row0, pref;
    std::vector<int32_t> h_row0;
};

template <int NI, int NJ, bool DIAG>
__global__ __launch_bounds__(64) void k_correlate(CorrArgs a)
{
    constexpr int NL = DIAG ? NI : NI + NJ;              // antennas the tile reads
    constexpr int NBL = DIAG ? NI * (NI + 1) / 2 : NI * NJ;
    constexpr int U = corr_rows_in_flight(NL);
    const int c = blockIdx.x * 64 + threadIdx.x, g = blockIdx.y;
    const int R = a.R, nrows = a.nrows;
    const size_t pol_stride = (size_t)R * PB_NCHANOUT, seg_stride = 2 * pol_stride, ant_stride = (size_t)a.S * seg_stride;
    const int r0 = a.row0[(size_t)g * PB_NCHANOUT + c];

    const float2 *xp[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int ant = (DIAG || l < NI) ? a.i0 + l : a.j0 + (l - NI);
        xp[l] = a.X + (size_t)ant * ant_stride + c;
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

    request();
    for (int kb = 0; kb < nrows; kb += U) {
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

    int b = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = DIAG ? i : 0; j < (DIAG ? NI : NJ); ++j) {
            corr_store(a, g, c, r0, corr_bl(a.A, a.i0 + i, DIAG ? a.i0 + j : a.j0 + j), acc[b]);
            ++b;
        }
}

// pref[bl][t] = the number of rows before t whose weight is > 0 for antenna i and for antenna j, t = 0 .. T
__global__ __launch_bounds__(64) void k_corr_prefix(const float *wrow, int A, size_t ant_stride, int T, int32_t *pref)
{
    const int i = blockIdx.x, j = blockIdx.y;
    if (j < i) return;
    const float *wi = wrow + (size_t)i * ant_stride, *wj = wrow + (size_t)j * ant_stride;
    int32_t *P = pref + (size_t)corr_bl(A, i, j) * (T + 1);
    const int lane = threadIdx.x;
    int total = 0;
    if (lane == 0) P[0] = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool ok = t < T && wi[t] > 0.f && wj[t] > 0.f;
        const unsigned long long m = __ballot(ok);
        if (t < T) P[t + 1] = total + __popcll(m & (~0ull >> (63 - lane)));
        total += __popcll(m);
    }
}

void corr_prefix_launch(const float *wrow, int A, size_t ant_stride, int T, int32_t *pref, hipStream_t st)
{
    k_corr_prefix<<<dim3(A, A), 64, 0, st>>>(wrow, A, ant_stride, T, pref);
}

template <int NI, int NJ, bool DIAG> static void corr_launch(const CorrArgs &a, int ngate, hipStream_t st)
{
    k_correlate<NI, NJ, DIAG><<<dim3(PB_NCHANOUT / 64, ngate), 64, 0, st>>>(a);
}

static void corr_launch_all(CorrArgs a, int ngate, hipStream_t st)
{
    for (int i0 = 0; i0 < a.A; i0 += 4) {
        a.i0 = a.j0 = i0;
        switch (a.A - i0 < 4 ? a.A - i0 : 4) {
        case 1: corr_launch<1, 1, true>(a, ngate, st); break;
        case 2: corr_launch<2, 2, true>(a, ngate, st); break;
        case 3: corr_launch<3, 3, true>(a, ngate, st); break;
        default: corr_launch<4, 4, true>(a, ngate, st); break;
        }
    }
    a.i0 = 0;
    for (int j0 = 4; j0 < a.A; j0 += 2) {
        a.j0 = j0;
        if (a.A - j0 >= 2) corr_launch<4, 2, false>(a, ngate, st);
        else corr_launch<4, 1, false>(a, ngate, st);
    }
}

void pb_correlate_free(pb_handle *h) { job_free(h->corr); }

// row0 is in h->corr->h_row0, checked: upload, launch, copy out, wait
static int corr_run(pb_handle *h, int stream, int nseg, int ngate, int nrows, float *vis, int32_t *rows_used)
{
    pb_corr_state *cs = h->corr;
    const int nbl = h->A * (h->A + 1) / 2, T = nseg * h->R;
    const size_t nrow0 = (size_t)ngate * PB_NCHANOUT, nused = nrow0 * nbl, nvis = nused * 8;
    if (!job_output_fits(nvis * sizeof(float))) return fail(h, PB_EINVAL, "pb_correlate: outputs beyond 2 GiB; use fewer gates per call");
    const bool kur = stream == PB_CORR_KUR;
    HIPCHK(h, cs->ensure(h->cfg.device));
    if (vis) HIPCHK(h, cs->vis.grow(h, nvis));
    if (rows_used) HIPCHK(h, cs->used.grow(h, nused));
    HIPCHK(h, cs->row0.grow(h, nrow0));
    if (kur && rows_used) HIPCHK(h, cs->pref.grow(h, (size_t)nbl * (T + 1)));

    const pb_handle::BufSet &b = h->set();
    // behind the set's channeliser and detect (ev_chan); whatever refills the set is queued by a later call, and this
    // one returns only when its own stream has drained
    HIPCHK(h, hipStreamWaitEvent(cs->st, b.ev_chan.e, 0));
    HIPCHK(h, cs->row0.from_host(cs->h_row0.data(), nrow0, cs->st));
    HIPCHK(h, cs->mark(0));
    CorrArgs a;
    a.X = (const float2 *)(kur ? b.d_Pkur.p : b.d_Praw.p);
    a.row0 = cs->row0.p;
    a.pref = nullptr;
    a.vis = vis ? (float2 *)cs->vis.p : nullptr;
    a.used = rows_used ? cs->used.p : nullptr;
    a.A = h->A;
    a.S = h->S;
    a.R = h->R;
    a.T = T;
    a.nrows = nrows;
    a.i0 = a.j0 = 0;
    if (kur && rows_used) {
        corr_prefix_launch(b.d_wrow.p, h->A, (size_t)h->S * h->R, T, cs->pref.p, cs->st);
        a.pref = cs->pref.p;
    }
    corr_launch_all(a, ngate, cs->st);
    HIPCHK(h, cs->launched(1));
    HIPCHK(h, cs->vis.to_host(vis, nvis, cs->st));
    HIPCHK(h, cs->used.to_host(rows_used, nused, cs->st));
    HIPCHK(h, cs->finish());
    return PB_OK;
}

extern "C" int pb_correlate_info(const pb_handle *h, int *nbl, int *nprod)
{
    if (!h) return PB_EINVAL;
    if (nbl) *nbl = h->A * (h->A + 1) / 2;
    if (nprod) *nprod = 4;
    return PB_OK;
}

extern "C" int pb_correlate_gated(pb_handle *h, int stream, int nseg, const int32_t *row0, int ngate, int nrows,
                                  float *vis, int32_t *rows_used)
{
    if (!h) return PB_EINVAL;
    if (int rc = spectra_check_config(h, "pb_correlate_gated", stream, nseg)) return rc;
    if (int rc = spectra_check_batch(h, "pb_correlate_gated", nseg)) return rc;
    if (ngate <= 0 || nrows <= 0) return fail(h, PB_EINVAL, "pb_correlate_gated: ngate and nrows must be positive");
    if (!row0) return fail(h, PB_EINVAL, "pb_correlate_gated: row0 is null");
    const int T = nseg * h->R;
    const size_t n = (size_t)ngate * PB_NCHANOUT;
    for (size_t k = 0; k < n; ++k)
        if (row0[k] < 0 || row0[k] > T - nrows) return fail(h, PB_EINVAL, "pb_correlate_gated: a window leaves the batch's rows");
    if (!h->corr) h->corr = new pb_corr_state;
    h->corr->h_row0.assign(row0, row0 + n);
    return corr_run(h, stream, nseg, ngate, nrows, vis, rows_used);
}

extern "C" int pb_correlate(pb_handle *h, int stream, int nseg, int int_rows, float *vis, int32_t *rows_used, int *ngate)
{
    if (!h) return PB_EINVAL;
    if (int rc = spectra_check_config(h, "pb_correlate", stream, nseg)) return rc;
    if (int rc = spectra_check_batch(h, "pb_correlate", nseg)) return rc;
    const int T = nseg * h->R;
    if (int_rows <= 0 || T % int_rows) return fail(h, PB_EINVAL, "pb_correlate: int_rows must be positive and divide the batch's rows");
    const int ng = T / int_rows;
    if (!h->corr) h->corr = new pb_corr_state;
    h->corr->h_row0.resize((size_t)ng * PB_NCHANOUT);
    for (int g = 0; g < ng; ++g)
        for (int c = 0; c < PB_NCHANOUT; ++c) h->corr->h_row0[(size_t)g * PB_NCHANOUT + c] = g * int_rows;
    if (ngate) *ngate = ng;
    return corr_run(h, stream, nseg, ng, int_rows, vis, rows_used);
}

extern "C" int pb_correlate_timers(const pb_handle *h, float *ms2)
{
    if (!h || !ms2) return PB_EINVAL;
    ms2[0] = h->corr ? h->corr->ms[0] : 0.f;
    ms2[1] = h->corr ? h->corr->ms[1] : 0.f;
    return PB_OK;
}
