// The incoherent sum's entry points of the C ABI (include/pb_hip.h: pb_coadd_*, pb_set_coadd_stream,
// pb_set_coadd_target), beside their kernels: coadd_codes.hip, coadd_tree.hip and the launch_coadd_* kernels of
// k_detect.hip.  Everything here runs on the coadd stream (pb_set_coadd_stream; the main stream without one).
#include <cmath>
#include <cstring>

#include "pb_internal.h"

extern "C" int pb_set_coadd_stream(pb_handle *h, void *stream)
{
    if (!h) return PB_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, sync_all(h));
    h->s_coadd = (hipStream_t)stream;
    return PB_OK;
}

// The incoherent sum is defined on the one-pol (AA+BB) planes: coherence output does not take part in it.
static int no_coherence(pb_handle *h, const char *what)
{
    if (!h->cfg.coherence) return PB_OK;
    return fail(h, PB_EINVAL, std::string(what) + ": the coadd entry points do not take coherence output (npol = 1 only)");
}

// The coadd stream, ordered behind the selected set's detect.  The fp32 planes and the codes come from that detect,
// which may have run on the second stream; on a coadd stream of its own (pb_set_coadd_stream) the wait holds up
// neither the next batch's channeliser nor its detect.  When the host already knows that detect has finished (e.g.
// the batch's bytes have been fetched), no device-side wait is queued: a pending cross-stream wait on that event was
// measured to cost the whole pipeline 0.12 ms per second of data.
static hipError_t coadd_stream_after_detect(pb_handle *h, hipStream_t *cs)
{
    *cs = h->s_coadd ? h->s_coadd : h->stream;
    if (hipEventQuery(h->set().ev_chan.e) == hipSuccess) return hipSuccess;
    return hipStreamWaitEvent(*cs, h->set().ev_chan.e, 0);
}

extern "C" int pb_coadd_local(pb_handle *h, int nseg, float *d_sum, int accumulate)
{
    if (!h || !d_sum) return PB_EINVAL;
    if (int rc = no_coherence(h, "pb_coadd_local")) return rc;
    if (!h->cfg.keep_ave) return fail(h, PB_ESTATE, "pb_coadd_local needs keep_ave=1");
    if (nseg < 1 || nseg > h->S) return fail(h, PB_EINVAL, "pb_coadd_local: nseg out of range");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const pb_handle::BufSet &b = h->set();
    hipStream_t cs;
    HIPCHK(h, coadd_stream_after_detect(h, &cs));
    if (b.d_coadd_target && d_sum == b.d_coadd_target && !accumulate) {
        // nant = 1 with a coadd target: detect wrote the plane into d_sum itself.  Nothing to launch; the
        // "planes consumed" event is recorded by pb_coadd_release, after the caller's collective.
        if (nseg > b.processed) return fail(h, PB_EINVAL, "pb_coadd_local: more segments than the batch holds");
        return PB_OK;
    }
    hipError_t e;
    {
        StreamScope on(h, cs);            // (StageTimer records on h->stream)
        StageTimer t(h, PB_ST_COADD);
        e = launch_coadd_local(h, nseg, d_sum, accumulate, cs);
        t.stop();
        if (e == hipSuccess) e = hipEventRecord(b.ev_cl.e, cs);
    }
    HIPCHK(h, e);
    return PB_OK;
}

// The same local sum taken from this batch's quantised codes (coadd_codes.hip): what a coadder fed from the co
// rings has to work with.  Needs no fp32 planes (keep_ave may be 0).
extern "C" int pb_coadd_local_codes(pb_handle *h, int nseg, float *d_sum, int accumulate)
{
    if (!h || !d_sum) return PB_EINVAL;
    if (int rc = no_coherence(h, "pb_coadd_local_codes")) return rc;
    if (nseg < 1 || nseg > h->S) return fail(h, PB_EINVAL, "pb_coadd_local_codes: nseg out of range");
    const pb_handle::BufSet &b = h->set();
    if (nseg > b.processed) return fail(h, PB_EINVAL, "pb_coadd_local_codes: more segments than the batch holds");
    if (b.d_coadd_target && d_sum == b.d_coadd_target)
        return fail(h, PB_ESTATE, "pb_coadd_local_codes: d_sum is the set's fp32 coadd target");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t cs;
    HIPCHK(h, coadd_stream_after_detect(h, &cs));
    hipError_t e = launch_coadd_local_codes(h, nseg, d_sum, accumulate, cs);
    if (e == hipSuccess) e = hipEventRecord(b.ev_cl.e, cs);      // (the set's next detect writes codes and planes alike)
    HIPCHK(h, e);
    return PB_OK;
}

// leaves of S over items[0..n) left to right: the even positions' subtree, then the odd positions'
static void tree_order_rec(const int32_t *items, int n, int32_t *&out)
{
    if (n <= 1) {
        if (n == 1) *out++ = items[0];
        return;
    }
    int32_t ev[PB_COADD_MAX_LEAVES], od[PB_COADD_MAX_LEAVES];
    int ne = 0, no = 0;
    for (int i = 0; i < n; ++i) (i & 1 ? od[no++] : ev[ne++]) = items[i];
    tree_order_rec(ev, ne, out);
    tree_order_rec(od, no, out);
}

extern "C" int pb_coadd_tree_order(int n, int32_t *order)
{
    if (!order || n < 1 || n > PB_COADD_MAX_LEAVES) return PB_EINVAL;
    int32_t items[PB_COADD_MAX_LEAVES];
    for (int i = 0; i < n; ++i) items[i] = i;
    int32_t *out = order;
    tree_order_rec(items, n, out);
    return PB_OK;
}

// The incoherent sum in the defined order (coadd_tree.hip): one rank's node of the tree from
// the selected set's fp32 planes, ordered against detect and the set's next batch exactly like pb_coadd_local.
extern "C" int pb_coadd_local_tree(pb_handle *h, int nseg, const int32_t *ant_order, int n, float *d_dst)
{
    if (!h || !d_dst || !ant_order) return PB_EINVAL;
    if (int rc = no_coherence(h, "pb_coadd_local_tree")) return rc;
    if (!h->cfg.keep_ave) return fail(h, PB_ESTATE, "pb_coadd_local_tree needs keep_ave=1");
    if (nseg < 1 || nseg > h->S) return fail(h, PB_EINVAL, "pb_coadd_local_tree: nseg out of range");
    const pb_handle::BufSet &b = h->set();
    if (nseg > b.processed) return fail(h, PB_EINVAL, "pb_coadd_local_tree: more segments than the batch holds");
    if (n < 1 || n > PB_COADD_MAX_LEAVES) return fail(h, PB_EINVAL, "pb_coadd_local_tree: 1..PB_COADD_MAX_LEAVES leaves");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int stream = h->cfg.rfi_mode == 0 ? 0 : 1;
    const float *leaves[PB_COADD_MAX_LEAVES];
    for (int i = 0; i < n; ++i) {
        const int a = ant_order[i];
        if (a < 0 || a >= h->A) return fail(h, PB_EINVAL, "pb_coadd_local_tree: antenna index out of range");
        leaves[i] = (b.d_coadd_target && a == 0) ? b.d_coadd_target
                                                  : b.d_ave.p + ((size_t)a * 2 + stream) * h->S * h->ave_per_seg;
        if (leaves[i] == d_dst && n > 1) return fail(h, PB_EINVAL, "pb_coadd_local_tree: d_dst is one of the leaves");
    }
    hipStream_t cs;
    HIPCHK(h, coadd_stream_after_detect(h, &cs));
    if (n == 1 && leaves[0] == d_dst) return PB_OK;       // (a coadd target: detect wrote the leaf where it is wanted;
                                                          //  pb_coadd_release books the "planes consumed" event)
    hipError_t e;
    {
        StreamScope on(h, cs);            // (StageTimer records on h->stream)
        StageTimer t(h, PB_ST_COADD);
        e = launch_coadd_tree(leaves, n, d_dst, (size_t)nseg * h->ave_per_seg, cs);
        t.stop();
        if (e == hipSuccess) e = hipEventRecord(b.ev_cl.e, cs);
    }
    HIPCHK(h, e);
    return PB_OK;
}

// The root's part: T_n over the gathered partial sums (caller-owned planes), on the coadd stream.
extern "C" int pb_coadd_tree(pb_handle *h, const float *const *d_leaves, int n, float *d_dst, size_t nfloat)
{
    if (!h || !d_leaves || !d_dst) return PB_EINVAL;
    if (int rc = no_coherence(h, "pb_coadd_tree")) return rc;
    if (n < 1 || n > PB_COADD_MAX_LEAVES) return fail(h, PB_EINVAL, "pb_coadd_tree: 1..PB_COADD_MAX_LEAVES leaves");
    if (nfloat & 3) return fail(h, PB_EINVAL, "pb_coadd_tree: nfloat must be a multiple of 4");
    for (int i = 0; i < n; ++i) {
        if (!d_leaves[i] || ((uintptr_t)d_leaves[i] & 15)) return fail(h, PB_EINVAL, "pb_coadd_tree: leaf null or not 16-byte aligned");
        if (d_leaves[i] == d_dst && n > 1) return fail(h, PB_EINVAL, "pb_coadd_tree: d_dst is one of the leaves");
    }
    if ((uintptr_t)d_dst & 15) return fail(h, PB_EINVAL, "pb_coadd_tree: d_dst not 16-byte aligned");
    if (n == 1 && d_leaves[0] == d_dst) return PB_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t cs = h->s_coadd ? h->s_coadd : h->stream;
    hipError_t e;
    {
        StreamScope on(h, cs);
        StageTimer t(h, PB_ST_COADD);
        e = launch_coadd_tree(d_leaves, n, d_dst, nfloat, cs);
        t.stop();
    }
    HIPCHK(h, e);
    return PB_OK;
}

extern "C" int pb_set_coadd_target(pb_handle *h, float *d_sum)
{
    if (!h) return PB_EINVAL;
    if (int rc = no_coherence(h, "pb_set_coadd_target")) return rc;
    if (d_sum && (h->A != 1 || !h->cfg.keep_ave || h->cfg.fft_backend != PB_FFT_LDS))
        return fail(h, PB_ESTATE, "pb_set_coadd_target needs nant=1, keep_ave=1 and the LDS back end");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, sync_all(h));              // no detect of this handle is writing a plane
    h->set().d_coadd_target = d_sum;
    return PB_OK;
}

extern "C" int pb_coadd_release(pb_handle *h)
{
    if (!h) return PB_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t cs = h->s_coadd ? h->s_coadd : h->stream;
    HIPCHK(h, hipEventRecord(h->set().ev_cl.e, cs));      // what the set's next detect waits for before it writes the planes
    return PB_OK;
}

// the two pinned / device slots the coadded bytes alternate between (allocated on first use)
static int coadd_slots(pb_handle *h)
{
    const size_t nb = (size_t)h->S * h->trim;
    if (!h->d_coadd_codes.p) {
        HIPCHK(h, h->d_coadd_codes.grow(h, 2 * nb));
        HIPCHK(h, h->h_coadd_codes.grow(2 * nb));
        for (Event &ev : h->ev_coadd) HIPCHK(h, ev.create());
        h->coadd_slot = 0;
    }
    return PB_OK;
}

// Root side of the incoherent sum: scale by 1/sqrt(N), requantise on the GPU, bring the bytes to
// pinned host memory asynchronously.  codes_host != NULL: wait and copy out (simple, blocking).
// codes_host == NULL: return at once; the bytes of call k are read with pb_coadd_fetch_ptr after
// later work has been queued (two pinned buffers alternate), so the root does not stall per batch.
extern "C" int pb_coadd_finish(pb_handle *h, int nseg, const float *d_sum, int nant_total, uint8_t *codes_host)
{
    if (!h || !d_sum || nant_total < 1) return PB_EINVAL;
    if (int rc = no_coherence(h, "pb_coadd_finish")) return rc;
    if (nseg < 1 || nseg > h->S) return fail(h, PB_EINVAL, "pb_coadd_finish: nseg out of range");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t nb = (size_t)h->S * h->trim;
    if (int rc = coadd_slots(h)) return rc;
    const int slot = h->coadd_slot;
    h->coadd_slot ^= 1;
    h->coadd_last = slot;
    const float scale = (float)(1.0 / sqrt((double)nant_total));
    // requantise and copy out on the coadd stream, in order (the slot's previous copy-out, two calls
    // ago, went through the same stream)
    hipStream_t cs = h->s_coadd ? h->s_coadd : h->stream;
    HIPCHK(h, launch_coadd_digitise(h, nseg, d_sum, scale, h->d_coadd_codes.p + slot * nb, cs));
    HIPCHK(h, launch_copy_out(h->sched, h->h_coadd_codes.p + slot * nb, h->d_coadd_codes.p + slot * nb, (size_t)nseg * h->trim, cs));
    HIPCHK(h, hipEventRecord(h->ev_coadd[slot].e, cs));
    if (codes_host) {
        HIPCHK(h, hipEventSynchronize(h->ev_coadd[slot].e));
        memcpy(codes_host, h->h_coadd_codes.p + slot * nb, (size_t)nseg * h->trim);
    }
    return PB_OK;
}

// One rank's slice of the ordered sum, requantised where it was summed (coadd.py, "sliced" layout).
extern "C" int pb_coadd_digitise(pb_handle *h, const float *d_sum, size_t nfloat, int nant_total, uint8_t *d_codes)
{
    if (!h || !d_sum || !d_codes || nant_total < 1) return PB_EINVAL;
    if (int rc = no_coherence(h, "pb_coadd_digitise")) return rc;
    if (h->cfg.npol != 1) return fail(h, PB_ESTATE, "pb_coadd_digitise: a flat plane range is a code range only with npol = 1");
    if (nfloat == 0 || (nfloat & 7)) return fail(h, PB_EINVAL, "pb_coadd_digitise: nfloat must be a positive multiple of 8");
    if (((uintptr_t)d_sum & 15) || ((uintptr_t)d_codes & 3)) return fail(h, PB_EINVAL, "pb_coadd_digitise: misaligned buffer");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t cs = h->s_coadd ? h->s_coadd : h->stream;
    const float scale = (float)(1.0 / sqrt((double)nant_total));
    HIPCHK(h, launch_coadd_digitise_flat(h, d_sum, nfloat, scale, d_codes, cs));
    return PB_OK;
}

// The batch's coadded bytes, assembled on the device by the caller, to the pinned buffer pb_coadd_fetch_ptr hands out.
extern "C" int pb_coadd_publish(pb_handle *h, const uint8_t *d_codes, size_t nbytes)
{
    if (!h || !d_codes) return PB_EINVAL;
    if (int rc = no_coherence(h, "pb_coadd_publish")) return rc;
    const size_t nb = (size_t)h->S * h->trim;
    if (nbytes == 0 || nbytes > nb) return fail(h, PB_EINVAL, "pb_coadd_publish: more bytes than a batch holds");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (int rc = coadd_slots(h)) return rc;
    const int slot = h->coadd_slot;
    h->coadd_slot ^= 1;
    h->coadd_last = slot;
    hipStream_t cs = h->s_coadd ? h->s_coadd : h->stream;
    HIPCHK(h, launch_copy_out(h->sched, h->h_coadd_codes.p + slot * nb, d_codes, nbytes, cs));
    HIPCHK(h, hipEventRecord(h->ev_coadd[slot].e, cs));
    return PB_OK;
}

extern "C" int pb_coadd_fetch_ptr(pb_handle *h, int age, const uint8_t **codes)
{
    if (!h || !codes) return PB_EINVAL;
    if (!h->d_coadd_codes.p) return fail(h, PB_ESTATE, "pb_coadd_fetch_ptr: no pb_coadd_finish yet");
    if (age < 0 || age > 1) return fail(h, PB_EINVAL, "pb_coadd_fetch_ptr: age must be 0 (latest) or 1 (previous)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int slot = age == 0 ? h->coadd_last : (h->coadd_last ^ 1);
    HIPCHK(h, hipEventSynchronize(h->ev_coadd[slot].e));
    *codes = h->h_coadd_codes.p + (size_t)slot * h->S * h->trim;
    return PB_OK;
}
