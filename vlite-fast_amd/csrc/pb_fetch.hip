// The way back to the host of the C ABI (include/pb_hip.h): the batch's bytes and planes (pb_fetch, pb_fetch_ptr,
// pb_output_dev), the intermediate results a debug_keep handle holds (pb_debug_fetch), and the stage timers with their
// event pool (pb_profile, pb_get_timers; StageTimer in pb_internal.h).
#include <cstring>

#include "pb_internal.h"

extern "C" int pb_fetch_ptr(pb_handle *h, int ant, int stream, const uint8_t **codes)
{
    if (!h || !codes) return PB_EINVAL;
    if (check_ant(h, ant)) return PB_EINVAL;
    if (stream < 0 || stream > 1) return fail(h, PB_EINVAL, "stream must be 0 or 1");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const pb_handle::BufSet &b = h->set();
    HIPCHK(h, hipEventSynchronize(b.ev_det.e));
    *codes = b.h_codes.p + ((size_t)ant * 2 + stream) * h->S * h->trim;
    return PB_OK;
}

extern "C" int pb_fetch(pb_handle *h, int ant, int seg0, int nseg, uint8_t *raw_codes, uint8_t *kur_codes,
                        float *weights, float *ave_raw, float *ave_kur)
{
    if (!h) return PB_EINVAL;
    if (check_ant(h, ant)) return PB_EINVAL;
    if (seg0 < 0 || nseg < 1 || seg0 + nseg > h->S) return fail(h, PB_EINVAL, "pb_fetch: segment range");
    if ((ave_raw || ave_kur) && !h->cfg.keep_ave) return fail(h, PB_ESTATE, "pb_fetch: fp32 planes need keep_ave=1");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // the selected set's detect + asynchronous D2H (pinned mirror h_codes) have an event of
    // their own, so fetching one set does not wait for work in flight on the other
    const pb_handle::BufSet &b = h->set();
    HIPCHK(h, hipEventSynchronize(b.ev_det.e));
    const size_t S = h->S;
    const uint8_t *c0 = b.h_codes.p + (((size_t)ant * 2 + 0) * S + seg0) * h->trim;
    const uint8_t *c1 = b.h_codes.p + (((size_t)ant * 2 + 1) * S + seg0) * h->trim;
    if (raw_codes) memcpy(raw_codes, c0, (size_t)nseg * h->trim);
    if (kur_codes) memcpy(kur_codes, c1, (size_t)nseg * h->trim);
    if (ave_raw) HIPCHK(h, hipMemcpy(ave_raw, b.d_ave.p + (((size_t)ant * 2 + 0) * S + seg0) * h->ave_per_seg,
                                    (size_t)nseg * h->ave_per_seg * sizeof(float), hipMemcpyDeviceToHost));
    const int cstream = h->cfg.rfi_mode == 0 ? 0 : 1;     // the stream whose plane a coadd target replaces
    if (b.d_coadd_target && ant == 0 && ((cstream == 0 && ave_raw) || (cstream == 1 && ave_kur))) {
        HIPCHK(h, hipMemcpy(cstream ? ave_kur : ave_raw, b.d_coadd_target + (size_t)seg0 * h->ave_per_seg,
                            (size_t)nseg * h->ave_per_seg * sizeof(float), hipMemcpyDeviceToHost));
        if (cstream) ave_kur = nullptr; else ave_raw = nullptr;
    }
    if (ave_kur) HIPCHK(h, hipMemcpy(ave_kur, b.d_ave.p + (((size_t)ant * 2 + 1) * S + seg0) * h->ave_per_seg,
                                    (size_t)nseg * h->ave_per_seg * sizeof(float), hipMemcpyDeviceToHost));
    if (weights) {
        // what tscrunch_weights sees: after pscrunch_weights (npol 1) rows below MIN_WEIGHT are 0
        std::vector<float> w((size_t)nseg * h->R);
        HIPCHK(h, hipMemcpy(w.data(), b.d_wrow.p + (size_t)ant * S * h->R + (size_t)seg0 * h->R,
                            w.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < w.size(); ++i) {
            float v = w[i];
            if (h->cfg.npol == 1) v = ((double)v >= 0.2) ? (float)(0.5 * (double)(v + v)) : 0.f;
            weights[i] = v;
        }
    }
    return PB_OK;
}

extern "C" int pb_output_dev(pb_handle *h, int ant, int stream, void **codes, void **ave)
{
    if (!h) return PB_EINVAL;
    if (check_ant(h, ant)) return PB_EINVAL;
    if (stream < 0 || stream > 1) return fail(h, PB_EINVAL, "stream must be 0 or 1");
    const pb_handle::BufSet &b = h->set();
    if (codes) *codes = b.d_codes.p + ((size_t)ant * 2 + stream) * h->S * h->trim;
    if (ave) {
        *ave = b.d_ave.p ? b.d_ave.p + ((size_t)ant * 2 + stream) * h->S * h->ave_per_seg : nullptr;
        if (b.d_coadd_target && ant == 0 && stream == (h->cfg.rfi_mode == 0 ? 0 : 1)) *ave = b.d_coadd_target;
    }
    return PB_OK;
}

extern "C" int pb_debug_fetch(pb_handle *h, int what, int ant, int seg, void *dst, size_t nbytes)
{
    if (!h || !dst) return PB_EINVAL;
    if (check_ant(h, ant)) return PB_EINVAL;
    if (seg < 0 || seg >= h->S) return fail(h, PB_EINVAL, "segment out of range");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, sync_all(h));
    const size_t nb = h->nblk_seg, cap = (size_t)h->S * nb;
    const pb_handle::BufSet &b = h->set();
    const bool per_row = what == PB_DBG_POW_FB || what == PB_DBG_KUR_FB || what == PB_DBG_DAG_FB;
    if ((per_row || what == PB_DBG_POW || what == PB_DBG_KUR || what == PB_DBG_DAG) && !b.d_stats.p)
        return fail(h, PB_ESTATE, "pb_debug_fetch: statistics need debug_keep=1");
    if (what == PB_DBG_POW || what == PB_DBG_KUR || what == PB_DBG_DAG) {
        if (nbytes != 2 * nb * sizeof(float)) return fail(h, PB_EINVAL, "pb_debug_fetch: size");
        for (int pol = 0; pol < 2; ++pol) {
            const float *src = b.d_stats.p + (size_t)ant * 6 * cap + ((size_t)what * 2 + pol) * cap + (size_t)seg * nb;
            HIPCHK(h, hipMemcpy((float *)dst + pol * nb, src, nb * sizeof(float), hipMemcpyDeviceToHost));
        }
        return PB_OK;
    }
    if (per_row) {
        const size_t rcap = (size_t)h->S * h->R;
        const float *fb = b.d_stats.p + (size_t)h->A * 6 * cap + (size_t)ant * 5 * rcap;
        const int npl = what == PB_DBG_DAG_FB ? 1 : 2;
        const int first = what == PB_DBG_POW_FB ? 0 : (what == PB_DBG_KUR_FB ? 2 : 4);
        if (nbytes != (size_t)npl * h->R * sizeof(float)) return fail(h, PB_EINVAL, "pb_debug_fetch: size");
        for (int pl = 0; pl < npl; ++pl)
            HIPCHK(h, hipMemcpy((float *)dst + (size_t)pl * h->R, fb + (size_t)(first + pl) * rcap + (size_t)seg * h->R,
                                (size_t)h->R * sizeof(float), hipMemcpyDeviceToHost));
        return PB_OK;
    }
    if (what == PB_DBG_FLAGS) {
        if (nbytes != nb) return fail(h, PB_EINVAL, "pb_debug_fetch: size");
        HIPCHK(h, hipMemcpy(dst, b.d_flags.p + (size_t)ant * cap + (size_t)seg * nb, nb, hipMemcpyDeviceToHost));
        return PB_OK;
    }
    if (what == PB_DBG_ROWWEIGHT) {
        if (nbytes != (size_t)h->R * sizeof(float)) return fail(h, PB_EINVAL, "pb_debug_fetch: size");
        HIPCHK(h, hipMemcpy(dst, b.d_wrow.p + (size_t)ant * h->S * h->R + (size_t)seg * h->R, nbytes, hipMemcpyDeviceToHost));
        return PB_OK;
    }
    return fail(h, PB_EINVAL, "pb_debug_fetch: unknown item");
}

// ---- the stage timers: the event pool of StageTimer (pb_internal.h)
hipEvent_t take_event(pb_handle *h)
{
    std::vector<hipEvent_t> &pool = h->ev_pool.free;
    if (!pool.empty()) {
        hipEvent_t e = pool.back();
        pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

// a finished event pair: its time to the stage's total, both events back to the pool
static void book_pair(pb_handle *h, const pb_handle::Pending &p)
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
        h->timers.ms[p.stage] += ms;
        h->timers.launches[p.stage] += 1;
    }
    h->ev_pool.free.push_back(p.a);
    h->ev_pool.free.push_back(p.b);
}

// Read back the oldest event pairs that have completed, without waiting for anything: keeps the
// pool small, so that a long profiled run creates no events (hipEventCreate costs tens of us).
void retire_done(pb_handle *h)
{
    size_t n = 0;
    while (n < h->pending.size() && hipEventQuery(h->pending[n].b) == hipSuccess) book_pair(h, h->pending[n++]);
    if (n) h->pending.erase(h->pending.begin(), h->pending.begin() + n);
}

// everything recorded is read back, so that every event is in the pool again (which is where pb_destroy leaves them)
void drain_timers(pb_handle *h)
{
    if (h->pending.empty()) return;
    (void)sync_all(h);
    for (const auto &p : h->pending) book_pair(h, p);
    h->pending.clear();
}

extern "C" int pb_profile(pb_handle *h, int enable)
{
    if (!h) return PB_EINVAL;
    h->profile = enable != 0;
    if (h->profile) {
        // enough events for a few batches in flight; later ones are recycled by retire_done
        (void)hipSetDevice(h->cfg.device);
        while (h->ev_pool.free.size() < 64) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) break;
            h->ev_pool.free.push_back(e);
        }
    }
    return PB_OK;
}

extern "C" int pb_get_timers(pb_handle *h, pb_timers *out, int reset)
{
    if (!h || !out) return PB_EINVAL;
    (void)hipSetDevice(h->cfg.device);
    drain_timers(h);
    *out = h->timers;
    if (reset) memset(&h->timers, 0, sizeof h->timers);
    return PB_OK;
}
