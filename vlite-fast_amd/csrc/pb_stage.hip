// Input staging of the C ABI (include/pb_hip.h): the stream a batch's input is queued on and what that stream waits for,
// planar input from the host or the device, VDIF blocks with their frame index, the caller's view of the input buffer;
// and the state that persists between batches and is set from outside: the bandpass and the PFB history.
#include <cstring>

#include "pb_internal.h"

// Stream that input staging goes to.  With >= 2 buffer sets the next batch is staged while the
// previous one computes: staging and the kurtosis pass share s_kur (ordered), the channeliser on the
// main stream waits for the kurtosis event.  Refilling the set that was processed last waits for
// that whole batch.
static hipError_t submit_stream(pb_handle *h, hipStream_t *out)
{
    if (h->sets.size() < 2) { *out = h->stream; return hipSuccess; }
    *out = h->s_kur.s;
    h->staged = true;          // the next pb_process orders its first kernel behind s_kur
    if (h->last_set == h->cur_set) {
        // refilling the set that was processed last: behind that whole batch -- detect / copy-out (ev_alldone); with
        // taps = 4 the history kernel, which reads the last three rows of d_in, ran on this very stream or before
        // the channeliser that detect followed
        return hipStreamWaitEvent(h->s_kur.s, h->ev_alldone.e, 0);
    }
    // hipFFT back end: its kurtosis pass (the last reader of d_in) runs on the MAIN stream, which s_kur is
    // not ordered behind: staging batch k+2 into this set must wait for the latest FFT stage, which is
    // queued behind every earlier reader of this set's input.
    if (h->cfg.fft_backend == PB_FFT_HIPFFT && h->last_set >= 0) return hipStreamWaitEvent(h->s_kur.s, h->ev_fftdone.e, 0);
    // In-library FFT: s_kur is not in general ordered behind the channeliser that read this set's input last, on
    // the main stream (the channeliser that flags its own rows leaves s_kur empty; with three or more sets the
    // kurtosis pass of the two-kernel path no longer waits for the previous channeliser either).  This set's
    // ev_chan -- its detect is done, queued behind that channeliser and, with taps = 4, behind the history kernel
    // that read the set's last rows -- does, and it completed while the batches in between were being channelised.
    if (h->set().processed > 0) return hipStreamWaitEvent(h->s_kur.s, h->set().ev_chan.e, 0);
    return hipSuccess;
}

// one segment's two polarisations, from the host or from device memory, into the selected set's input
static int submit_planar(pb_handle *h, const char *who, int ant, int seg, const void *pol0, const void *pol1, size_t nsamp,
                         hipMemcpyKind kind)
{
    if (!h || !pol0 || !pol1) return PB_EINVAL;
    if (check_ant(h, ant)) return PB_EINVAL;
    if (seg < 0 || seg >= h->S) return fail(h, PB_EINVAL, "segment slot out of range");
    if (nsamp != h->seg_samples) return fail(h, PB_EINVAL, std::string(who) + ": nsamp must equal seg_samples_per_pol");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    uint8_t *dst = h->set().d_in.p + (((size_t)ant * h->S + seg) * 2) * h->seg_samples;
    hipStream_t ss;
    HIPCHK(h, submit_stream(h, &ss));
    HIPCHK(h, hipMemcpyAsync(dst, pol0, nsamp, kind, ss));
    HIPCHK(h, hipMemcpyAsync(dst + h->seg_samples, pol1, nsamp, kind, ss));
    return PB_OK;
}

extern "C" int pb_submit_planar(pb_handle *h, int ant, int seg, const uint8_t *pol0, const uint8_t *pol1, size_t nsamp)
{
    return submit_planar(h, "pb_submit_planar", ant, seg, pol0, pol1, nsamp, hipMemcpyHostToDevice);
}

extern "C" int pb_submit_planar_dev(pb_handle *h, int ant, int seg, const void *pol0, const void *pol1, size_t nsamp)
{
    return submit_planar(h, "pb_submit_planar_dev", ant, seg, pol0, pol1, nsamp, hipMemcpyDeviceToDevice);
}

extern "C" int pb_submit_vdif_at(pb_handle *h, int ant, int seg0, const uint8_t *block, size_t nbytes,
                                 int64_t sec0, int64_t fr0)
{
    if (!h || !block) return PB_EINVAL;
    if (check_ant(h, ant)) return PB_EINVAL;
    if (nbytes == 0 || nbytes % (2 * PB_VDIF_FRAME)) return fail(h, PB_EINVAL, "pb_submit_vdif: block is not a whole number of frame pairs");
    const size_t nslots = nbytes / PB_VDIF_FRAME, nfr = nslots / 2;
    if ((nfr * PB_VDIF_DATA) % h->seg_samples) return fail(h, PB_EINVAL, "pb_submit_vdif: block does not fill whole segments");
    const size_t nsegs = nfr * PB_VDIF_DATA / h->seg_samples;
    if (seg0 < 0 || seg0 + nsegs > (size_t)h->S) return fail(h, PB_EINVAL, "pb_submit_vdif: segments out of range");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    pb_handle::BufSet &b = h->set();
    // The frame index lives in page-locked memory of its own per buffer set, so that its H2D copy -- like
    // the block's -- is asynchronous and this call returns without waiting for the device (it used to
    // synchronise the stream because the index was a stack vector).  The event says the previous copy out
    // of this buffer has completed; before then the buffer is neither rewritten nor, to grow, let go of.
    if (b.ev_idx.e) HIPCHK(h, hipEventSynchronize(b.ev_idx.e));
    HIPCHK(h, b.h_frame_idx.grow(2 * nfr));
    HIPCHK(h, b.ev_idx.create());
    // index the headers: word0 bits 0-29 seconds, word1 bits 0-23 frame, word3 bits 16-25 thread
    int32_t *idx = b.h_frame_idx.p;
    for (size_t i = 0; i < 2 * nfr; ++i) idx[i] = -1;
    uint32_t w0, w1, w3;
    for (size_t i = 0; i < nslots; ++i) {
        const uint8_t *p = block + i * PB_VDIF_FRAME;
        memcpy(&w0, p, 4);
        memcpy(&w1, p + 4, 4);
        memcpy(&w3, p + 12, 4);
        if (w0 & 0x80000000u) continue;  // invalid-data bit
        const int thread = ((w3 >> 16) & 0x3ff) != 0;
        const int64_t rel = ((int64_t)(w0 & 0x3fffffff) - sec0) * PB_FRAMES_PER_SEC + (int64_t)(w1 & 0xffffff) - fr0;
        if (rel < 0 || rel >= (int64_t)nfr) continue;
        idx[(size_t)thread * nfr + rel] = (int32_t)i;
    }
    if (h->d_vdif.cap < nbytes || h->d_frame_idx.cap < 2 * nfr) {
        HIPCHK(h, sync_all(h));
        HIPCHK(h, h->d_vdif.grow(h, nbytes));
        HIPCHK(h, h->d_frame_idx.alloc(2 * nfr));
    }
    // d_vdif / d_frame_idx are shared by the buffer sets: every use of them is on the staging stream, in order
    hipStream_t ss;
    HIPCHK(h, submit_stream(h, &ss));
    HIPCHK(h, hipMemcpyAsync(h->d_vdif.p, block, nbytes, hipMemcpyHostToDevice, ss));
    HIPCHK(h, hipMemcpyAsync(h->d_frame_idx.p, idx, 2 * nfr * sizeof(int32_t), hipMemcpyHostToDevice, ss));
    HIPCHK(h, hipEventRecord(b.ev_idx.e, ss));
    hipError_t e;
    {
        StreamScope on(h, ss);
        e = launch_deframe(h, ant, seg0, nfr);
    }
    HIPCHK(h, e);
    return PB_OK;
}

extern "C" int pb_submit_vdif(pb_handle *h, int ant, int seg0, const uint8_t *block, size_t nbytes)
{
    if (!h || !block || nbytes < PB_VDIF_FRAME) return PB_EINVAL;
    uint32_t w0, w1;
    memcpy(&w0, block, 4);
    memcpy(&w1, block + 4, 4);
    return pb_submit_vdif_at(h, ant, seg0, block, nbytes, (int64_t)(w0 & 0x3fffffff), (int64_t)(w1 & 0xffffff));
}

extern "C" int pb_input_dev(pb_handle *h, int ant, void **dptr, size_t *nbytes)
{
    if (!h || !dptr) return PB_EINVAL;
    if (check_ant(h, ant)) return PB_EINVAL;
    *dptr = h->set().d_in.p + (size_t)ant * h->S * 2 * h->seg_samples;
    if (nbytes) *nbytes = (size_t)h->S * 2 * h->seg_samples;
    return PB_OK;
}

extern "C" int pb_reset_bandpass(pb_handle *h, int ant)
{
    if (!h) return PB_EINVAL;
    if (check_ant(h, ant)) return PB_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // the last detect (which may be on the second stream) still owns the bandpass; the next one is
    // ordered behind this stream by its channeliser's event
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_alldone.e, 0));
    HIPCHK(h, hipMemsetAsync(h->d_bp.p + (size_t)ant * 4 * PB_NCHANOUT, 0, 4 * PB_NCHANOUT * sizeof(float), h->stream));
    return PB_OK;
}

extern "C" int pb_reset_history(pb_handle *h, int ant)
{
    if (!h) return PB_EINVAL;
    if (check_ant(h, ant)) return PB_EINVAL;
    if (h->cfg.taps != 4) return PB_OK;           // only the PFB window carries rows across calls
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, sync_all(h));
    for (int slot = 0; slot < 2; ++slot) {
        const size_t a = (size_t)slot * h->A + ant;
        HIPCHK(h, hipMemset(h->d_hist_in.p + a * 2 * 3 * PFB_HIST_STRIDE, 0, (size_t)2 * 3 * PFB_HIST_STRIDE));
        HIPCHK(h, hipMemset(h->d_hist_flags.p + a * 3 * PB_BLK_PER_FFT, 1, 3 * PB_BLK_PER_FFT));
        HIPCHK(h, hipMemset(h->d_hist_valid.p + a * 3, 0, 3));
    }
    HIPCHK(h, hipStreamSynchronize(nullptr));     // (the handle's streams do not wait for the null stream by themselves)
    return PB_OK;
}

// one antenna's bandpass state of either stream (nullptr: left out) to the host or from it, with the device idle
static int copy_bandpass(pb_handle *h, int ant, float *raw, float *kur, hipMemcpyKind kind)
{
    if (!h) return PB_EINVAL;
    if (check_ant(h, ant)) return PB_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, sync_all(h));
    const bool out = kind == hipMemcpyDeviceToHost;
    float *host[2] = {raw, kur}, *dev = h->d_bp.p + (size_t)ant * 4 * PB_NCHANOUT;
    for (int str = 0; str < 2; ++str, dev += 2 * PB_NCHANOUT)
        if (host[str]) HIPCHK(h, hipMemcpy(out ? host[str] : dev, out ? dev : host[str], 2 * PB_NCHANOUT * sizeof(float), kind));
    return PB_OK;
}

extern "C" int pb_get_bandpass(pb_handle *h, int ant, float *raw, float *kur)
{
    return copy_bandpass(h, ant, raw, kur, hipMemcpyDeviceToHost);
}

extern "C" int pb_set_bandpass(pb_handle *h, int ant, const float *raw, const float *kur)
{
    return copy_bandpass(h, ant, (float *)raw, (float *)kur, hipMemcpyHostToDevice);      // (read only, in this direction)
}
