// The host side of a call that runs beside the pipeline: on a stream of its own, in timed stages, on device buffers it
// owns, back when its outputs have reached the host.  The correlator, the beamformer and the imager are such jobs: their
// state derives from PbJob<stages>, holds its buffers as DevBuf members (pb_own.h) and is freed by job_free.
#pragma once
#include "pb_internal.h"

#include <cmath>

// a non-blocking stream, N stages between N + 1 events, and the stages' device times of the last call
template <int N>
struct PB_LOCAL PbJob {
    hipStream_t st = nullptr;
    hipEvent_t ev[N + 1] = {};
    float ms[N] = {};
    hipError_t ensure(int device)      // the device current; the stream and the events made by the first call
    {
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess && !st) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        for (hipEvent_t &x : ev)
            if (e == hipSuccess && !x) e = hipEventCreate(&x);
        return e;
    }
    hipError_t mark(int k) { return hipEventRecord(ev[k], st); }      // stage k - 1 ends and stage k begins here
    hipError_t launched(int k) { hipError_t e = hipGetLastError(); return e == hipSuccess ? mark(k) : e; }   // behind kernels
    hipError_t finish()      // the last stage ends; wait for the stream; ms[k] = the time between marks k and k + 1
    {
        hipError_t e = mark(N);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        for (int k = 0; k < N && e == hipSuccess; ++k) e = hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
        return e;
    }
};

// what a job's free function is (its device current; s = nullptr: never used): the stream drained, then all of it gone
template <class S>
static void job_free(S *&s)
{
    if (!s) return;
    if (s->st) { (void)hipStreamSynchronize(s->st); (void)hipStreamDestroy(s->st); }
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
    s = nullptr;
}

// ---- what the calls that read a handle's spectra refuse (pb_correlate, pb_correlate_gated, pb_beamform), under the
// call's name w.  In two parts, because the beamformer judges its own arguments between them.
#define PB_SPECTRA_MAX_ANT 8

// the handle keeps `stream`'s spectra and nseg can be a number of segments
static inline int spectra_check_config(pb_handle *h, const std::string &w, int stream, int nseg)
{
    if (!h->cfg.coherence) return fail(h, PB_EINVAL, w + ": the handle keeps no spectra (needs coherence = 1)");
    if (h->A > PB_SPECTRA_MAX_ANT) return fail(h, PB_EINVAL, w + ": at most 8 antennas");
    if (stream != PB_CORR_RAW && stream != PB_CORR_KUR) return fail(h, PB_EINVAL, w + ": stream must be 0 (raw) or 1 (excised)");
    if ((stream == PB_CORR_RAW && h->cfg.rfi_mode == 1) || (stream == PB_CORR_KUR && h->cfg.rfi_mode == 0))
        return fail(h, PB_EINVAL, w + ": the handle's rfi_mode does not produce that stream");
    if (nseg < 1) return fail(h, PB_EINVAL, w + ": nseg must be positive");
    return PB_OK;
}

// the selected set's last pb_process left nseg segments of them
static inline int spectra_check_batch(pb_handle *h, const std::string &w, int nseg)
{
    if (h->set().processed < 1) return fail(h, PB_ESTATE, w + ": no pb_process on the selected set yet");
    if (nseg > h->set().processed) return fail(h, PB_ESTATE, w + ": more segments than the set's last pb_process processed");
    return PB_OK;
}

static inline bool job_output_fits(size_t bytes) { return bytes <= ((size_t)2 << 30); }      // a call's outputs: 2 GiB
// a delay in samples is finite and within 2^24; its phase slope in turns per channel
static inline bool delay_ok(double d) { return std::isfinite(d) && std::fabs(d) <= 16777216.0; }
static inline double delay_slope(double d) { return d / PB_NFFT; }
