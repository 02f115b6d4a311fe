// pb_process: the per-call kernel sequence that replaces the segment loop body of src/process_baseband.cu:1108-1376, as
// a graph over the handle's streams (main, s_kur, s_det, s_copy) in three phases: flagging (kurtosis pass, row weights,
// PFB history), the transform, detect + copy-out.  DESIGN.md section 4.3a describes the graph; tests/test_gpu_schedules.py
// runs every branch of it to the same bytes.
#include "pb_internal.h"

static int exec_fft(pb_handle *h, int nseg)
{
    const long batch = (long)nseg * 2 * h->R;
    hipfftHandle plan;
    auto it = h->plans.find(batch);
    if (it == h->plans.end()) {
        int n[1] = {PB_NFFT};
        hipfftResult r = hipfftPlanMany(&plan, 1, n, nullptr, 1, PB_NFFT, nullptr, 1, PB_NCHAN, HIPFFT_R2C, (int)batch);
        if (r != HIPFFT_SUCCESS) return fail(h, PB_EHIP, "hipfftPlanMany failed: " + std::to_string((int)r));
        r = hipfftSetStream(plan, h->stream);
        if (r != HIPFFT_SUCCESS) return fail(h, PB_EHIP, "hipfftSetStream failed");
        h->plans[batch] = plan;
    } else {
        plan = it->second;
    }
    const size_t in_ant = (size_t)h->S * 2 * h->seg_samples;
    const size_t x_ant = (size_t)h->S * 2 * h->R * PB_NCHAN;
    const pb_handle::BufSet &b = h->set();
    for (int a = 0; a < h->A; ++a) {
        if (h->cfg.rfi_mode != 1) {
            hipfftResult r = hipfftExecR2C(plan, b.d_fraw.p + a * in_ant, (hipfftComplex *)(b.d_Xraw.p + a * x_ant));
            if (r != HIPFFT_SUCCESS) return fail(h, PB_EHIP, "hipfftExecR2C failed: " + std::to_string((int)r));
        }
        if (h->cfg.rfi_mode != 0) {
            hipfftResult r = hipfftExecR2C(plan, b.d_fkur.p + a * in_ant, (hipfftComplex *)(b.d_Xkur.p + a * x_ant));
            if (r != HIPFFT_SUCCESS) return fail(h, PB_EHIP, "hipfftExecR2C failed: " + std::to_string((int)r));
        }
    }
    return PB_OK;
}

// Every plane the configured RFI mode / FFT back end launches kernels on exists in the selected buffer set: a
// launcher never dereferences a stream's buffers that pb_create did not allocate (modes 0 / 1 have one stream).
static int check_planes(pb_handle *h)
{
    const bool hipfft = h->cfg.fft_backend == PB_FFT_HIPFFT;
    const bool need_raw = h->cfg.rfi_mode != 1, need_kur = h->cfg.rfi_mode != 0;
    const pb_handle::BufSet &b = h->set();
    bool ok = b.d_in.p && b.d_flags.p && b.d_wrow.p && b.d_codes.p && b.h_codes.p && h->d_bp.p;
    if (need_raw) ok = ok && b.d_Praw.p && (!hipfft || (b.d_fraw.p && b.d_Xraw.p));
    if (need_kur) ok = ok && b.d_Pkur.p && (!hipfft || (b.d_fkur.p && b.d_Xkur.p));
    if (h->cfg.keep_ave) ok = ok && b.d_ave.p;
    if (h->cfg.taps == 4) ok = ok && h->d_hist_in.p && h->d_hist_flags.p && h->d_hist_valid.p && h->d_tapE.p;
    return ok ? PB_OK : fail(h, PB_ESTATE, "pb_process: a buffer of the selected set is missing for this RFI mode / back end");
}

// the batch's filterbank bytes of every antenna, of the streams the RFI mode produces, to the set's pinned mirror
static hipError_t copy_out_codes(pb_handle *h, const pb_handle::BufSet &b, int nseg, hipStream_t st)
{
    hipError_t e = hipSuccess;
    for (int a = 0; a < h->A && e == hipSuccess; ++a)
        for (int str = 0; str < 2 && e == hipSuccess; ++str) {
            if (str == 0 ? h->cfg.rfi_mode == 1 : h->cfg.rfi_mode == 0) continue;
            const size_t o = ((size_t)a * 2 + str) * h->S * h->trim;
            e = launch_copy_out(h->sched, b.h_codes.p + o, b.d_codes.p + o, (size_t)nseg * h->trim, st);
        }
    return e;
}

// ---- phase 1: flagging.  On return the main stream is ordered behind everything the transform reads.
static hipError_t queue_flagging(pb_handle *h, pb_handle::BufSet &b, int nseg)
{
    const bool hipfft = h->cfg.fft_backend == PB_FFT_HIPFFT;
    // The kurtosis pass only needs the raw bytes, and it is a light memory/LDS kernel while
    // detect of the PREVIOUS batch is a latency-bound one that leaves the CUs mostly idle: when
    // the previous batch used another buffer set, run kurtosis on its own stream, released as
    // soon as the previous channeliser has finished, i.e. beside the previous detect.
    const bool fused = pb_fused_kurtosis(h);     // the channeliser flags its own rows: nothing to launch here
    const bool overlap = !fused && !hipfft && h->sets.size() >= 2 && h->last_set >= 0 && h->last_set != h->cur_set;
    hipStream_t s_kur = h->s_kur.s;
    hipError_t e = hipSuccess;
    {
        StreamScope on(h, overlap ? s_kur : h->stream);   // the overlap path: the kurtosis stage goes to s_kur
        if (overlap) {
            // Three or more buffer sets: the kurtosis pass of this batch touches nothing the previous batch's
            // channeliser uses (another set; the PFB history kernel behind it waits for that channeliser itself),
            // so it does not wait for that channeliser and runs beside it -- taps = 4: 0.990 -> 0.965 ms per second
            // of data, the two-kernel taps = 1 path 0.660 -> 0.623 (same box, alternating).  With two sets this
            // set's flags and weights are still being read by the previous batch's channeliser's successor, detect,
            // until ev_chan; the wait for the channeliser keeps the kurtosis pass beside that detect.
            // PB_KUR_EARLY=0 restores the wait.
            if (!(h->sched.kur_early && h->sets.size() >= 3)) e = hipStreamWaitEvent(s_kur, h->ev_fftdone.e, 0);
            if (e == hipSuccess) e = hipStreamWaitEvent(s_kur, b.ev_chan.e, 0);  // flags / weights of this set free (its detect is done)
        } else if (h->sets.size() >= 2 && (h->staged || !fused)) {
            // staging went to s_kur: the main stream must see it.  (Nothing staged since the last call -- the
            // caller writes the input buffers itself, pb_input_dev -- and nothing queued on s_kur: no event pair,
            // a cross-stream dependency costs the command processor ~10-25 us even when it is already met.)
            e = hipEventRecord(h->ev_kur.e, s_kur);
            if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, h->ev_kur.e, 0);
        }
        h->staged = false;
        if (e == hipSuccess && !fused) {
            {
                StageTimer t(h, PB_ST_KURTOSIS);
                // (PB_SKIP & 4, PB_EXPERIMENTS builds only: only once the set holds the flags of the same input from an
                //  earlier call -- the experiment re-processes one second of data, and without flags there would be no
                //  excised transforms either)
                if (!((pb_skip_mask() & 4) && b.processed > 0)) e = launch_kurtosis_flag(h, nseg, hipfft);
                t.stop();
            }
            // taps = 4: the weights read the flags of the previous batch's last rows (history slot hist_rd, filled by
            // that batch's history kernel earlier on this stream).
            // ... or on the main stream, when that batch was not on the overlap path (the first batch, a batch that
            // repeated its set): ev_hist, recorded behind every history kernel on whichever stream ran it, orders the
            // weights behind it either way (free when both are on this stream).
            if (e == hipSuccess && h->cfg.taps == 4) e = hipStreamWaitEvent(h->stream, h->ev_hist.e, 0);
            if (e == hipSuccess) e = launch_pfb_weights(h, nseg);
            if (e == hipSuccess && h->cfg.taps == 4) {
                // The channeliser only needs what has been queued up to here: release it now.  Then keep this
                // batch's last three rows and flags for the next one in the OTHER history slot -- the one the
                // previous batch's channeliser reads, hence behind it (ev_fftdone still holds its record); the next
                // batch's weights and staging follow on this stream, its channeliser behind them.  (Round 2 ran the
                // history kernel behind the channeliser on the main stream and the next weights behind THAT: two
                // cross-stream hand-overs between consecutive channelisers.)
                if (overlap) e = hipEventRecord(h->ev_kur.e, s_kur);
                if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, h->ev_fftdone.e, 0);
                if (e == hipSuccess) e = launch_pfb_history(h, nseg);
                if (e == hipSuccess) e = hipEventRecord(h->ev_hist.e, h->stream);
            }
        }
        if (overlap && e == hipSuccess && h->cfg.taps != 4) e = hipEventRecord(h->ev_kur.e, s_kur);
    }
    if (overlap && e == hipSuccess) e = hipStreamWaitEvent(h->stream, h->ev_kur.e, 0);
    return e;
}

// ---- phase 2: the transform, on the main stream
static int queue_transform(pb_handle *h, int nseg, int inject_now)
{
    if (h->cfg.fft_backend == PB_FFT_HIPFFT) {
        StageTimer t(h, PB_ST_FFT);
        if (int rc = exec_fft(h, nseg)) return rc;
        t.stop();
        if (inject_now > 0) {
            StageTimer ti(h, PB_ST_INJECT);
            HIPCHK(h, launch_inject_c64(h, nseg, inject_now));
            ti.stop();
        }
    } else {
        StageTimer t(h, PB_ST_CHANNELIZE);
        if (!(pb_skip_mask() & 1))
            HIPCHK(h, h->cfg.taps == 4 ? launch_channelize_pfb(h, nseg, inject_now) : launch_channelize(h, nseg, inject_now));
        t.stop();
    }
    return PB_OK;
}

// ---- phase 3: detect on stream sd, then the copy-out of its bytes on stream sc, which is always another one: behind
// detect on the same stream the copy-out would hold up the next batch's detect whenever it is slow (many antennas, few
// copy workgroups).  What the two paths of pb_process really do differently is in the last two arguments:
//   wait_fftdone          sd is not the main stream, so detect has to be told that the transform is done
//   alldone_behind_copy   ev_alldone -- the whole batch, what refilling this set (pb_stage.hip: submit_stream) and
//                         pb_reset_bandpass wait for -- is recorded behind the copy-out on sc; without it behind detect
//                         on sd, and the copy-out is covered by the set's ev_det alone
static int queue_detect_and_copy_out(pb_handle *h, pb_handle::BufSet &b, int nseg, int inject_now, hipStream_t sd,
                                     hipStream_t sc, bool wait_fftdone, bool alldone_behind_copy)
{
    if (wait_fftdone) HIPCHK(h, hipStreamWaitEvent(sd, h->ev_fftdone.e, 0));
    HIPCHK(h, hipStreamWaitEvent(sd, b.ev_det.e, 0));  // this set's previous bytes have left
    HIPCHK(h, hipStreamWaitEvent(sd, b.ev_cl.e, 0));   // planes of this set were summed
    {
        StreamScope on(h, sd);
        StageTimer t(h, PB_ST_DETECT);
        if (!(pb_skip_mask() & 2)) HIPCHK(h, launch_detect(h, nseg, inject_now));
        t.stop();
    }
    HIPCHK(h, hipEventRecord(b.ev_chan.e, sd));        // this set's kernels are done
    if (!alldone_behind_copy) HIPCHK(h, hipEventRecord(h->ev_alldone.e, sd));
    HIPCHK(h, hipStreamWaitEvent(sc, b.ev_chan.e, 0));
    HIPCHK(h, copy_out_codes(h, b, nseg, sc));
    HIPCHK(h, hipEventRecord(b.ev_det.e, sc));
    if (alldone_behind_copy) HIPCHK(h, hipEventRecord(h->ev_alldone.e, sc));
    return PB_OK;
}

extern "C" int pb_process(pb_handle *h, int nseg, int inject_now)
{
    if (!h) return PB_EINVAL;
    if (nseg < 1 || nseg > h->S) return fail(h, PB_EINVAL, "pb_process: nseg out of range");
    if (int rc = check_planes(h)) return rc;
    if (!h->cfg.inject_frb) inject_now = 0;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // What this batch's first kernels overwrite -- the set's flags, weights and power planes -- was last read by the
    // set's previous detect (ev_chan).  The copy-out of that batch's bytes (ev_det) only has to have drained before
    // THIS batch's detect overwrites the code buffer: waiting for it here held the channeliser back by ~0.1 ms per
    // step once the kurtosis pass in front of it was gone (dispatch timeline, profiles/r03_notes.md).
    pb_handle::BufSet &b = h->set();
    HIPCHK(h, hipStreamWaitEvent(h->stream, b.ev_chan.e, 0));
    HIPCHK(h, queue_flagging(h, b, nseg));
    if (int rc = queue_transform(h, nseg, inject_now)) return rc;
    HIPCHK(h, hipEventRecord(h->ev_fftdone.e, h->stream));
    if (h->cfg.taps == 4) h->hist_rd ^= 1;       // the next batch reads what this batch's history kernel has kept
    h->last_set = h->cur_set;
    // With two or more buffer sets, detect + D2H of this batch run on the second stream so that they
    // overlap the NEXT batch's kurtosis and channeliser.  Detect is latency-bound on its serial
    // bandpass wave (one 48 KB workgroup per CU), the channeliser VALU-bound: side by side the step is
    // ~9 % shorter than back to back (0.915 vs 1.007 ms per second of data; PB_OVERLAP_DETECT=0 turns
    // it off).  With one buffer set detect stays on the main stream and only the copy-out leaves it, for s_det.
    const bool beside = h->sched.overlap_detect && h->sets.size() >= 2 && h->cfg.fft_backend != PB_FFT_HIPFFT;
    if (int rc = beside ? queue_detect_and_copy_out(h, b, nseg, inject_now, h->s_det.s, h->s_copy.s, true, true)
                        : queue_detect_and_copy_out(h, b, nseg, inject_now, h->stream, h->s_det.s, false, false))
        return rc;
    b.processed = nseg;
    return PB_OK;
}
