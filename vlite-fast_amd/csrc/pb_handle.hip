// C ABI of libpb_hip.so (include/pb_hip.h), the handle itself: configuration, pb_create / pb_destroy, the main stream,
// errors.  No CPU fallback exists: every entry point needs a HIP device.  The other concerns that share the handle:
// pb_tables.hip (constant tables), pb_stage.hip (input staging, bandpass, history), pb_process.hip (the stream graph of
// one batch), pb_fetch.hip (read-back, stage timers); beside them pb_coadd.hip, the array jobs and search_*.hip.
// What they share is in pb_internal.h, what owns the handle's resources in pb_own.h.  EVERY read of the environment and
// every `#if PB_EXPERIMENTS` is in this file: the experiments library differs from the shipped one in this one object.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pb_internal.h"

static std::string g_create_err;

hipError_t sync_all(pb_handle *h)
{
    hipError_t e = hipStreamSynchronize(h->stream);
    for (hipStream_t s : {h->s_det.s, h->s_copy.s, h->s_kur.s, h->s_coadd})
        if (e == hipSuccess && s) e = hipStreamSynchronize(s);
    return e;
}

int fail(pb_handle *h, int code, const std::string &msg)
{
    if (h) h->err = msg;
    else g_create_err = msg;
    return code;
}

extern "C" const char *pb_version(void) { return "pb_hip 0.1 (gfx950)"; }

// Launches left out on request -- RESULTS INVALID -- for the energy / upper-bound measurements of tools/energy_probe.py,
// tools/taps1_unfused_bound.sh and tools/pfb_fused_ab.sh: bit 0 the channeliser, bit 1 detect, bit 2 the kurtosis pass.
// Compiled only into the experiments build (`make exp` -> libpb_hip_exp.so, -DPB_EXPERIMENTS=1, selected with
// PB_LIBPATH): the shipped library does not read the variable and cannot be talked into skipping a kernel.
int pb_skip_mask()
{
#if PB_EXPERIMENTS
    static const int skip = getenv("PB_SKIP") ? atoi(getenv("PB_SKIP")) : 0;
    return skip;
#else
    return 0;
#endif
}

static int env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

#ifdef FFT_LEAN
// variant builds of the lean channeliser only (tools/lean_prio_emulation.sh): its dynamic LDS, in bytes
int pb_lean_lds(int dflt) { return env_int("PB_LEAN_LDS", dflt); }
#endif

PbSched pb_read_sched()
{
    PbSched s;
    s.overlap_detect = env_int("PB_OVERLAP_DETECT", 1);
    s.kur_early = env_int("PB_KUR_EARLY", 1);
    s.detect_depth = env_int("PB_DETECT_DEPTH", 0);
    // switches that only ever served one timing experiment each are read by the experiments build alone
    s.copy_dma = 0;
    s.copy_wgs = 8;
    s.det_cus = 0;
    s.det_prio = 1;
#if PB_EXPERIMENTS
    s.copy_dma = env_int("PB_COPY_DMA", 0);
    s.copy_wgs = env_int("PB_COPY_WGS", 8);
    s.det_cus = env_int("PB_DET_CUS", 0);
    s.det_prio = env_int("PB_DET_PRIO", 1);
#endif
    return s;
}

bool pb_fused_kurtosis(const pb_handle *h)
{
    // h->fuse (PB_FUSE_KURTOSIS when the handle was created): 0 never, 1 (default) the rectangular window.  taps = 4
    // keeps kurtosis pass + weights + channeliser: a channeliser that flags its own rows was built in round 4, was
    // bit-exact and 17 % SLOWER (profiles/r04_notes.md section 10) and left the library in round 5
    // (tools/experiments/k_channelize_pfb_kur.patch).
    if (h->fuse < 1 || h->cfg.taps != 1) return false;
    return h->cfg.fft_backend == PB_FFT_LDS && h->cfg.rfi_mode != 0 && !h->cfg.debug_keep;
}

// (the caller's memory, not the handle's: the one hipHostFree outside pb_own.h)
extern "C" void *pb_host_alloc(size_t nbytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, nbytes ? nbytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

extern "C" void pb_host_free(void *p) { if (p) (void)hipHostFree(p); }

extern "C" void pb_config_default(pb_config *c)
{
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c;      // (device 0; inject_frb, keep_ave, debug_keep, coherence off: the memset)
    c->nant = 1;
    c->nbit = 2;        // reference default NBIT, src/process_baseband.cu:31,54
    c->npol = 1;
    c->rfi_mode = 2;    // :351
    c->taps = 1;
    c->fft_backend = PB_FFT_LDS;
    c->rows_per_seg = 1024;
    c->max_seg = 10;
    c->nsets = 1;
}

static int create_impl(pb_handle *h)
{
    const pb_config &c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device));
    HIPCHK(h, hipStreamCreateWithFlags(&h->s_main.s, hipStreamNonBlocking));
    h->stream = h->s_main.s;
    {
        // detect is latency-bound and small (one workgroup per CU): give its stream the highest
        // priority so that its workgroups slot in between the channeliser's as CUs free up
        int lo = 0, hi = 0;
        HIPCHK(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
        // timing experiments: PB_DET_CUS=n confines detect to n CUs of every 32 (a CU mask on its stream), so that
        // its workgroups pack three to a CU there instead of taking one channeliser slot on every CU
        const int det_cus = h->sched.det_cus;
        if (det_cus > 0 && det_cus < 32) {
            uint32_t mask[8];
            for (int i = 0; i < 8; ++i) mask[i] = (1u << det_cus) - 1u;
            HIPCHK(h, hipExtStreamCreateWithCUMask(&h->s_det.s, 8, mask));
        } else {
            // (PB_DET_PRIO=0: detect's stream at the default priority; timing experiments)
            HIPCHK(h, hipStreamCreateWithPriority(&h->s_det.s, hipStreamNonBlocking, h->sched.det_prio ? hi : lo));
        }
    }
    HIPCHK(h, hipStreamCreateWithFlags(&h->s_kur.s, hipStreamNonBlocking));
    HIPCHK(h, hipStreamCreateWithFlags(&h->s_copy.s, hipStreamNonBlocking));
    for (Event *ev : {&h->ev_fftdone, &h->ev_kur, &h->ev_hist, &h->ev_alldone}) HIPCHK(h, ev->create());
    const size_t A = h->A, S = h->S, R = h->R;
    const size_t in_elems = A * S * 2 * h->seg_samples;
    HIPCHK(h, h->d_bp.grow(h, A * 2 * 2 * PB_NCHANOUT));
    HIPCHK(h, hipMemset(h->d_bp.p, 0, A * 2 * 2 * PB_NCHANOUT * sizeof(float)));  // :702,708
    // One buffer set per pipeline slot (cfg.nsets): while detect + D2H of one batch run on the
    // second stream, kurtosis + channeliser of the next batch fill the other set.
    h->sets = std::vector<pb_handle::BufSet>(c.nsets);
    for (pb_handle::BufSet &b : h->sets) {
        HIPCHK(h, b.d_in.grow(h, in_elems + 64));   // + overhang of the channeliser's 16-byte row loads
        HIPCHK(h, b.d_flags.grow(h, A * S * h->nblk_seg));
        HIPCHK(h, hipMemset(b.d_flags.p, 0, A * S * h->nblk_seg));
        HIPCHK(h, b.d_wrow.grow(h, 2 * A * S * R));   // weights, then the rows' flag masks (pb_rowmask)
        HIPCHK(h, hipMemset(b.d_wrow.p + A * S * R, 0, A * S * R * sizeof(uint32_t)));
        {
            // rfi_mode 0 never computes weights: every row counts fully
            std::vector<float> ones(A * S * R, 1.0f);
            HIPCHK(h, hipMemcpy(b.d_wrow.p, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        if (c.debug_keep) HIPCHK(h, b.d_stats.grow(h, A * 6 * S * h->nblk_seg + A * 5 * S * R));
        const bool need_raw = c.rfi_mode != 1, need_kur = c.rfi_mode != 0;
        if (c.fft_backend == PB_FFT_HIPFFT) {
            if (need_raw) HIPCHK(h, b.d_fraw.grow(h, in_elems));
            if (need_kur) HIPCHK(h, b.d_fkur.grow(h, in_elems));
            const size_t xn = A * S * 2 * R * PB_NCHAN;
            if (need_raw) HIPCHK(h, b.d_Xraw.grow(h, xn));
            if (need_kur) HIPCHK(h, b.d_Xkur.grow(h, xn));
        }
        {
            // power planes: written by the LDS channeliser, or from the complex spectra of hipFFT; coherence output:
            // the complex in-band spectra (float2) in their place
            const size_t pn = A * S * 2 * R * PB_NCHANOUT * (c.coherence ? 2 : 1);
            if (need_raw) HIPCHK(h, b.d_Praw.grow(h, pn));
            if (need_kur) HIPCHK(h, b.d_Pkur.grow(h, pn));
        }
        HIPCHK(h, b.d_codes.grow(h, A * 2 * S * h->trim));
        HIPCHK(h, hipMemset(b.d_codes.p, 0, A * 2 * S * h->trim));
        HIPCHK(h, b.h_codes.grow(A * 2 * S * h->trim));
        memset(b.h_codes.p, 0, A * 2 * S * h->trim);
        if (c.keep_ave) {
            HIPCHK(h, b.d_ave.grow(h, A * 2 * S * h->ave_per_seg));
            HIPCHK(h, hipMemset(b.d_ave.p, 0, A * 2 * S * h->ave_per_seg * sizeof(float)));
        }
        for (Event *ev : {&b.ev_chan, &b.ev_det, &b.ev_cl}) HIPCHK(h, ev->create());
    }
    if (c.inject_frb) {
        // DM of 80, 2 ms, amplitude 1.05: src/process_baseband.cu:717,1238-1239
        if (int rc = set_frb(h, 80.f, -1.f, 1.05f)) return rc;
    }
    if (int rc = build_fft_tables(h)) return rc;
    if (c.taps == 4)
        if (int rc = build_pfb_history(h)) return rc;
    // (PB_DAG_BANDS=0, a test hook: the flag decision without the bands on purpose -- tests/test_gpu_parity.py checks
    // that the flags stay bit-exact)
    return build_dag(h, env_int("PB_DAG_BANDS", 1) != 0);
}

extern "C" int pb_create(const pb_config *cfg, pb_handle **out)
{
    if (!cfg || !out) return fail(nullptr, PB_EINVAL, "pb_create: null argument");
    *out = nullptr;
    // a caller built against the header before `coherence` was appended passes the shorter struct: the fields it
    // does not have take their defaults (0)
    const size_t before_coherence = offsetof(pb_config, coherence);
    if (cfg->struct_size != sizeof(pb_config) && cfg->struct_size != before_coherence)
        return fail(nullptr, PB_EINVAL, "pb_create: pb_config size mismatch");
    pb_config grown;
    memset(&grown, 0, sizeof grown);
    memcpy(&grown, cfg, cfg->struct_size);
    grown.struct_size = sizeof grown;
    const pb_config &c = grown;
    if (!(c.nbit == 2 || c.nbit == 4 || c.nbit == 8)) return fail(nullptr, PB_EINVAL, "Unsupported NBIT!");
    if (!(c.npol == 1 || c.npol == 2)) return fail(nullptr, PB_EINVAL, "Unsupported npol!");
    if (c.rfi_mode < 0 || c.rfi_mode > 2) return fail(nullptr, PB_EINVAL, "Unsupported RFI mode!");
    if (!(c.taps == 1 || c.taps == 4)) return fail(nullptr, PB_EINVAL, "taps must be 1 or 4");
    if (c.taps == 4 && c.fft_backend != PB_FFT_LDS) return fail(nullptr, PB_EINVAL, "taps=4 needs the LDS FFT back end");
    if (!(c.fft_backend == PB_FFT_LDS || c.fft_backend == PB_FFT_HIPFFT)) return fail(nullptr, PB_EINVAL, "bad fft_backend");
    if (c.nant < 1 || c.max_seg < 1) return fail(nullptr, PB_EINVAL, "nant and max_seg must be >= 1");
    if (c.nsets < 1 || c.nsets > 8) return fail(nullptr, PB_EINVAL, "nsets must be 1..8");
    if (c.rows_per_seg < 8 || c.rows_per_seg % PB_NSCRUNCH) return fail(nullptr, PB_EINVAL, "rows_per_seg must be a positive multiple of 8");
    if (!(c.coherence == 0 || c.coherence == 1)) return fail(nullptr, PB_EINVAL, "coherence must be 0 or 1");
    if (c.coherence) {
        // coherence output: AA, BB, CR, CI; what it is not built for is refused
        if (c.npol != 2) return fail(nullptr, PB_EINVAL, "coherence output needs npol = 2 (-P 2 --coherence)");
        if (c.taps != 1) return fail(nullptr, PB_EINVAL, "coherence output is not implemented for taps = 4 (PFB)");
        if (c.fft_backend != PB_FFT_LDS) return fail(nullptr, PB_EINVAL, "coherence output needs the LDS FFT back end, not hipFFT");
        if (c.debug_keep) return fail(nullptr, PB_EINVAL, "coherence output is not implemented with debug_keep = 1");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, PB_EHIP, "pb_create: no HIP device (libpb_hip has no CPU fallback)");
    if (c.device < 0 || c.device >= ndev) return fail(nullptr, PB_EINVAL, "pb_create: bad device id");

    pb_handle *h = new pb_handle();
    h->cfg = c;
    h->fuse = env_int("PB_FUSE_KURTOSIS", 1);
    h->sched = pb_read_sched();
    h->R = c.rows_per_seg;
    h->S = c.max_seg;
    h->A = c.nant;
    h->seg_samples = (size_t)h->R * PB_NFFT;
    h->nblk_seg = (size_t)h->R * PB_BLK_PER_FFT;
    const int polfac = c.npol == 1 ? 2 : 1;
    h->trim = (size_t)2 * h->R * PB_NCHANOUT / (polfac * PB_NSCRUNCH) / (8 / c.nbit);
    h->ave_per_seg = (size_t)2 * h->R * PB_NCHANOUT / (polfac * PB_NSCRUNCH);
    if (c.coherence) {
        // four products per output sample: [time][AA, BB, CR, CI][4096]
        h->trim = (size_t)4 * (h->R / PB_NSCRUNCH) * PB_NCHANOUT * c.nbit / 8;
        h->ave_per_seg = (size_t)4 * (h->R / PB_NSCRUNCH) * PB_NCHANOUT;
    }
    int rc = create_impl(h);
    if (rc != PB_OK) {
        // whatever create_impl had made by then belongs to a member of the handle, which pb_destroy lets go of
        g_create_err = h->err;
        pb_destroy(h);
        return rc;
    }
    *out = h;
    return PB_OK;
}

extern "C" void pb_destroy(pb_handle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    // Every stream the handle queues work on drains before a buffer goes.  Not s_coadd: it is the caller's, who may
    // have retired it by now.
    for (hipStream_t s : {h->stream, h->s_det.s, h->s_copy.s, h->s_kur.s})
        if (s) (void)hipStreamSynchronize(s);
    pb_correlate_free(h);
    pb_correlate_track_free(h);
    pb_beamform_free(h);
    pb_beam_plane_free(h);
    for (auto &kv : h->plans) hipfftDestroy(kv.second);
    drain_timers(h);
    delete h;      // buffers and events, then the streams: the order of pb_handle's members
}

extern "C" const char *pb_last_error(const pb_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" int pb_query(const pb_handle *h, pb_sizes *o)
{
    if (!h || !o) return PB_EINVAL;
    o->seg_samples_per_pol = h->seg_samples;
    o->input_bytes_per_seg = 2 * h->seg_samples;
    o->code_bytes_per_seg = h->trim;
    o->ave_floats_per_seg = h->ave_per_seg;
    o->rows_per_seg = h->R;
    o->blocks_per_seg_pol = h->nblk_seg;
    o->device_bytes = h->device_bytes;
    return PB_OK;
}

extern "C" int pb_set_stream(pb_handle *h, void *s)
{
    if (!h) return PB_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, sync_all(h));
    HIPCHK(h, h->s_main.destroy());      // (the handle's own, if the main stream was that)
    if (!s) HIPCHK(h, hipStreamCreateWithFlags(&h->s_main.s, hipStreamNonBlocking));
    h->stream = s ? (hipStream_t)s : h->s_main.s;
    for (auto &kv : h->plans) hipfftSetStream(kv.second, h->stream);
    return PB_OK;
}

extern "C" int pb_sync(pb_handle *h)
{
    if (!h) return PB_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, sync_all(h));
    return PB_OK;
}

extern "C" int pb_select_set(pb_handle *h, int set)
{
    if (!h) return PB_EINVAL;
    if (set < 0 || set >= (int)h->sets.size()) return fail(h, PB_EINVAL, "pb_select_set: no such buffer set");
    h->cur_set = set;
    return PB_OK;
}
