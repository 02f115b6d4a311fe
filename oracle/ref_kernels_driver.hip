/*
 * ref_kernels_driver.hip -- host entry points that launch the REFERENCE's own kernels.
 *
 * TEST INFRASTRUCTURE ONLY.  oracle/ref_kernels.mk links this file with the reference's
 * src/pb_kernels.cu (compiled as it lies, behind oracle/ref_shim/cufft.h) into
 * oracle/_ref/libref_kernels.so and libref_kernels_fmad.so.  This file holds no kernel: every
 * __global__ it launches is the reference's, declared by src/process_baseband.h, which is included
 * for those prototypes and for nothing else -- the sizes below are restated and checked against the
 * header by static_assert.
 *
 * What is restated here, because src/process_baseband.cu cannot be compiled: the launch sites.
 * Each launch carries the reference's grid and block with its line beside it
 * (src/process_baseband.cu:717, :1152-1352), `nsms` is the device's multiProcessorCount as at :474-475,
 * and every buffer has the size of the reference's allocation (:578-709) for the given rows per
 * segment, so that no kernel reads past what the reference gives it.
 *
 * Every refk_* entry point: hipMalloc, hipMemset to zero, upload, launch(es), download, free.
 * It returns 0, or the hipError_t of the first HIP call that failed (nothing later runs), or
 * -1 for arguments the reference's shapes do not allow.
 */
#include "process_baseband.h"

#include <stddef.h>
#include <stdint.h>

#define REFK_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int K_NTHREAD = 512;
constexpr int K_NFFT = 12500;
constexpr int K_NCHAN = 6251;
constexpr int K_NSCRUNCH = 8;
constexpr int K_NKURTO = 500;
constexpr int K_ROWS = 1024;                 /* FFTS_PER_SEG: fixed INSIDE the spectral kernels */
constexpr int K_NCHANOUT = 4096;
constexpr int K_VLITE_RATE = 128000000;
static_assert(K_NTHREAD == NTHREAD && K_NFFT == NFFT && K_NCHAN == NCHAN && K_NSCRUNCH == NSCRUNCH, "header moved");
static_assert(K_NKURTO == NKURTO && K_ROWS == (FFTS_PER_SEG) && K_NCHANOUT == CHANMAX - CHANMIN + 1, "header moved");
static_assert(K_VLITE_RATE == VLITE_RATE && K_VLITE_RATE / 10 / K_NFFT == K_ROWS, "header moved");

struct Buf {
    void *p = nullptr;
    ~Buf() { if (p) (void)hipFree(p); }          /* only on an early return; the normal path calls release() */
    hipError_t alloc0(size_t bytes)
    {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        if (e != hipSuccess) { p = nullptr; return e; }
        return hipMemset(p, 0, bytes ? bytes : 1);
    }
    hipError_t upload(const void *h, size_t bytes)
    {
        hipError_t e = alloc0(bytes);
        if (e != hipSuccess) return e;
        return hipMemcpy(p, h, bytes, hipMemcpyHostToDevice);
    }
    hipError_t download(void *h, size_t bytes) const
    {
        return h ? hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost) : hipSuccess;
    }
    hipError_t release()
    {
        void *q = p;
        p = nullptr;
        return q ? hipFree(q) : hipSuccess;
    }
    float *f() const { return (float *)p; }
    cufftComplex *c() const { return (cufftComplex *)p; }
    unsigned char *u() const { return (unsigned char *)p; }
};

#define TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
/* after a launch: the launch's own status (src/process_baseband.cu's cudaGetLastError), then the kernel's */
#define LAUNCHED() do { TRY(hipGetLastError()); TRY(hipDeviceSynchronize()); } while (0)

hipError_t get_nsms(int *nsms)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    return hipDeviceGetAttribute(nsms, hipDeviceAttributeMultiprocessorCount, dev);   /* :474-475 */
}

/* shapes of src/process_baseband.cu:593-595, :618 for `rows` filterbank rows per pol and segment */
struct TimeShape {
    size_t samps_per_chunk, nkurto_per_chunk;
    int fft_per_chunk;
    explicit TimeShape(int rows)
        : samps_per_chunk(2 * (size_t)rows * K_NFFT), nkurto_per_chunk(samps_per_chunk / K_NKURTO), fft_per_chunk(2 * rows) {}
};

bool time_rows_ok(int rows) { return rows > 0 && rows <= 4096 && (2 * rows) % 8 == 0; }   /* block_kurtosis: 8 rows a block */

constexpr size_t SPEC_ELEMS = (size_t)2 * K_ROWS * K_NCHAN;     /* fft_per_chunk*NCHAN, :604 */
constexpr int FFT_PER_CHUNK = 2 * K_ROWS;

size_t scrunch_elems(int npol) { return SPEC_ELEMS / ((npol == 1 ? 2 : 1) * K_NSCRUNCH); }              /* :657-658 */
size_t trim_bytes(int npol, int nbit)                                                                    /* :667, :675 */
{
    return (size_t)FFT_PER_CHUNK * K_NCHANOUT / ((npol == 1 ? 2 : 1) * K_NSCRUNCH) / (8 / nbit);
}

}  // namespace

REFK_API int refk_nsms(int *nsms)
{
    TRY(get_nsms(nsms));
    return 0;
}

/* ------------------------------------------------------------------ time domain, K1-K5 */

REFK_API int refk_convertarray(float *time, const unsigned char *utime, size_t n)
{
    int nsms;
    TRY(get_nsms(&nsms));
    Buf u, t;
    TRY(u.upload(utime, n));
    TRY(t.alloc0(sizeof(float) * n));
    convertarray<<<nsms * 32, K_NTHREAD>>>(t.f(), u.u(), n);                       /* :1152 */
    LAUNCHED();
    TRY(t.download(time, sizeof(float) * n));
    TRY(u.release());
    TRY(t.release());
    return 0;
}

/* time: nkurto blocks of 500 samples; pow, kur: nkurto entries each */
REFK_API int refk_kurtosis(const float *time, float *pow, float *kur, size_t nkurto)
{
    if (nkurto == 0 || nkurto > 2 * (size_t)4096 * 25) return -1;
    Buf t, pk;
    TRY(t.upload(time, sizeof(float) * nkurto * K_NKURTO));
    TRY(pk.alloc0(2 * sizeof(float) * nkurto));                                    /* :626, kur_dev = pow_dev + nkurto :629 */
    kurtosis<<<(unsigned)nkurto, 256>>>(t.f(), pk.f(), pk.f() + nkurto);           /* :1167 */
    LAUNCHED();
    TRY(hipMemcpy(pow, pk.f(), sizeof(float) * nkurto, hipMemcpyDeviceToHost));
    TRY(hipMemcpy(kur, pk.f() + nkurto, sizeof(float) * nkurto, hipMemcpyDeviceToHost));
    TRY(t.release());
    TRY(pk.release());
    return 0;
}

/* kur, dag: 2*n entries (both pols); which = 0: compute_dagostino, 1: compute_dagostino2 */
static int dagostino(const float *kur, float *dag, size_t n, int which)
{
    int nsms;
    TRY(get_nsms(&nsms));
    Buf k, d;
    TRY(k.upload(kur, sizeof(float) * 2 * n));
    TRY(d.alloc0(sizeof(float) * 2 * n));
    if (which == 0)
        compute_dagostino<<<nsms * 32, K_NTHREAD>>>(k.f(), d.f(), n);              /* :1173, n = nkurto_per_chunk/2 */
    else
        compute_dagostino2<<<nsms * 32, K_NTHREAD>>>(k.f(), d.f(), n);             /* :1183, n = fft_per_chunk/2 */
    LAUNCHED();
    TRY(d.download(dag, sizeof(float) * 2 * n));
    TRY(k.release());
    TRY(d.release());
    return 0;
}

REFK_API int refk_compute_dagostino(const float *kur, float *dag, size_t n) { return dagostino(kur, dag, n, 0); }
REFK_API int refk_compute_dagostino2(const float *kur, float *dag, size_t n) { return dagostino(kur, dag, n, 1); }

/* pow, kur, dag: 25 * fft_per_chunk entries; pow_fb, kur_fb: fft_per_chunk entries */
REFK_API int refk_block_kurtosis(const float *pow, const float *kur, const float *dag, float *pow_fb, float *kur_fb,
                                 int fft_per_chunk)
{
    if (fft_per_chunk <= 0 || fft_per_chunk % 8 || fft_per_chunk > 8192) return -1;
    const size_t nk = (size_t)fft_per_chunk * (K_NFFT / K_NKURTO);
    Buf pk, d, fb;
    TRY(pk.alloc0(2 * sizeof(float) * nk));
    TRY(hipMemcpy(pk.f(), pow, sizeof(float) * nk, hipMemcpyHostToDevice));
    TRY(hipMemcpy(pk.f() + nk, kur, sizeof(float) * nk, hipMemcpyHostToDevice));
    TRY(d.upload(dag, sizeof(float) * nk));
    TRY(fb.alloc0(2 * sizeof(float) * fft_per_chunk));                             /* :628, kur_fb_dev :630 */
    block_kurtosis<<<fft_per_chunk / 8, 256>>>(pk.f(), pk.f() + nk, d.f(), fb.f(), fb.f() + fft_per_chunk);   /* :1179 */
    LAUNCHED();
    TRY(hipMemcpy(pow_fb, fb.f(), sizeof(float) * fft_per_chunk, hipMemcpyDeviceToHost));
    TRY(hipMemcpy(kur_fb, fb.f() + fft_per_chunk, sizeof(float) * fft_per_chunk, hipMemcpyDeviceToHost));
    TRY(pk.release());
    TRY(d.release());
    TRY(fb.release());
    return 0;
}

/* in, out: 12500 * fft_per_chunk samples; dag: 25 * fft_per_chunk; norms: fft_per_chunk (zeroed here, :1187).
 * inplace != 0: out is the same device buffer as in (RFI mode 1, :606); fake != 0: apply_kurtosis_fake. */
static int apply(const float *in, float *out, const float *dag, float *norms, int fft_per_chunk, int inplace, int fake)
{
    if (fft_per_chunk <= 0 || fft_per_chunk > 8192) return -1;
    const size_t nsamp = (size_t)fft_per_chunk * K_NFFT, nk = nsamp / K_NKURTO;
    Buf i, o, d, fb, w;
    TRY(i.upload(in, sizeof(float) * nsamp));
    if (!inplace) TRY(o.alloc0(sizeof(float) * nsamp));
    TRY(d.upload(dag, sizeof(float) * nk));
    TRY(fb.alloc0(sizeof(float) * fft_per_chunk));                                 /* dag_fb_dev :639; never read (:255-256) */
    TRY(w.alloc0(sizeof(float) * fft_per_chunk));                                  /* :643 and the memset of :1187 */
    float *dst = inplace ? i.f() : o.f();
    if (!fake)
        apply_kurtosis<<<(unsigned)nk, 256>>>(i.f(), dst, d.f(), fb.f(), w.f());   /* :1195 */
    else
        apply_kurtosis_fake<<<(unsigned)nk, 256>>>(i.f(), dst, d.f(), fb.f(), w.f());   /* :1201 */
    LAUNCHED();
    TRY(hipMemcpy(out, dst, sizeof(float) * nsamp, hipMemcpyDeviceToHost));
    TRY(w.download(norms, sizeof(float) * fft_per_chunk));
    TRY(i.release());
    TRY(o.release());
    TRY(d.release());
    TRY(fb.release());
    TRY(w.release());
    return 0;
}

REFK_API int refk_apply_kurtosis(const float *in, float *out, const float *dag, float *norms, int fft_per_chunk, int inplace)
{
    return apply(in, out, dag, norms, fft_per_chunk, inplace, 0);
}

REFK_API int refk_apply_kurtosis_fake(const float *in, float *out, const float *dag, float *norms, int fft_per_chunk,
                                      int inplace)
{
    return apply(in, out, dag, norms, fft_per_chunk, inplace, 1);
}

/* ------------------------------------------------------------------ spectral, 1024 rows per pol (fixed by the kernels) */

REFK_API int refk_set_frb_delays(float *frb_delays, float dm)
{
    Buf d;
    TRY(d.alloc0(sizeof(float) * K_NCHAN));                                        /* :715 */
    set_frb_delays<<<K_NCHAN / K_NTHREAD + 1, K_NTHREAD>>>(d.f(), dm);             /* :717 */
    LAUNCHED();
    TRY(d.download(frb_delays, sizeof(float) * K_NCHAN));
    TRY(d.release());
    return 0;
}

/* fft_out: [2][1024][6251] complex, in place */
REFK_API int refk_inject_frb(float *fft_out, const float *frb_delays, int nfft_since_frb, float frb_width, float frb_amp)
{
    Buf f, d;
    TRY(f.upload(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    TRY(d.upload(frb_delays, sizeof(float) * K_NCHAN));
    inject_frb<<<K_NCHAN / K_NTHREAD + 1, K_NTHREAD>>>(f.c(), d.f(), nfft_since_frb, frb_width, frb_amp);   /* :1241 */
    LAUNCHED();
    TRY(f.download(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    TRY(f.release());
    TRY(d.release());
    return 0;
}

/* fft_out: [2][1024][6251] complex, in place; bp: [2][6251], in place */
REFK_API int refk_detect_and_normalize2(float *fft_out, float *bp, float scale)
{
    Buf f, b;
    TRY(f.upload(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    TRY(b.upload(bp, sizeof(float) * K_NCHAN * 2));                                /* :700-701 */
    detect_and_normalize2<<<(K_NCHAN * 2) / K_NTHREAD + 1, K_NTHREAD>>>(f.c(), b.f(), scale);   /* :1259 */
    LAUNCHED();
    TRY(f.download(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    TRY(b.download(bp, sizeof(float) * K_NCHAN * 2));
    TRY(f.release());
    TRY(b.release());
    return 0;
}

/* kur_weights: 2048 entries (fft_per_chunk, :643) */
REFK_API int refk_detect_and_normalize3(float *fft_out, const float *kur_weights, float *bp, float scale)
{
    Buf f, w, b;
    TRY(f.upload(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    TRY(w.upload(kur_weights, sizeof(float) * FFT_PER_CHUNK));
    TRY(b.upload(bp, sizeof(float) * K_NCHAN * 2));                                /* :706-707 */
    detect_and_normalize3<<<(K_NCHAN * 2) / K_NTHREAD + 1, K_NTHREAD>>>(f.c(), w.f(), b.f(), scale);   /* :1265 */
    LAUNCHED();
    TRY(f.download(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    TRY(b.download(bp, sizeof(float) * K_NCHAN * 2));
    TRY(f.release());
    TRY(w.release());
    TRY(b.release());
    return 0;
}

/* npol == 1 only (:1279); maxn = fft_per_chunk*NCHAN/2 (:1278) */
REFK_API int refk_pscrunch(float *fft_out)
{
    int nsms;
    TRY(get_nsms(&nsms));
    Buf f;
    TRY(f.upload(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    pscrunch<<<nsms * 32, K_NTHREAD>>>(f.c(), SPEC_ELEMS / 2);                      /* :1282 */
    LAUNCHED();
    TRY(f.download(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    TRY(f.release());
    return 0;
}

/* kur_weights: 2048 entries, rewritten in place */
REFK_API int refk_pscrunch_weights(float *fft_out, float *kur_weights)
{
    int nsms;
    TRY(get_nsms(&nsms));
    Buf f, w;
    TRY(f.upload(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    TRY(w.upload(kur_weights, sizeof(float) * FFT_PER_CHUNK));
    pscrunch_weights<<<nsms * 32, K_NTHREAD>>>(f.c(), w.f(), SPEC_ELEMS / 2);       /* :1287 */
    LAUNCHED();
    TRY(f.download(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    TRY(w.download(kur_weights, sizeof(float) * FFT_PER_CHUNK));
    TRY(f.release());
    TRY(w.release());
    return 0;
}

/* fft_ave: scrunch_elems(npol) floats (:658-660); maxn of :1278, :1301 */
REFK_API int refk_tscrunch(const float *fft_out, float *fft_ave, int npol)
{
    if (npol != 1 && npol != 2) return -1;
    int nsms;
    TRY(get_nsms(&nsms));
    Buf f, a;
    TRY(f.upload(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    TRY(a.alloc0(sizeof(float) * scrunch_elems(npol)));
    tscrunch<<<nsms * 32, K_NTHREAD>>>(f.c(), a.f(), scrunch_elems(npol));          /* :1304 */
    LAUNCHED();
    TRY(a.download(fft_ave, sizeof(float) * scrunch_elems(npol)));
    TRY(f.release());
    TRY(a.release());
    return 0;
}

REFK_API int refk_tscrunch_weights(const float *fft_out, float *fft_ave, const float *kur_weights, int npol)
{
    if (npol != 1 && npol != 2) return -1;
    int nsms;
    TRY(get_nsms(&nsms));
    Buf f, a, w;
    TRY(f.upload(fft_out, sizeof(cufftComplex) * SPEC_ELEMS));
    TRY(a.alloc0(sizeof(float) * scrunch_elems(npol)));
    TRY(w.upload(kur_weights, sizeof(float) * FFT_PER_CHUNK));
    tscrunch_weights<<<nsms * 32, K_NTHREAD>>>(f.c(), a.f(), w.f(), scrunch_elems(npol));   /* :1309 */
    LAUNCHED();
    TRY(a.download(fft_ave, sizeof(float) * scrunch_elems(npol)));
    TRY(f.release());
    TRY(a.release());
    TRY(w.release());
    return 0;
}

/* one packer launch (no synchronisation); maxn of :1322 */
static int sel_and_dig(int npol, int nbit, int nsms, float *dev_ave, unsigned char *dev_out)
{
    size_t maxn = scrunch_elems(npol);
    maxn = (size_t)K_NCHANOUT * (maxn / K_NCHAN) / (8 / nbit);                      /* :1322 */
    if (maxn != trim_bytes(npol, nbit)) return -1;
    switch (nbit) {
    case 2: sel_and_dig_2b<<<nsms * 32, K_NTHREAD>>>(dev_ave, dev_out, maxn, npol); break;   /* :1326 */
    case 4: sel_and_dig_4b<<<nsms * 32, K_NTHREAD>>>(dev_ave, dev_out, maxn, npol); break;   /* :1333 */
    case 8: sel_and_dig_8b<<<nsms * 32, K_NTHREAD>>>(dev_ave, dev_out, maxn, npol); break;   /* :1340 */
    default: return -1;
    }
    return 0;
}

/* fft_ave: scrunch_elems(npol) floats; out: trim_bytes(npol, nbit) bytes */
static int sel_and_dig_host(const float *fft_ave, unsigned char *out, int npol, int nbit)
{
    if (npol != 1 && npol != 2) return -1;
    int nsms;
    TRY(get_nsms(&nsms));
    Buf a, o;
    TRY(a.upload(fft_ave, sizeof(float) * scrunch_elems(npol)));
    TRY(o.alloc0(trim_bytes(npol, nbit)));                                         /* :676-677 */
    int rc = sel_and_dig(npol, nbit, nsms, a.f(), o.u());
    if (rc) return rc;
    LAUNCHED();                                                                    /* :1354 */
    TRY(o.download(out, trim_bytes(npol, nbit)));
    TRY(a.release());
    TRY(o.release());
    return 0;
}

REFK_API int refk_sel_and_dig_2b(const float *fft_ave, unsigned char *out, int npol) { return sel_and_dig_host(fft_ave, out, npol, 2); }
REFK_API int refk_sel_and_dig_4b(const float *fft_ave, unsigned char *out, int npol) { return sel_and_dig_host(fft_ave, out, npol, 4); }
REFK_API int refk_sel_and_dig_8b(const float *fft_ave, unsigned char *out, int npol) { return sel_and_dig_host(fft_ave, out, npol, 8); }

/* ------------------------------------------------------------------ the two chains, no round trips in between */

/* K1 -> K5 in the order of src/process_baseband.cu:1152-1203 on one segment of `rows` rows per pol.
 * udat: [2][rows*12500] bytes.  rfi_mode 1: apply_kurtosis writes in place (fft_in_kur == fft_in, :606);
 * rfi_mode 2: into a second buffer (:607-609).  Outputs (any may be NULL): time (fft_in after the chain),
 * time_kur (fft_in_kur), pow / kur / dag (50*rows each), pow_fb / kur_fb / dag_fb (2*rows each), weights (2*rows). */
REFK_API int refk_chain_time(const unsigned char *udat, int rows, int rfi_mode, float *time, float *time_kur, float *pow,
                             float *kur, float *dag, float *pow_fb, float *kur_fb, float *dag_fb, float *weights)
{
    if (!time_rows_ok(rows) || (rfi_mode != 1 && rfi_mode != 2)) return -1;
    const TimeShape s(rows);
    int nsms;
    TRY(get_nsms(&nsms));
    Buf u, in, ink, pk, pkfb, d, dfb, w;
    TRY(u.upload(udat, s.samps_per_chunk));                                        /* :582 */
    TRY(in.alloc0(sizeof(float) * s.samps_per_chunk));                             /* :602 */
    if (rfi_mode == 2) TRY(ink.alloc0(sizeof(float) * s.samps_per_chunk));         /* :607-609 */
    TRY(pk.alloc0(2 * sizeof(float) * s.nkurto_per_chunk));                        /* :626 */
    TRY(pkfb.alloc0(2 * sizeof(float) * s.fft_per_chunk));                         /* :628 */
    TRY(d.alloc0(sizeof(float) * s.nkurto_per_chunk));                             /* :637 */
    TRY(dfb.alloc0(sizeof(float) * s.fft_per_chunk));                              /* :639 */
    TRY(w.alloc0(sizeof(float) * s.fft_per_chunk));                                /* :643 */
    float *fft_in = in.f(), *fft_in_kur = rfi_mode == 2 ? ink.f() : in.f();
    float *pow_dev = pk.f(), *kur_dev = pk.f() + s.nkurto_per_chunk;               /* :629 */
    float *pow_fb_dev = pkfb.f(), *kur_fb_dev = pkfb.f() + s.fft_per_chunk;        /* :630 */

    convertarray<<<nsms * 32, K_NTHREAD>>>(fft_in, u.u(), s.samps_per_chunk);      /* :1152 */
    TRY(hipGetLastError());
    kurtosis<<<(unsigned)s.nkurto_per_chunk, 256>>>(fft_in, pow_dev, kur_dev);     /* :1167 */
    TRY(hipGetLastError());
    compute_dagostino<<<nsms * 32, K_NTHREAD>>>(kur_dev, d.f(), s.nkurto_per_chunk / 2);   /* :1173 */
    TRY(hipGetLastError());
    block_kurtosis<<<s.fft_per_chunk / 8, 256>>>(pow_dev, kur_dev, d.f(), pow_fb_dev, kur_fb_dev);   /* :1179 */
    TRY(hipGetLastError());
    compute_dagostino2<<<nsms * 32, K_NTHREAD>>>(kur_fb_dev, dfb.f(), s.fft_per_chunk / 2);   /* :1183 */
    TRY(hipGetLastError());
    TRY(hipMemset(w.p, 0, sizeof(float) * s.fft_per_chunk));                       /* :1187 */
    apply_kurtosis<<<(unsigned)s.nkurto_per_chunk, 256>>>(fft_in, fft_in_kur, d.f(), dfb.f(), w.f());   /* :1195 */
    LAUNCHED();

    TRY(in.download(time, sizeof(float) * s.samps_per_chunk));
    if (time_kur) TRY(hipMemcpy(time_kur, fft_in_kur, sizeof(float) * s.samps_per_chunk, hipMemcpyDeviceToHost));
    if (pow) TRY(hipMemcpy(pow, pow_dev, sizeof(float) * s.nkurto_per_chunk, hipMemcpyDeviceToHost));
    if (kur) TRY(hipMemcpy(kur, kur_dev, sizeof(float) * s.nkurto_per_chunk, hipMemcpyDeviceToHost));
    TRY(d.download(dag, sizeof(float) * s.nkurto_per_chunk));
    if (pow_fb) TRY(hipMemcpy(pow_fb, pow_fb_dev, sizeof(float) * s.fft_per_chunk, hipMemcpyDeviceToHost));
    if (kur_fb) TRY(hipMemcpy(kur_fb, kur_fb_dev, sizeof(float) * s.fft_per_chunk, hipMemcpyDeviceToHost));
    TRY(dfb.download(dag_fb, sizeof(float) * s.fft_per_chunk));
    TRY(w.download(weights, sizeof(float) * s.fft_per_chunk));
    TRY(u.release());
    TRY(in.release());
    TRY(ink.release());
    TRY(pk.release());
    TRY(pkfb.release());
    TRY(d.release());
    TRY(dfb.release());
    TRY(w.release());
    return 0;
}

/* src/process_baseband.cu:1231-1352 for one segment of 1024 rows per pol, the FFTs' outputs given.
 * spec_raw: fft_out, spec_kur: fft_out_kur, [2][1024][6251] complex each (RFI mode 0 reads only spec_raw, mode 1 only
 * spec_kur).  weights: 2048 entries, as apply_kurtosis left them.  bp_raw / bp_kur: [2][6251] persistent state, updated in
 * place (RFI mode 1 uses bp_raw alone, bp_kur_dev == bp_dev, :703).  frb_delays != NULL and inject_now > 0: inject_frb
 * with the constants of :1238-1240.  Outputs (any may be NULL): ave_raw / ave_kur (the fp32 planes), codes_raw /
 * codes_kur, weights_out (after pscrunch_weights). */
REFK_API int refk_chain_detect(const float *spec_raw, const float *spec_kur, const float *weights, float *bp_raw,
                               float *bp_kur, const float *frb_delays, int inject_now, int rfi_mode, int npol, int nbit,
                               float *ave_raw, float *ave_kur, unsigned char *codes_raw, unsigned char *codes_kur,
                               float *weights_out)
{
    if (rfi_mode < 0 || rfi_mode > 2 || (npol != 1 && npol != 2) || (nbit != 2 && nbit != 4 && nbit != 8)) return -1;
    int nsms;
    TRY(get_nsms(&nsms));
    const bool raw = rfi_mode == 0 || rfi_mode == 2, exc = rfi_mode == 1 || rfi_mode == 2;
    const size_t spec_bytes = sizeof(cufftComplex) * SPEC_ELEMS, bp_bytes = sizeof(float) * K_NCHAN * 2;
    const size_t scrunch = scrunch_elems(npol), trim = trim_bytes(npol, nbit);
    Buf f, fk, w, b, bk, del, a, ak, t, tk;
    /* buffer aliasing per RFI mode as at :606-613, :661-664, :684-686, :703-709: mode 1 runs its one stream in the first set */
    TRY(f.upload(rfi_mode == 1 ? spec_kur : spec_raw, spec_bytes));
    if (rfi_mode == 2) TRY(fk.upload(spec_kur, spec_bytes));
    if (exc) TRY(w.upload(weights, sizeof(float) * FFT_PER_CHUNK));
    TRY(b.upload(bp_raw, bp_bytes));
    if (rfi_mode == 2) TRY(bk.upload(bp_kur, bp_bytes));
    TRY(a.alloc0(sizeof(float) * scrunch));
    if (rfi_mode == 2) TRY(ak.alloc0(sizeof(float) * scrunch));
    TRY(t.alloc0(trim));
    if (rfi_mode == 2) TRY(tk.alloc0(trim));
    cufftComplex *fft_out = f.c(), *fft_out_kur = rfi_mode == 2 ? fk.c() : f.c();
    float *bp_dev = b.f(), *bp_kur_dev = rfi_mode == 2 ? bk.f() : b.f();
    float *fft_ave = a.f(), *fft_ave_kur = rfi_mode == 2 ? ak.f() : a.f();
    unsigned char *trim_dev = t.u(), *trim_kur_dev = rfi_mode == 2 ? tk.u() : t.u();
    const double tsmooth = 1, tsamp = double(K_NFFT) / K_VLITE_RATE * K_NSCRUNCH;    /* :739-740 */
    const float bp_scale = tsamp / tsmooth;                                         /* :741 */

    if (frb_delays && inject_now > 0) {
        TRY(del.upload(frb_delays, sizeof(float) * K_NCHAN));
        const float frb_width = 2e-3 * 10 * K_VLITE_RATE / 10 / K_NFFT;            /* :1238, the macros expanded left to right */
        const float frb_amp = 1.05;                                                 /* :1239 */
        const int nfft_since_frb = (inject_now - 1) * K_ROWS;                       /* :1240 */
        inject_frb<<<K_NCHAN / K_NTHREAD + 1, K_NTHREAD>>>(fft_out, del.f(), nfft_since_frb, frb_width, frb_amp);   /* :1241 */
        TRY(hipGetLastError());
        if (rfi_mode > 1) {
            inject_frb<<<K_NCHAN / K_NTHREAD + 1, K_NTHREAD>>>(fft_out_kur, del.f(), nfft_since_frb, frb_width, frb_amp);   /* :1246 */
            TRY(hipGetLastError());
        }
    }
    if (raw) {
        detect_and_normalize2<<<(K_NCHAN * 2) / K_NTHREAD + 1, K_NTHREAD>>>(fft_out, bp_dev, bp_scale);   /* :1259 */
        TRY(hipGetLastError());
    }
    if (exc) {
        detect_and_normalize3<<<(K_NCHAN * 2) / K_NTHREAD + 1, K_NTHREAD>>>(fft_out_kur, w.f(), bp_kur_dev, bp_scale);   /* :1265 */
        TRY(hipGetLastError());
    }
    size_t maxn = SPEC_ELEMS / (npol == 1 ? 2 : 1);                                 /* :1278 */
    if (npol == 1) {
        if (raw) {
            pscrunch<<<nsms * 32, K_NTHREAD>>>(fft_out, maxn);                      /* :1282 */
            TRY(hipGetLastError());
        }
        if (exc) {
            pscrunch_weights<<<nsms * 32, K_NTHREAD>>>(fft_out_kur, w.f(), maxn);   /* :1287 */
            TRY(hipGetLastError());
        }
    }
    maxn /= K_NSCRUNCH;                                                             /* :1301 */
    if (raw) {
        tscrunch<<<nsms * 32, K_NTHREAD>>>(fft_out, fft_ave, maxn);                 /* :1304 */
        TRY(hipGetLastError());
    }
    if (exc) {
        tscrunch_weights<<<nsms * 32, K_NTHREAD>>>(fft_out_kur, fft_ave_kur, w.f(), maxn);   /* :1309 */
        TRY(hipGetLastError());
    }
    int rc = sel_and_dig(npol, nbit, nsms, fft_ave, trim_dev);    /* :1326 / :1333 / :1340 */
    if (rc) return rc;
    if (rfi_mode > 1) {
        rc = sel_and_dig(npol, nbit, nsms, fft_ave_kur, trim_kur_dev);   /* :1329 / :1336 / :1343 */
        if (rc) return rc;
    }
    LAUNCHED();                                                                     /* :1354 */

    if (raw) {
        TRY(a.download(ave_raw, sizeof(float) * scrunch));
        TRY(t.download(codes_raw, trim));
    }
    if (exc) {
        if (ave_kur) TRY(hipMemcpy(ave_kur, fft_ave_kur, sizeof(float) * scrunch, hipMemcpyDeviceToHost));
        if (codes_kur) TRY(hipMemcpy(codes_kur, trim_kur_dev, trim, hipMemcpyDeviceToHost));
        TRY(w.download(weights_out, sizeof(float) * FFT_PER_CHUNK));
    }
    TRY(b.download(bp_raw, bp_bytes));
    if (rfi_mode == 2) TRY(bk.download(bp_kur, bp_bytes));
    TRY(f.release());
    TRY(fk.release());
    TRY(w.release());
    TRY(b.release());
    TRY(bk.release());
    TRY(del.release());
    TRY(a.release());
    TRY(ak.release());
    TRY(t.release());
    TRY(tk.release());
    return 0;
}
