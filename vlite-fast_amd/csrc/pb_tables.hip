// The constant tables a handle carries, built on the host when it is created (pb_handle.hip: create_impl): the D'Agostino
// constants and the band search, the FFT twiddles and FIR taps, the PFB history slots with the window energies, the FRB
// delays (pb_set_frb_params); and the debug entry points that check them on the device (pb_debug_dag_check, pb_channelize_f32).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "kurtosis_dev.h"
#include "pb_internal.h"

// D'Agostino constants with the reference's float/double evaluation (src/pb_kernels.cu:4-11)
static DagConsts make_dag(float NK)
{
    const double mu1 = -6. / (NK + 1);
    const float den = (NK + 1) * (NK + 1) * (NK + 3) * (NK + 5);
    const double mu2 = (24. * NK * (NK - 2) * (NK - 3)) / den;
    const float q = NK * NK - 5 * NK + 2;
    const float d2 = (NK + 7) * (NK + 9);
    const float d3 = NK * (NK - 2) * (NK - 3);
    const double g1 = 6. * q / d2 * sqrt((6. * (NK + 3) * (NK + 5)) / d3);
    const double A = 6. + (8. / g1) * (2. / g1 + sqrt(1. + 4. / (g1 * g1)));
    DagConsts c;
    c.t_lo_sure = c.t_hi_clear = 0.f;                                  // (no crossings known: every t is in a
    c.t_lo_clear = c.t_hi_sure = __builtin_inff();                     //  "band", the score itself decides)
    c.one_m_2_over_A = (1 - 2. / A);
    c.mu1 = mu1;
    c.Z1 = sqrt(4.5 * A);
    c.Z2 = 1 - 2. / (9 * A);
    c.Z3 = sqrt(2. / (mu2 * (A - 4)));
    return c;
}

// Where the D'Agostino score crosses DAG_THRESH as a function of t (DagConsts): the crossings are located on the host
// (the score is the same IEEE double arithmetic there) by bisection over the positive floats, then the DEVICE
// evaluates the score on every float within DAG_WIN of each crossing and the bands are read off its answers: below /
// above a crossing by more than the window the score is monotonic beyond doubt (one float step of t moves it by
// 4e-7, the cube root's last-ulp wobble by at most 1.2e-6: three steps).
#define DAG_WIN 256
static int find_dag_bands(pb_handle *h, DagConsts &c)
{
    auto flagged = [&](uint32_t bits) { return dag_of_t(__builtin_bit_cast(float, bits), c) > 3.0f; };
    const float t_mid = (float)(c.Z2 * c.Z2 * c.Z2);                 // score 0
    const uint32_t b_mid = __builtin_bit_cast(uint32_t, t_mid);
    uint32_t lo = __builtin_bit_cast(uint32_t, 1e-6f), hi = b_mid;   // flagged at lo, clear at hi
    if (!flagged(lo) || flagged(hi)) return fail(h, PB_ESTATE, "D'Agostino score: no lower crossing");
    while (hi - lo > 1) {
        const uint32_t m = lo + (hi - lo) / 2;
        if (flagged(m)) lo = m; else hi = m;
    }
    const uint32_t cross_lo = hi;
    lo = b_mid;
    hi = __builtin_bit_cast(uint32_t, 100.0f);                        // clear at lo, flagged at hi
    if (flagged(lo) || !flagged(hi)) return fail(h, PB_ESTATE, "D'Agostino score: no upper crossing");
    while (hi - lo > 1) {
        const uint32_t m = lo + (hi - lo) / 2;
        if (flagged(m)) hi = m; else lo = m;
    }
    const uint32_t cross_hi = hi;
    const int n = 2 * DAG_WIN + 1;
    DevBuf<uint8_t> d_f;
    std::vector<uint8_t> f(2 * n);
    HIPCHK(h, d_f.alloc(2 * n));
    HIPCHK(h, launch_dag_scan(h, c, cross_lo - DAG_WIN, n, d_f.p));
    HIPCHK(h, launch_dag_scan(h, c, cross_hi - DAG_WIN, n, d_f.p + n));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(f.data(), d_f.p, 2 * n, hipMemcpyDeviceToHost));
    const uint8_t *a = f.data(), *b = f.data() + n;
    // lower crossing: flagged ... flagged | band | clear ... clear
    int first_clear = 0, last_flag = n - 1;
    while (first_clear < n && a[first_clear]) ++first_clear;
    while (last_flag >= 0 && !a[last_flag]) --last_flag;
    // upper crossing: clear ... clear | band | flagged ... flagged
    int first_flag = 0, last_clear = n - 1;
    while (first_flag < n && !b[first_flag]) ++first_flag;
    while (last_clear >= 0 && b[last_clear]) --last_clear;
    if (first_clear < 8 || last_flag > n - 9 || last_flag < 0 || first_clear >= n || first_flag < 8 || last_clear > n - 9 ||
        last_clear < 0 || first_flag >= n)
        return fail(h, PB_ESTATE, "D'Agostino score: crossing not inside the scanned window");
    c.t_lo_sure = __builtin_bit_cast(float, cross_lo - DAG_WIN + (uint32_t)(first_clear - 1));
    c.t_lo_clear = __builtin_bit_cast(float, cross_lo - DAG_WIN + (uint32_t)(last_flag + 1));
    c.t_hi_clear = __builtin_bit_cast(float, cross_hi - DAG_WIN + (uint32_t)(first_flag - 1));
    c.t_hi_sure = __builtin_bit_cast(float, cross_hi - DAG_WIN + (uint32_t)(last_clear + 1));
    return PB_OK;
}

int build_dag(pb_handle *h, bool search_bands)
{
    h->dag = make_dag((float)PB_NKURTO);
    h->dag_fb = make_dag((float)PB_NFFT);
    if (!search_bands) {
        h->dag_bands = -1;
    } else if (int rcb = find_dag_bands(h, h->dag)) {
        // The bands only save work (the score is then evaluated in a few floats around the crossings instead of
        // everywhere): if the search does not bracket the crossings -- host and device disagreeing by more than the
        // scanned window -- fall back to "no bands", where the score itself decides every flag: same flags, more
        // arithmetic.  That disagreement is worth knowing about on a library pinned bit for bit: it is said once on
        // stderr and kept in the handle (pb_debug_dag_check reports the bands as 0, inf, 0, inf).  A HIP error is fatal.
        if (rcb != PB_ESTATE) return rcb;
        fprintf(stderr, "libpb_hip: warning: %s -- flag decision falls back to evaluating the D'Agostino score for "
                        "every block (results unchanged, kurtosis statistic slower)\n", h->err.c_str());
        h->dag = make_dag((float)PB_NKURTO);
        h->dag_bands = -2;
        h->err.clear();
    } else {
        h->dag_bands = 1;
    }
    // (a copy in device memory for the channeliser that flags its own rows: ten fewer scalar registers of arguments)
    HIPCHK(h, h->d_dag.alloc(1));
    HIPCHK(h, hipMemcpy(h->d_dag.p, &h->dag, sizeof(DagConsts), hipMemcpyHostToDevice));
    return PB_OK;
}

static float2 cis_neg(double num, double den)
{
    const double a = 2.0 * M_PI * num / den;
    return make_float2((float)cos(a), (float)(-sin(a)));
}

// a table of n elements in device memory, counted in device_bytes
template <class T>
static int upload(pb_handle *h, DevBuf<T> &d, const T *src, size_t n)
{
    HIPCHK(h, d.grow(h, n));
    HIPCHK(h, hipMemcpy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return PB_OK;
}

int build_fft_tables(pb_handle *h)
{
    std::vector<float2> tw2(600), tw3(6250), post(PB_NCHAN);
    // fft_lds.h's layouts.  tw2[pair = (r-1)/2][k][2], r = 1..24: twiddles (r, r + 1) as one 16-byte entry with the lane's
    // k fastest, so a wave's load touches 4 cache lines, not one 192-byte row per k.  tw3[j][r-1], r = 1..9 (+ 1 pad):
    // per-thread contiguous (the same re-layout of tw3 gains as much again but costs the two-kernel channeliser a
    // register spill, profiles/r05_notes.md)
    for (int k = 0; k < 25; ++k)
        for (int r = 1; r < 25; ++r) tw2[(((r - 1) / 2) * 25 + k) * 2 + ((r - 1) & 1)] = cis_neg((double)(r * k), 625.0);
    for (int j = 0; j < 625; ++j) {
        for (int r = 1; r < 10; ++r) tw3[j * 10 + (r - 1)] = cis_neg((double)(r * j), 6250.0);
        tw3[j * 10 + 9] = make_float2(0.f, 0.f);
    }
    for (int k = 0; k < PB_NCHAN; ++k) {
        const double a = 2.0 * M_PI * (double)k / (double)PB_NFFT;
        post[k] = make_float2((float)(-sin(a)), (float)(-cos(a)));
    }
    FftTables &t = h->ft;
    if (int rc = upload(h, t.tw2, tw2.data(), tw2.size())) return rc;
    if (int rc = upload(h, t.tw3, tw3.data(), tw3.size())) return rc;
    if (int rc = upload(h, t.post, post.data(), post.size())) return rc;
    if (int rc = upload(h, t.postc, post.data() + PB_CHANMIN, (size_t)PB_NCHANOUT)) return rc;
    // 4-tap Hamming WOLA taps of analysis/baseband.py:1207-1232 (always built: 200 KB):
    // tap j = window[j ns : (j+1) ns] * norms[0] * (j ? norms[j] : 1), evaluated in double
    const int ns = PB_NFFT, nw = 4;
    std::vector<double> win((size_t)nw * ns);
    for (size_t k = 0; k < win.size(); ++k)
        win[k] = 0.54 - 0.46 * cos(2.0 * M_PI * (double)k / (double)(win.size() - 1));
    double norms[4];
    for (int j = 0; j < nw; ++j) {
        double s = 0;
        for (int k = 0; k < ns; ++k) s += win[(size_t)j * ns + k] * win[(size_t)j * ns + k];
        norms[j] = 1. / s;
    }
    std::vector<float> taps((size_t)nw * ns);
    for (int j = 0; j < nw; ++j)
        for (int k = 0; k < ns; ++k)
            taps[(size_t)j * ns + k] = (float)(win[(size_t)j * ns + k] * norms[0] * (j ? norms[j] : 1.0));
    if (int rc = upload(h, t.taps, taps.data(), taps.size())) return rc;
    std::vector<float2> tn((size_t)(ns / 2) * 4);
    for (int n = 0; n < ns / 2; ++n)
        for (int j = 0; j < 4; ++j)
            tn[(size_t)n * 4 + j] = make_float2(taps[(size_t)j * ns + 2 * n], taps[(size_t)j * ns + 2 * n + 1]);
    return upload(h, t.taps_n, tn.data(), tn.size());
}

// taps = 4 (after build_fft_tables): the two history slots, empty, and the window's energy per (tap, 500-sample block)
int build_pfb_history(pb_handle *h)
{
    // two slots each: a batch's channeliser and weights read slot hist_rd, its history kernel fills the other one
    const size_t A = h->A, hb = 2 * A * 2 * 3 * PFB_HIST_STRIDE;
    HIPCHK(h, h->d_hist_in.grow(h, hb));
    HIPCHK(h, hipMemset(h->d_hist_in.p, 0, hb));
    HIPCHK(h, h->d_hist_flags.grow(h, 2 * A * 3 * PB_BLK_PER_FFT));
    HIPCHK(h, hipMemset(h->d_hist_flags.p, 1, 2 * A * 3 * PB_BLK_PER_FFT));
    HIPCHK(h, h->d_hist_valid.grow(h, 2 * A * 3));
    HIPCHK(h, hipMemset(h->d_hist_valid.p, 0, 2 * A * 3));
    h->hist_rd = 0;
    // from the float taps the kernel multiplies by
    std::vector<float> taps((size_t)4 * PB_NFFT), E(101);
    HIPCHK(h, hipMemcpy(taps.data(), h->ft.taps.p, taps.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int j = 0; j < 4; ++j)
        for (int b = 0; b < PB_BLK_PER_FFT; ++b) {
            double e = 0;
            for (int m = 0; m < PB_NKURTO; ++m) {
                const double t = taps[(size_t)j * PB_NFFT + b * PB_NKURTO + m];
                e += t * t;
            }
            E[j * PB_BLK_PER_FFT + b] = (float)e;
        }
    float totf = 0.f;
    for (int i = 0; i < 100; ++i) totf = totf + E[i];      // same order as k_pfb_weights sums
    E[100] = totf;
    return upload(h, h->d_tapE, E.data(), E.size());
}

// set_frb_delays, src/pb_kernels.cu:338-346; width_rows < 0 selects the reference's 2 ms
// (frb_width = 2e-3*SEG_PER_SEC*FFTS_PER_SEG with the macro expanded left to right, :1238)
int set_frb(pb_handle *h, float dm, float width_rows, float amp)
{
    std::vector<float> d(PB_NCHAN);
    const double rate = (double)h->R * PB_NFFT * 10;
    for (int i = 0; i < PB_NCHAN; ++i) {
        const double freq = 0.384 - (i * 0.064) / PB_NCHAN;
        const double scale = 4.15e-3 * dm * 10 * rate / 10 / PB_NFFT;
        d[i] = (float)(scale / (freq * freq) - scale / (0.384 * 0.384));
    }
    if (int rc = upload(h, h->d_frb_delays, d.data(), d.size())) return rc;      // (made by the first call)
    h->frb_width = width_rows < 0 ? (float)(2e-3 * 10 * rate / 10 / PB_NFFT) : width_rows;
    h->frb_amp = amp;
    return PB_OK;
}

extern "C" int pb_set_frb_params(pb_handle *h, float dm, float width_rows, float amp)
{
    if (!h) return PB_EINVAL;
    if (!h->cfg.inject_frb) return fail(h, PB_ESTATE, "pb_set_frb_params needs inject_frb=1");
    if (!(dm >= 0) || !(amp > 0)) return fail(h, PB_EINVAL, "pb_set_frb_params: bad dm or amp");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, sync_all(h));
    return set_frb(h, dm, width_rows, amp);
}

extern "C" int pb_debug_dag_check(pb_handle *h, float kur_lo, float kur_hi, uint64_t *nchecked, uint64_t *nmismatch,
                                  float *bands4)
{
    if (!h || !nchecked || !nmismatch) return PB_EINVAL;
    if (!(kur_lo > 0) || !(kur_hi >= kur_lo)) return fail(h, PB_EINVAL, "pb_debug_dag_check: 0 < kur_lo <= kur_hi");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const uint32_t b0 = __builtin_bit_cast(uint32_t, kur_lo), b1 = __builtin_bit_cast(uint32_t, kur_hi);
    const uint64_t n = (uint64_t)(b1 - b0) + 1;
    DevBuf<unsigned long long> d_bad;
    unsigned long long bad = 0;
    HIPCHK(h, d_bad.alloc(1));
    HIPCHK(h, hipMemset(d_bad.p, 0, sizeof bad));
    HIPCHK(h, launch_dag_check(h, b0, n, d_bad.p));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
    *nchecked = n;
    *nmismatch = bad;
    const float bands[4] = {h->dag.t_lo_sure, h->dag.t_lo_clear, h->dag.t_hi_clear, h->dag.t_hi_sure};
    if (bands4) memcpy(bands4, bands, sizeof bands);
    return PB_OK;
}

extern "C" int pb_channelize_f32(pb_handle *h, const float *x, int nrows, int taps, float *out)
{
    if (!h || !x || !out || nrows < 1) return PB_EINVAL;
    if (!(taps == 1 || taps == 4)) return fail(h, PB_EINVAL, "taps must be 1 or 4");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DevBuf<float> d_x;
    DevBuf<float2> d_o;
    const size_t nin = (size_t)(nrows + taps - 1) * PB_NFFT, nout = (size_t)nrows * PB_NCHAN;
    HIPCHK(h, d_x.alloc(nin));
    HIPCHK(h, d_o.alloc(nout));
    HIPCHK(h, hipMemcpy(d_x.p, x, nin * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, launch_channelize_f32(h, d_x.p, nrows, taps, d_o.p));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, d_o.p, nout * sizeof(float2), hipMemcpyDeviceToHost));
    return PB_OK;
}
