// Channeliser: 8-bit unpack + 12500-point real FFT + square-law detect of the 4096 output
// channels, one workgroup per (row, pol), everything between the raw bytes and the
// power spectrum staying in registers and LDS.
//
// Replaces, per FFT row:  convertarray (src/pb_kernels.cu:23-33), the copy/zero half of
// apply_kurtosis (:267-287), cufftExecR2C (src/process_baseband.cu:1222-1224), inject_frb
// (src/pb_kernels.cu:348-391), the |X|^2 of detect_and_normalize2/3 (:416, :481) and the
// division by the row weight of detect_and_normalize3 (:452, :481).
//
// FFT: the 12500 real samples are packed as 6250 complex, transformed by three Stockham
// passes of radix 25, 25, 10 and split back into the real-input spectrum.  The operation
// order (butterfly formulas, where fmaf is used, twiddle tables) is the specification in
// oracle/pb_oracle.c "K6"; results agree with the oracle bit for bit.  Pass-1 butterfly input
// r comes from 500-sample kurtosis block r, so a flagged block is simply a zeroed input.
//
// Passes (rfi_mode 2): every (row, pol) workgroup transforms the unflagged data and writes the raw
// power plane.  A row without a flagged block gets NOTHING in the excised plane: its excised power is
// the raw power over the full weight 1 + 2^-23, which detect's excised stream derives from the raw
// plane (k_detect2.hip, CONV == 2).  Only when some block is flagged does the workgroup run a second
// pass on the zeroed data (or write +inf, "no data", if every block is flagged).  (The coherence twins
// still store both planes for every row.)
//
// FRB injection (inject_frb): k_channelize and k_channelize_kur hold no injection code; launch_channelize picks their
// twins k_inject_chan and k_inject_chan_kur, the same text with the per-channel window test compiled in, for the calls
// that have a pulse to inject.
//
// Coherence output (pb_config.coherence): the same kernels, instantiated with COH = true (k_coh_chan,
// k_coh_chan_kur), store the complex in-band spectrum X (4096 x float2 per row and pol, after injection) in
// place of |X|^2, undivided by the row weight; a row of weight 0 gets zeros in the excised plane.
// k_detect_coh.hip forms the power, the cross products and everything after them.
//
// LDS: one 6250 x float2 buffer (50 000 B) used in place: every pass reads its inputs into
// registers, barriers, then writes.  3 workgroups per CU.
// HBM traffic per (row, pol): 12.5 KB of samples read, 16 KB of power written (+ 16 KB for a row with flags);
// twiddles (tw2 4.9 KB, tw3 49 KB, post 49 KB) stay in L2.
#include <cstdlib>
#include <cstring>

#include "pb_internal.h"

#ifdef CH_STAMP
// timing experiments (variant builds only): the clock at the phase boundaries of every workgroup's first
// transform (+ its XCC id and flag mask); read back with pb_internal_ch_stamps
#define CH_STAMP_MAXWG 40960
__shared__ unsigned long long ch_ts[9];
__device__ unsigned long long g_ch_stamp[CH_STAMP_MAXWG][13];
extern "C" int pb_internal_ch_stamps(unsigned long long *out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ch_stamp), sizeof(g_ch_stamp));
}
#ifndef CH_STAMP_TID
#define CH_STAMP_TID 0
#endif
#define FFT_STAMP(i) do { if (threadIdx.x == CH_STAMP_TID) ch_ts[i] = __builtin_amdgcn_s_memtime(); } while (0)
#endif
#include "fft_lds.h"
#include "kurtosis_dev.h"

#ifndef CH_ABL
#define CH_ABL 0      // energy / timing experiments (variant builds only, results invalid): 2 no plane stores, 4 no
                      // spectrum step, 8 no FFT passes, 16 no staging / unpack of the transforms  (1, no moments of the
                      // statistic, and 32, dword reads for the moments, went with the shared row_block_moments;
                      // their results are in profiles/r04_notes.md section 8)
#endif
struct ChanArgs {
    const uint8_t *in;      // [A][S][2][seg_samples]
    size_t in_ant_stride, seg_samples;
    const float *wrow;        // [A][S*R] row weights and
    const uint32_t *rowmask;  // flag masks from k_kurtosis_row (bit r = block r flagged)
    size_t wrow_ant_stride;
    float *Praw, *Pkur;     // [A][S][2][R][4096]
    size_t p_ant_stride;
    const float2 *tw2, *tw3, *post;
    const float2 *postc;    // post[2155..6250], 16-byte aligned copy
    FrbParams frb;          // delays == nullptr: no injection
    int R, rfi_mode, inject_now;
    // k_channelize_kur only: where the row's flags, weight and mask go, and the D'Agostino constants
    uint8_t *flags;         // [A][S*R*25]
    size_t flags_ant_stride;
    float *wrow_out;
    uint32_t *rowmask_out;
    const DagConsts *dag;
};

// The row's 12500 bytes go to LDS through 16-byte loads (narrow per-lane loads are bound by the address unit,
// not by HBM: 2-byte loads move 128 B per wave instruction, these 1 KiB).  Rows are only 4-byte aligned, so the
// aligned 16-byte chunks that cover the row are fetched (d_in is padded for the overhang): chunks tid, tid+256,
// tid+512 always exist (782 or 783 in all), tid+768 for tid < 15.
struct RowStage {
    uint4 t0, t1, t2, t3;
};
__device__ __forceinline__ size_t row_byte(const ChanArgs &a, int seg, int row, int pol, int ant)
{
    return (size_t)ant * a.in_ant_stride + ((size_t)seg * 2 + pol) * a.seg_samples + (size_t)row * PB_NFFT;
}
__device__ __forceinline__ void stage_request(const ChanArgs &a, int tid, int seg, int row, int pol, int ant, RowStage &st)
{
    const size_t rbyte = row_byte(a, seg, row, pol, ant);
    const unsigned o = (unsigned)(rbyte & 15);   // offset of the row's first byte in its first chunk
    const uint4 *src16 = (const uint4 *)(a.in + (rbyte - o));
    const int nch = (int)((o + PB_NFFT + 15) >> 4);   // <= 783
    st.t0 = src16[tid];
    st.t1 = src16[tid + 256];
    st.t2 = src16[tid + 512];
    st.t3 = make_uint4(0u, 0u, 0u, 0u);
    if (tid + 768 < nch) st.t3 = src16[tid + 768];
}

// x / (1 + 2^-23), the division of a row without flags (87 % of rows on clean noise), on the bits: the quotient
// is the first or the second float below x -- the second when x's mantissa field m is 0 or >= 0x400002
// (m 2^-23 >= 1.5 + ...: the exact quotient m (1 - 2^-23 + 2^-46 - ...) lies below the midpoint) -- checked
// against the IEEE division for every positive normal binary32 from 0x00800002 up (tools/check_div_full_weight.c);
// smaller values, zeros and non-finite ones take the division.  For one value, with b the bits of x:
//     m1 = (b & 0x7fffffu) - 1u;   quotient bits = b - (m1 >= 0x400001u ? 2u : 1u)
//     unless b - 0x00800002u >= 0x7f800000u - 0x00800002u, which divides.
// The kernels apply it to a thread's four powers at a time (div_row_weight4, spectrum_div4.h): five vector
// instructions per value, then ONE range test for the four (the unsigned maximum of b - 0x00800002u) and a branch on a
// vote of the wave, i.e. a scalar branch that ordinary data never takes -- about 7 issue slots per value.  With the
// range test as an early return per value the compiler built an exec-mask diamond around every one of a thread's
// sixteen values: 13 slots per value, 11 of the true division's instructions not executed but 8 of masking added.
#include "spectrum_div4.h"

// One transform of one (row, pol): ROLE 0 = raw spectrum (the coherence twins: also the excised plane's when the row
// has no flagged block), ROLE 1 = excised spectrum (flagged blocks zeroed).  The row's bytes have been
// requested by stage_request; mask and wrow may still be in flight (ROLE 0 first needs them after the FFT).
// next_row >= 0: the bytes of that row (of the same segment and pol) are requested into st as soon as the FFT is
// done, so that their latency runs under this transform's spectrum step.
// FIX: code 0 -> 128 on every staging (the input buffer has not been patched by a kurtosis pass); next_pol: the
// polarisation of the next transform's row.
// prestaged: the row's (patched) bytes already lie at the start of buf -- the statistic of k_channelize_kur staged
// them there -- so nothing is staged and no barrier precedes the unpack.
// DEFER (k_channelize_kur, ROLE 0): the row's flag mask and weight are not known yet when the transform starts (one
// wave works them out while the others unpack); they are read from `smw` after the FFT, where ROLE 0 first needs
// them, and what to request next (the same row again for its excised transform, else `after_row` of pol 1) is decided
// there too.
// INJ 0: no FRB injection code at all (k_channelize, k_channelize_kur: production runs without injection, and a
// run-time test put a uniform branch, the booleans' re-materialisation and the injection parameters' registers into
// every channel); INJ 1: the run-time test (the injecting twins k_inject_chan*, chosen by launch_channelize when
// there is something to inject, and the coherence twins).
template <int ROLE, bool FIX = false, bool DEFER = false, bool COH = false, int INJ = 1>
__device__ __forceinline__ void channelize_pass(const ChanArgs &a, f2 *buf, int tid, int seg, int row, int pol, int ant,
                                                RowStage &st, unsigned mask, float wrow, size_t prow, int next_row,
                                                int next_pol = -1, bool prestaged = false,
                                                const unsigned *smw = nullptr, int after_row = -1)
{
    if (next_pol < 0) next_pol = pol;
    FFT_STAMP(0);
    const unsigned o = (unsigned)(row_byte(a, seg, row, pol, ant) & 15);   // recomputed, not carried from the request
    if (!prestaged) {
        // a dropped-frame byte (0) means "no sample" = 0.0 = code 128 (convertarray :23-33), so that the
        // conversion below is one fma per sample pair.  The kurtosis kernel has already patched such codes in
        // the input buffer; only RFI mode 0, which has no kurtosis pass, does it here (four per instruction).
        uint4 *stage = (uint4 *)buf;
        const bool last = tid + 768 < (int)((o + PB_NFFT + 15) >> 4);
        if (FIX || a.rfi_mode == 0) {
            stage[tid] = fix_zero_codes(st.t0);
            stage[tid + 256] = fix_zero_codes(st.t1);
            stage[tid + 512] = fix_zero_codes(st.t2);
            if (last) stage[tid + 768] = fix_zero_codes(st.t3);
        } else {
            stage[tid] = st.t0;
            stage[tid + 256] = st.t1;
            stage[tid + 512] = st.t2;
            if (last) stage[tid + 768] = st.t3;
        }
        __syncthreads();
    }
    FFT_STAMP(1);
    f2 v[25];
    if (tid < 250) {
        const unsigned zmask = ROLE == 1 ? mask : 0u;
        const uint16_t *sb = (const uint16_t *)((const uint8_t *)buf + o);
#pragma unroll
        for (int r = 0; r < 25; ++r) {
            unsigned w = sb[tid + 250 * r];
            if ((zmask >> r) & 1u) w = 0x8080u;   // flagged block -> zeros (apply_kurtosis :243-295)
            v[r] = cvt_pair_c(w);
        }
    }
    __syncthreads();   // all samples are in registers before pass 1 overwrites buf
    FFT_STAMP(2);
    // The spectrum step's eight twiddle loads are requested from inside pass 3: one L2 latency for the
    // whole step instead of one per 1024-channel slice, and most of it hidden under pass 3 (the step was
    // 25-35 % of a workgroup's life, almost all of it waiting).
    float4 tq[4][2];
    auto load_tq = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            tq[i][0] = *(const float4 *)(a.postc + tid * 4 + 1024 * i);
            tq[i][1] = *(const float4 *)(a.postc + tid * 4 + 1024 * i + 2);
        }
    };
#if CH_ABL & 8
    load_tq();
    if (tid < 250)
        for (int r = 0; r < 25; ++r) buf[tid * 25 + r] = v[r];
    __syncthreads();
#else
    fft6250(v, buf, (const f2 *)a.tw2, (const f2 *)a.tw3, tid, load_tq);
#endif
    if (DEFER) {
        // (written by wave 0 before the barrier in front of pass 1)
        mask = __builtin_amdgcn_readfirstlane(smw[0]);
        wrow = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(smw[1]));
        const bool again = (a.rfi_mode == 1 || (a.rfi_mode == 2 && mask != 0)) && mask != 0x1ffffffu;
        next_row = again ? row : after_row;
        next_pol = again ? pol : 1;
    }
#ifndef FFT_LEAN
    if (next_row >= 0) stage_request(a, tid, seg, next_row, next_pol, ant, st);
#endif

    // FRB injection window of this row, per channel (inject_frb :361-380)
    const bool inject = INJ && a.frb.delays != nullptr && a.inject_now > 0;
    const int since = inject ? (a.inject_now - 1 + seg) * a.R : 0;
    const bool also_kur = a.rfi_mode == 2 && ROLE == 0 && mask == 0;
    // the weight of a row without flags: 25 x 0.04f summed left to right = 1 + 2^-23
    const bool full_w = __builtin_bit_cast(unsigned, wrow) == 0x3f800001u;
    float *P0 = (ROLE == 1 ? a.Pkur : a.Praw) + prow;
    float *P1 = a.Pkur + prow;
    // What is the same for the whole row is settled here, once, and handed to the four slices through registers the
    // compiler cannot re-derive (left to itself it redid the 64-bit scalar adds of both row pointers and the two
    // tests in every slice, 14 issue slots each time): the two planes' rows, and what the excised plane gets from
    // this transform -- 0 nothing, 2 the powers over wrow.  A row of the full weight (every row without flags) gets
    // NOTHING: its excised power is a function of the raw plane, pow / (1 + 2^-23), and detect's excised stream takes it
    // from there (k_detect2.hip, CONV == 2) -- the division and 16 KB of stores per (row, pol) less, for 83 - 87 % of rows.
    // (1, the powers over 1 + 2^-23 on the bits, is what this kernel stored for such a row before; the rule lives on in
    // spectrum_div4.h for detect.)
    int kur_how = also_kur && !full_w ? 2 : 0;
    if constexpr (!COH) asm volatile("" : "+s"(kur_how), "+s"(P0), "+s"(P1));
    // four consecutive channels per thread: 16-byte twiddle loads and 16-byte power stores (one
    // channel per lane would spare the 8-way LDS bank conflicts of these reads, but its 4-byte stores
    // measured 9 % slower overall)
#pragma unroll
    for (int i = 0; i < ((CH_ABL & 4) ? 0 : 4); ++i) {
        const int c4 = tid * 4 + 1024 * i;
        const float4 t01 = tq[i][0], t23 = tq[i][1];
        const f2 tw[4] = {mk2(t01.x, t01.y), mk2(t01.z, t01.w), mk2(t23.x, t23.y), mk2(t23.z, t23.w)};
        float pw[4];
        const int k0 = PB_CHANMIN + c4;
        f2 zas[4], zbs[4];
        read_z_pairs(buf, k0, zas, zbs);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + q;
            const f2 za = zas[q];
            const f2 zb = zbs[q];
            f2 E, O;
            addsub_conj(za, zb, E, O);
            const f2 Pq = cmul(O, tw[q]);
            f2 X = mk2(0.5f, 0.5f) * (E + Pq);
            if (inject) {
                const float d = a.frb.delays[k];
                const int lo = (int)(d + 0.5) - since;
                const int hi = (int)(d + a.frb.width + 0.5) - since;
                if (row >= lo && row <= hi) X = X * mk2(a.frb.amp, a.frb.amp);
            }
            if constexpr (COH) {
                // the complex spectrum, stored at once (for the excised plane too when the row has no flagged
                // block); the planes are float2, so row prow starts 2 prow floats in
                *(float2 *)(P0 + prow + 2 * (k - PB_CHANMIN)) = make_float2(X.x, X.y);
                if (ROLE == 0 && also_kur) *(float2 *)(P1 + prow + 2 * (k - PB_CHANMIN)) = make_float2(X.x, X.y);
            } else {
                // (one add into the value's place in the store quad: left to pair the four sums into packed adds,
                //  the compiler spends more on moving the halves together than the pairing saves)
                const f2 sq = X * X;
                asm("v_add_f32 %0, %1, %2" : "=v"(pw[q]) : "v"(sq.x), "v"(sq.y));
            }
        }
        if constexpr (COH) continue;
        // the excised plane carries pow / w (detect_and_normalize3 :452,:481), so that the
        // serial bandpass recurrence downstream has no division in it.  (The rows' pointers have been through
        // registers: the casts say again that they are global memory.  The thread's address is one 64-bit vector
        // add per store; holding it, or a 32-bit offset beside scalar bases, across the slices cost registers the
        // kernel does not have -- 8 to 24 bytes of scratch in every form tried.)
        if (ROLE == 0) store_plane4((pb_gfloat *)(P0 + c4), pw[0], pw[1], pw[2], pw[3]);
        if (ROLE == 1)
            store_plane4((pb_gfloat *)(P0 + c4), pw[0] / wrow, pw[1] / wrow, pw[2] / wrow, pw[3] / wrow);
        else if (kur_how) {
            div_row_weight4(pw, wrow, kur_how == 1);
            store_plane4((pb_gfloat *)(P1 + c4), pw[0], pw[1], pw[2], pw[3]);
        }
    }
#ifdef FFT_LEAN
    if (next_row >= 0) stage_request(a, tid, seg, next_row, next_pol, ant, st);
#endif
#ifdef CH_STAMP
    if (ROLE == 0 && threadIdx.x == CH_STAMP_TID) {
        ch_ts[7] = __builtin_amdgcn_s_memtime();
        const unsigned wg = blockIdx.x + gridDim.x * blockIdx.y;
        if (wg < CH_STAMP_MAXWG && blockIdx.z == 0) {
            for (int i = 0; i < 8; ++i) g_ch_stamp[wg][i] = ch_ts[i];
            g_ch_stamp[wg][8] = __builtin_amdgcn_s_getreg(20 | (3 << 11));   // HW_REG_XCC_ID[3:0]
            g_ch_stamp[wg][9] = mask;
            g_ch_stamp[wg][10] = __builtin_amdgcn_s_getreg(4 | (31 << 11));      // HW_REG_HW_ID
            g_ch_stamp[wg][11] = __builtin_amdgcn_s_memrealtime();
            g_ch_stamp[wg][12] = ch_ts[8];   // kernel entry
        }
    }
#endif
}

// Three workgroups per CU (LDS 3 x 50 000 B, <= 168 VGPRs).  A workgroup takes CH_ROWS consecutive rows of one
// (segment, pol) and requests the bytes of its next transform (the same row again when it has flagged blocks,
// else the next row) while the current one is in its spectrum step.  Measured (profiles/r02_notes.md, per-workgroup
// clock stamps): the request-to-LDS latency is 3000 cycles of a 22 000-cycle transform and a workgroup hand-over
// ~1500, yet 2 rows per workgroup are only 1-2 % faster than 1, and 8 or 16 are slower: the three co-resident
// workgroups fill each other's waits, and longer runs of rows bring the workgroups of a CU into step.
// Measured earlier (profiles/r01 notes):
//  * capping residency at two to let a detect workgroup of the previous batch co-reside does not
//    pay -- both kernels are bound by VALU issue, so side by side they only stretch each other;
//  * fully persistent workgroups (768 for the whole launch) were 12 % SLOWER than one workgroup per (row, pol):
//    the dispatcher's staggered starts overlap the workgroups' load, FFT and store phases better than a
//    lock-step loop does.  Short runs of rows keep that staggering.
#ifndef CH_ROWS
#define CH_ROWS 2
#endif
// ---- the channeliser that computes the flags of its own row (RFI modes 1 and 2, taps = 1) ----
// One workgroup = one FFT row of BOTH polarisations: the flag of a 500-sample block is the max over the two pols of
// the D'Agostino score, so the row's 2 x 25 blocks are reduced first (k_kurtosis_row's phase: the two rows staged in
// the FFT buffer, the reference's halving tree per block, 50 lanes of double-precision scores, ballot -> mask and
// weight, also written out for detect and the debug readers), then the transforms of pol 0 and pol 1 follow as in
// k_channelize, the next transform's bytes requested while the current one is in its spectrum step.  What it saves
// against kurtosis kernel + channeliser: the second read of every byte (256 MB per second of data), a kernel whose
// only overlap partner was the previous batch's detect (0.06 ms alone, 0.13 there), and a cross-stream hand-over;
// the next batch's channeliser then starts straight behind this one and detect runs wholly beside it.
// The input buffer is NOT patched for code 0 here (nobody reads it again but this workgroup): every staging fixes
// the codes on the way (FIX).
#ifdef KUR_STAMP
// timing experiments (variant builds only, tools/kur_stamps.py): the clock at the phase boundaries of every workgroup
__device__ unsigned long long g_kur_stamp[4][10240][10];   // the last four launches (a.frb.since counts them); [8], [9]: s_memrealtime (100 MHz, one clock for the chip) at entry / exit
extern "C" int pb_internal_kur_stamps(unsigned long long *out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_kur_stamp), sizeof(g_kur_stamp));
}
#define KSTAMP(i) do { if (threadIdx.x == 0) kts[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define KSTAMP(i)
#endif
#define CH_COH 0
#define CH_INJ 0
#define CH_K_PLAIN k_channelize
#define CH_K_KUR k_channelize_kur
#include "k_channelize_kernels.inc"
#undef CH_INJ
#undef CH_K_PLAIN
#undef CH_K_KUR
#define CH_INJ 1
#define CH_K_PLAIN k_inject_chan
#define CH_K_KUR k_inject_chan_kur
#include "k_channelize_kernels.inc"
#undef CH_COH
#undef CH_K_PLAIN
#undef CH_K_KUR
#define CH_COH 1
#define CH_K_PLAIN k_coh_chan
#define CH_K_KUR k_coh_chan_kur
#include "k_channelize_kernels.inc"
#undef CH_COH
#undef CH_INJ
#undef CH_K_PLAIN
#undef CH_K_KUR

static bool check_consts(std::string &why)
{
    // the literals of fft_consts.h must be what libm gives here and in the oracle
    auto same = [](float a, double b) { float c = (float)b; return memcmp(&a, &c, 4) == 0; };
    bool ok = same(FC_C1, cos(2.0 * M_PI / 5.0)) && same(FC_C2, cos(4.0 * M_PI / 5.0)) &&
              same(FC_S1, sin(2.0 * M_PI / 5.0)) && same(FC_S2, sin(4.0 * M_PI / 5.0));
    for (int x = 1; x < 5 && ok; ++x)
        for (int y = 1; y < 5 && ok; ++y) {
            const double ang = 2.0 * M_PI * (double)(x * y) / 25.0;
            ok = same(kW25[x * 5 + y][0], cos(ang)) && same(kW25[x * 5 + y][1], -sin(ang));
        }
    for (int k = 1; k < 5 && ok; ++k) {
        const double ang = 2.0 * M_PI * (double)k / 10.0;
        ok = same(kW10[k][0], cos(ang)) && same(kW10[k][1], -sin(ang));
    }
    if (!ok) why = "fft_consts.h does not match this host's libm; rerun tools/gen_fft_consts.py";
    return ok;
}

hipError_t launch_channelize(pb_handle *h, int nseg, int inject_now)
{
    static int consts_ok = -1;
    if (consts_ok < 0) {
        std::string why;
        consts_ok = check_consts(why) ? 1 : 0;
        if (!consts_ok) h->err = why;
    }
    if (!consts_ok) return hipErrorInvalidValue;
    if (nseg <= 0) return hipSuccess;
    const pb_handle::BufSet &b = h->set();
    ChanArgs a;
    a.in = b.d_in.p;
    a.in_ant_stride = (size_t)h->S * 2 * h->seg_samples;
    a.seg_samples = h->seg_samples;
    a.wrow = b.d_wrow.p;
    a.rowmask = pb_rowmask(h);
    a.wrow_ant_stride = (size_t)h->S * h->R;
    a.Praw = b.d_Praw.p;
    a.Pkur = b.d_Pkur.p;
    a.p_ant_stride = (size_t)h->S * 2 * h->R * PB_NCHANOUT;
    a.tw2 = h->ft.tw2.p;
    a.tw3 = h->ft.tw3.p;
    a.post = h->ft.post.p;
    a.postc = h->ft.postc.p;
    a.frb.delays = (inject_now > 0) ? h->d_frb_delays.p : nullptr;
    a.frb.width = h->frb_width;
    a.frb.amp = h->frb_amp;
#ifdef KUR_STAMP
    static int kur_launches = 0;
    a.frb.since = kur_launches++;     // (unused by the kernels: which of the four stamp buffers)
#else
    a.frb.since = 0;
#endif
    a.R = h->R;
    a.rfi_mode = h->cfg.rfi_mode;
    a.inject_now = inject_now;
    a.flags = b.d_flags.p;
    a.flags_ant_stride = (size_t)h->S * h->nblk_seg;
    a.wrow_out = b.d_wrow.p;
    a.rowmask_out = pb_rowmask(h);
    a.dag = h->d_dag.p;
    // the power-plane kernels carry no injection code; their twins that do run only when there is a pulse to inject
    const bool inject = inject_now > 0 && a.frb.delays != nullptr;
    if (pb_fused_kurtosis(h)) {
        // one workgroup per row (both pols): it computes the row's flags itself
        dim3 gk((unsigned)h->R, (unsigned)nseg, (unsigned)h->A);
        if (h->cfg.coherence) k_coh_chan_kur<<<gk, 256, 0, h->stream>>>(a);
        else if (inject) k_inject_chan_kur<<<gk, 256, 0, h->stream>>>(a);
        else k_channelize_kur<<<gk, 256, 0, h->stream>>>(a);
        return hipGetLastError();
    }
    dim3 grid((unsigned)((h->R + CH_ROWS - 1) / CH_ROWS), (unsigned)(nseg * 2), (unsigned)h->A);
    if (h->cfg.coherence) {
        k_coh_chan<<<grid, 256, 0, h->stream>>>(a);
        return hipGetLastError();
    }
#ifdef FFT_LEAN
    static const int lean_lds = pb_lean_lds(M_HALF * 8);
#else
    const int lean_lds = 0;
#endif
    if (inject) k_inject_chan<<<grid, 256, lean_lds, h->stream>>>(a);
    else k_channelize<<<grid, 256, lean_lds, h->stream>>>(a);
    return hipGetLastError();
}

// ---- float-input channeliser with optional 4-tap FIR (pb_channelize_f32) ----
// x: (nrows + taps - 1) rows of 12500 floats; out row t = rfft(sum_j taps[j] * x[row t + j]),
// the WOLA form of analysis/baseband.py:1226-1233.
__global__ __launch_bounds__(256) void k_channelize_f32(const float *__restrict__ x, int taps,
                                                        const float *__restrict__ fir, float2 *__restrict__ out,
                                                        const float2 *tw2, const float2 *tw3, const float2 *post)
{
    __shared__ f2 buf[M_HALF];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const float *xr = x + row * PB_NFFT;
    f2 v[25];
    if (tid < 250) {
#pragma unroll
        for (int r = 0; r < 25; ++r) {
            const int n = 2 * (tid + 250 * r);
            if (taps == 1) {
                v[r] = *(const f2 *)(xr + n);
            } else {
                float2 acc = make_float2(0.f, 0.f);
                for (int j = 0; j < 4; ++j) {
                    const float2 s = *(const float2 *)(xr + (size_t)j * PB_NFFT + n);
                    const float2 t = *(const float2 *)(fir + (size_t)j * PB_NFFT + n);
                    const float px = t.x * s.x, py = t.y * s.y;
                    acc.x = j ? acc.x + px : px;
                    acc.y = j ? acc.y + py : py;
                }
                v[r] = mk2(acc.x, acc.y);
            }
        }
    }
    fft6250(v, buf, (const f2 *)tw2, (const f2 *)tw3, tid);
    for (int k = tid; k < PB_NCHAN; k += 256) {
        const f2 X = rsplit(buf, (const f2 *)post, k);
        out[row * PB_NCHAN + k] = make_float2(X.x, X.y);
    }
}

hipError_t launch_channelize_f32(pb_handle *h, const float *d_x, int nrows, int taps, float2 *d_out)
{
    hipError_t e = launch_channelize(h, 0, 0);  // validates the compile-time constants
    if (e != hipSuccess) return e;
    k_channelize_f32<<<nrows, 256, 0, h->stream>>>(d_x, taps, h->ft.taps.p, d_out, h->ft.tw2.p, h->ft.tw3.p, h->ft.post.p);
    return hipGetLastError();
}
