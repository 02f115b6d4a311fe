/*
 * pb_hip.h -- C ABI of libpb_hip.so: the MI355X baseband -> filterbank hot path.
 *
 * The reference (kerrm/vlite-fast) has no plugin / FFI interface for this path: it is the
 * body of one executable, src/process_baseband.cu main() (:334-1614), calling the kernels
 * of src/pb_kernels.cu.  The drop-in boundary is therefore the process boundary
 * (scripts/start_process:50 -> `process_baseband -k -K -w -b -g -o -C`), and this header
 * is what a host process -- ours in Python, or the reference's own main() with its CUDA
 * calls replaced -- binds in place of the per-segment device code at
 * src/process_baseband.cu:1108-1376.  Each entry point names the reference lines it
 * replaces.
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative
 * PB_E* code and leaves a message for pb_last_error(); nothing throws across the
 * boundary (the reference is fail-stop: cudacheck -> throw 20, src/cuda_util.cu:4-12).
 * A handle owns one GPU's state and is not thread-safe; different handles are independent.
 *
 * Geometry (compile-time in the reference, src/process_baseband.h:16-55):
 *   NFFT 12500, NCHAN 6251, NSCRUNCH 8, NKURTO 500, CHANMIN 2155, CHANMAX 6250
 *   -> 4096 output channels; a *segment* is rows_per_seg FFT rows of one antenna, both
 *   polarisations (the reference fixes rows_per_seg = FFTS_PER_SEG = 1024 = 100 ms).
 * Only the 4096 output channels (FFT bins 2155..6250) are carried past the FFT: the other
 * 2155 bins never reach an output of the reference, so planes named "compact" below are
 * [..][4096] where the reference's are [..][6251] offset by CHANMIN.
 */
#ifndef PB_HIP_H
#define PB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PB_NFFT 12500
#define PB_NCHAN 6251
#define PB_NSCRUNCH 8
#define PB_NKURTO 500
#define PB_CHANMIN 2155
#define PB_CHANMAX 6250
#define PB_NCHANOUT 4096
#define PB_BLK_PER_FFT 25
#define PB_VDIF_FRAME 5032
#define PB_VDIF_DATA 5000
#define PB_FRAMES_PER_SEC 25600

#define PB_OK 0
#define PB_EINVAL (-22)
#define PB_ENOMEM (-12)
#define PB_EHIP (-5)      /* a HIP / hipFFT call failed; see pb_last_error */
#define PB_ESTATE (-1)

#define PB_FFT_LDS 0      /* in-library fixed-order radix 25x25x10 FFT in LDS (bit-exact vs oracle) */
#define PB_FFT_HIPFFT 1   /* hipFFT/rocFFT R2C plan, as the reference uses cuFFT */

typedef struct pb_handle pb_handle;

typedef struct pb_config {
    uint32_t struct_size;   /* sizeof(pb_config), for ABI growth (pb_create also takes the size without `coherence`:
                               callers built before it was appended get coherence = 0) */
    int32_t device;         /* -g   src/process_baseband.cu:458-472 */
    int32_t nant;           /* antennas batched on this GPU (reference: one process each) */
    int32_t nbit;           /* -b   2 | 4 | 8              :416-425 */
    int32_t npol;           /* -P   1 = AA+BB, 2 = AA,BB    :439-448 */
    int32_t rfi_mode;       /* -r   0 | 1 | 2              :427-437 */
    int32_t taps;           /* 1 = rectangular window (reference GPU path),
                               4 = 4-tap Hamming WOLA of analysis/baseband.py:1207 */
    int32_t fft_backend;    /* PB_FFT_LDS | PB_FFT_HIPFFT */
    int32_t rows_per_seg;   /* FFTS_PER_SEG (1024); any positive multiple of 8 */
    int32_t max_seg;        /* segments staged per pb_process call (>= 1) */
    int32_t inject_frb;     /* -i   :399-401, :711-718 */
    int32_t keep_ave;       /* also keep the fp32 pre-quantisation planes (coadd input) */
    int32_t debug_keep;     /* keep kurtosis statistics for pb_debug_fetch (selects the kurtosis kernel + channeliser
                             * pair; without it the in-library-FFT channeliser flags its own rows: same results) */
    int32_t nsets;          /* buffer sets for batch pipelining, 1..8 (1 = none, 2 = double-buffered, 3 = the host
                             * collects the batch queued two calls ago) */
    int32_t coherence;      /* 1 = coherence output (needs npol = 2), 0 = off */
} pb_config;

/* Coherence output (coherence = 1, "-P 2 --coherence"): per output time sample [time][4][4096] in the order
 * AA, BB, CR, CI (the AABBCRCI coherence products).  Pol A = VDIF thread 0, pol B = thread 1, row t of each.
 * AA and BB are byte for byte what npol = 2 writes.  With A = (ax, ay), B = (bx, by) the complex in-band spectra
 * of the row (after injection), every line one binary32 operation, left to right, no contraction:
 *   re = ax*bx + ay*by          im = ay*bx - ax*by     (im = Im(A conj B): swapping the pols negates CI)
 *   raw stream:     n = bpA' * bpB'                       (bandpass after this row's update, as AA / BB divide by)
 *   excised stream: n = (bpA' * wA) * (bpB' * wB)         (row weights after apply_kurtosis); CR = CI = 0 if
 *                   either weight is 0 or either pol's power takes the 11x clip
 *   d = sqrtf(n);  CR = re / d * 1.41421356f;  CI = im / d * 1.41421356f
 * Time scrunch: raw = tscrunch (sum of 8 rows, * (float)sqrt(1./8)); excised = tscrunch_weights with the row
 * weight (float)(0.5 * (wA + wB)) when both weights are >= 0.2, else the row is skipped.  The 8/4/2-bit quantisers
 * with npol = 4.  code_bytes_per_seg = 4 * R/8 * 4096 * nbit/8, ave_floats_per_seg = 4 * R/8 * 4096 (compact
 * [4][R/8][4096]).  Not offered (PB_EINVAL): taps = 4, PB_FFT_HIPFFT, debug_keep, the pb_coadd_* entry points. */

typedef struct pb_sizes {
    uint64_t seg_samples_per_pol;  /* rows_per_seg * 12500 */
    uint64_t input_bytes_per_seg;  /* 2 * seg_samples_per_pol */
    uint64_t code_bytes_per_seg;   /* "trim", src/process_baseband.cu:667-675 */
    uint64_t ave_floats_per_seg;   /* compact: (npol==1?1:2, coherence: 4) * rows_per_seg/8 * 4096 */
    uint64_t rows_per_seg;
    uint64_t blocks_per_seg_pol;   /* rows_per_seg * 25 kurtosis blocks */
    uint64_t device_bytes;         /* HBM held by the handle */
} pb_sizes;

/* per-stage device time, hipEvent pairs on the handle's stream (reference: the PROFILE
 * stopwatch, src/process_baseband.h:9-13, src/process_baseband.cu:1538-1558) */
#define PB_NSTAGE 8
enum { PB_ST_KURTOSIS = 0, PB_ST_CHANNELIZE = 1, PB_ST_FFT = 2, PB_ST_INJECT = 3,
       PB_ST_DETECT = 4, PB_ST_DEFRAME = 5, PB_ST_COADD = 6, PB_ST_H2D = 7 };
typedef struct pb_timers {
    double ms[PB_NSTAGE];
    uint64_t launches[PB_NSTAGE];
} pb_timers;

/* what pb_debug_fetch can return (needs debug_keep=1 for the first three) */
enum { PB_DBG_POW = 0,      /* float [2][nblk]   kurtosis `pow`  src/pb_kernels.cu:104 */
       PB_DBG_KUR = 1,      /* float [2][nblk]   `kur`           :105 */
       PB_DBG_DAG = 2,      /* float [2][nblk]   `dag`           :132 */
       PB_DBG_FLAGS = 3,    /* uint8 [nblk]      dag > DAG_THRESH (:256), shared by both pols */
       PB_DBG_ROWWEIGHT = 4, /* float [rows]     kur_weights after apply_kurtosis (:292) */
       PB_DBG_POW_FB = 5,   /* float [2][rows]   block_kurtosis `pow_block` :140-212 (diagnostic, K4) */
       PB_DBG_KUR_FB = 6,   /* float [2][rows]   block_kurtosis `kur_block` */
       PB_DBG_DAG_FB = 7    /* float [rows]      compute_dagostino2 over FFT rows :219-241 */ };

void pb_config_default(pb_config *cfg);

/* replaces the one-time allocations + cufftPlan1d, src/process_baseband.cu:472-709 */
int pb_create(const pb_config *cfg, pb_handle **out);
/* replaces :1572-1602 */
void pb_destroy(pb_handle *h);
const char *pb_last_error(const pb_handle *h);   /* h may be NULL: last pb_create failure */
int pb_query(const pb_handle *h, pb_sizes *out);

/* run on a caller-supplied hipStream_t (e.g. torch's current stream); NULL = own stream */
int pb_set_stream(pb_handle *h, void *hip_stream);
int pb_sync(pb_handle *h);

/* bandpass state bp_dev / bp_kur_dev (:700-709): zero = "initialise from the next
 * segment's mean" (src/pb_kernels.cu:406-411,444-461).  Compact [2 pols][4096]. */
int pb_reset_bandpass(pb_handle *h, int ant);
/* taps=4 only: forget the three rows the FIR window carries over from the previous call (start of
 * a new observation).  No-op for taps=1. */
int pb_reset_history(pb_handle *h, int ant);
int pb_get_bandpass(pb_handle *h, int ant, float *bp_raw, float *bp_kur);
int pb_set_bandpass(pb_handle *h, int ant, const float *bp_raw, const float *bp_kur);

/* Stage one segment of one antenna from host memory: the two blocking H2D copies at
 * src/process_baseband.cu:1116-1122 (pol-planar 8-bit samples). */
int pb_submit_planar(pb_handle *h, int ant, int seg, const uint8_t *pol0, const uint8_t *pol1,
                     size_t nsamp_per_pol);
/* Same from device memory (HBM-resident producer), device-to-device on the handle's stream. */
int pb_submit_planar_dev(pb_handle *h, int ant, int seg, const void *d_pol0, const void *d_pol1,
                         size_t nsamp_per_pol);
/* Stage from a raw 1-s ring block of 5032-B VDIF frames (the layout writer/genbase put in
 * ring 0x40): replaces the host frame-demux loop :1015-1067 AND the H2D copies; the
 * headers are indexed on the host, payloads are gathered on the GPU.  seg0 = first of the
 * rows_per_seg-sized segments the block fills (10 per second at rows_per_seg = 1024).
 * Missing frames are zero-filled (the writer's gap fill, src/writer.c:674-688). */
int pb_submit_vdif(pb_handle *h, int ant, int seg0, const uint8_t *block, size_t nbytes);
/* The same with the block's time origin given explicitly (VDIF seconds-from-epoch of its first sample
 * and the frame number within that second), as the reference places every frame by its own header
 * (:1032-1045: frame number and thread id decide the slot, not arrival order): a frame that is absent --
 * the very first one included -- leaves zeros, frames of other seconds in the block are ignored.
 * pb_submit_vdif takes the origin from the block's first frame.  Both return as soon as the copies and
 * the gather kernel are queued; `block` must stay untouched until the batch's output has been fetched
 * (or pb_sync): page-locked memory makes the copy truly asynchronous. */
int pb_submit_vdif_at(pb_handle *h, int ant, int seg0, const uint8_t *block, size_t nbytes,
                      int64_t second, int64_t frame0);
/* HBM-resident producers write here directly: [max_seg][2 pols][seg_samples_per_pol] u8 */
int pb_input_dev(pb_handle *h, int ant, void **dptr, size_t *nbytes);

/* All device work of the segment loop body, src/process_baseband.cu:1152-1354, for
 * segments [0, nseg) of every antenna, asynchronously on the handle's stream.
 * inject_now: the reference's inject_frb_now counter (:1231-1251) for segment 0 of this
 * call (0 = none); it is advanced per segment internally. */
int pb_process(pb_handle *h, int nseg, int inject_now);

/* Parameters of the injected test FRB (needs inject_frb=1).  Reference: DM 80, 2 ms, x1.05,
 * compile-time (src/process_baseband.cu:717,1238-1239); generalised so that BASELINE config 3
 * (DM 500) can be synthesised.  width_rows < 0 selects the reference's 2 ms. */
int pb_set_frb_params(pb_handle *h, float dm, float width_rows, float amp);

/* The D2H copies at :1370-1375.  Any pointer may be NULL.  raw_codes / kur_codes:
 * nseg * code_bytes_per_seg; ave_*: nseg * ave_floats_per_seg (needs keep_ave);
 * weights: nseg * rows_per_seg, kur_weights as tscrunch_weights sees them. */
int pb_fetch(pb_handle *h, int ant, int seg0, int nseg, uint8_t *raw_codes, uint8_t *kur_codes,
             float *weights, float *ave_raw, float *ave_kur);
/* Pipelining across batches (nsets >= 2): every submit / process / fetch / debug call acts on
 * the SELECTED buffer set.  Typical loop: select(k % n); submit; process; select((k-1) % n); fetch
 * (n = 3: fetch batch k-2, whose bytes have arrived, so that the wait never delays queuing batch k+1).
 * Detect + D2H of one set run on streams of their own while the next set's channeliser (and, with
 * taps = 4 / the hipFFT back end / debug_keep, its kurtosis pass) runs on the first; the bandpass state
 * is shared and advances in pb_process order.  A set's input may be restaged once its previous detect
 * is done; its filterbank bytes must have been fetched before the pb_process after next on that set. */
int pb_select_set(pb_handle *h, int set);
/* zero-copy view of the selected set's filterbank bytes in pinned host memory (valid until the
 * next pb_process on that set): [max_seg][code_bytes_per_seg] of antenna ant, stream 0/1 */
int pb_fetch_ptr(pb_handle *h, int ant, int stream, const uint8_t **codes);
/* device addresses of the same outputs, [max_seg][..] each (stream 0 = raw, 1 = kur) */
int pb_output_dev(pb_handle *h, int ant, int stream, void **codes, void **ave);

/* Incoherent sum (replaces the external MPI coadder scripts/start_coadd:16; arithmetic
 * unpinned): d_sum[seg][ave_floats] (+)= sum over this handle's antennas
 * of their fp32 kur-stream planes (raw stream if rfi_mode 0).  The cross-GPU step is an
 * RCCL reduce of d_sum done by the host (torch.distributed); then on the root:
 * codes = sel_and_dig(d_sum / sqrt(nant_total)). */
int pb_coadd_local(pb_handle *h, int nseg, float *d_sum, int accumulate);
/* The same local sum from the batch's QUANTISED codes instead of the fp32 planes: d_sum (+)= sum over antennas of
 * the centre of each code's quantiser cell, in the fp32 planes' layout (so the reduce and pb_coadd_finish are
 * unchanged).  This is what a coadder fed from the co rings (writer.c:343-352) can do; offered for like-for-like
 * comparisons with the fp32 mode, which is the default.  Works with keep_ave = 0. */
int pb_coadd_local_codes(pb_handle *h, int nseg, float *d_sum, int accumulate);
/* One antenna per handle (nant = 1, the sharding of BASELINE configs[3] at one antenna per GPU): the plane to
 * be reduced IS the antenna's fp32 plane, so detect can write it straight into the caller's buffer and the local
 * sum needs no kernel at all (a 21-MB copy per second of data that cost 0.085 ms of a 0.68-ms step beside the
 * channeliser).  pb_set_coadd_target gives the SELECTED buffer set its own d_sum (NULL: back to the internal
 * plane); pb_coadd_local(h, nseg, that pointer, 0) then only orders the coadd stream behind detect, and
 * pb_coadd_release -- called after the host has queued the collective (and pb_coadd_finish on the root) on the
 * coadd stream -- tells the library that the buffer may be overwritten by the set's next batch. */
/* The incoherent sum in a DEFINED order, so that the coadded bytes do not depend on how the antennas are spread over
 * GPUs or on a collective's internal order (the reference's coadder, scripts/start_coadd:16,20-58,
 * is an external MPI program whose arithmetic is not in the repository).  The order: antennas split by the parity of
 * their index, recursively -- S(o, s) = S(o, 2s) + S(o + s, 2s), a single antenna's plane at the leaves, coadded =
 * S(0, 1).  With the leaves listed left to right that is T_1(x) = x, T_n(x_0..x_{n-1}) = T_ceil(n/2)(x_0..) +
 * T_floor(n/2)(x_ceil(n/2)..), which is what these two calls evaluate, fp32, element by element:
 *   pb_coadd_local_tree: d_dst[seg][ave_floats] = T_n over the fp32 planes (kur stream; raw if rfi_mode 0) of this
 *     handle's antennas ant_order[0..n) of the selected set's batch -- one rank's node of the tree.  Ordered against
 *     detect and the set's next batch like pb_coadd_local.  Needs keep_ave.
 *   pb_coadd_tree: d_dst[0..nfloat) = T_n over n caller-owned device planes d_leaves[0..n) (the root: the ranks'
 *     partial sums as gathered), on the coadd stream.  d_dst must not be one of the leaves unless n = 1.
 * n <= PB_COADD_MAX_LEAVES; planes 16-byte aligned, nfloat a multiple of 4.  Which plane is which leaf is the host's
 * business (vlite-fast_amd/coadd.py: tree_order); pb_coadd_finish(d_dst) follows on the root. */
#define PB_COADD_MAX_LEAVES 32
/* the leaf order of that tree over 0 .. n-1 (even positions first, recursively: 0 | 0 1 | 0 2 1 | 0 2 1 3 | 0 4 2 1 3 |
 * ... ; bit reversal when n is a power of two): order[0..n) for 1 <= n <= PB_COADD_MAX_LEAVES.  Host only, no handle. */
int pb_coadd_tree_order(int n, int32_t *order);
int pb_coadd_local_tree(pb_handle *h, int nseg, const int32_t *ant_order, int n, float *d_dst);
int pb_coadd_tree(pb_handle *h, const float *const *d_leaves, int n, float *d_dst, size_t nfloat);
/* The root's work spread over the ranks ("sliced" layout of the ordered sum, coadd.py): every rank sums and
 * requantises 1/W of the plane, and only code bytes travel to rank 0.
 *   pb_coadd_digitise: d_codes[0 .. nfloat * nbit / 8) = sel_and_dig(d_sum[0 .. nfloat) / sqrt(nant_total)) for a FLAT
 *     range of the npol = 1 plane (sample i of the plane is sample i of the code stream; with two polarisations the code
 *     stream interleaves them, src/pb_kernels.cu:723-727, and a flat range is not a code range: PB_ESTATE).  Device to
 *     device, on the coadd stream; nfloat a multiple of 8.
 *   pb_coadd_publish: the coadded code bytes of one batch, assembled on the device by the caller (the gathered
 *     slices), go to the pinned host buffer that pb_coadd_fetch_ptr hands out -- what pb_coadd_finish does with the
 *     bytes it computes itself.  nbytes <= max_seg * code_bytes_per_seg. */
int pb_coadd_digitise(pb_handle *h, const float *d_sum, size_t nfloat, int nant_total, uint8_t *d_codes);
int pb_coadd_publish(pb_handle *h, const uint8_t *d_codes, size_t nbytes);
int pb_set_coadd_target(pb_handle *h, float *d_sum);
int pb_coadd_release(pb_handle *h);
/* Run pb_coadd_local / pb_coadd_finish (and so the collective the host queues between them) on
 * `stream` (a hipStream_t; NULL = the handle's main stream, the default).  On a stream of its own the
 * sum of batch k, its RCCL reduce and the root's requantisation overlap the kernels of batch k+1;
 * the library orders them against detect of the same buffer set with events. */
int pb_set_coadd_stream(pb_handle *h, void *stream);
int pb_coadd_finish(pb_handle *h, int nseg, const float *d_sum, int nant_total,
                    uint8_t *codes_host);   /* codes_host NULL: asynchronous, see pb_coadd_fetch_ptr */
/* pinned-host view of the coadded bytes of the latest (age 0) or previous (age 1) pb_coadd_finish */
int pb_coadd_fetch_ptr(pb_handle *h, int age, const uint8_t **codes);

/* ---- correlator: the X step over a handle's antennas (reference: analysis/baseband.py `correlate` :807 and
 * analysis/beamforming.py :446, which form the per-channel correlation matrix of all antennas over FFT chunks; the F
 * step is this library's own 12500-point FFT).  Needs coherence = 1: the channeliser then leaves the complex in-band
 * spectra of every antenna, both pols and both streams on the device, and these calls pair antenna i with antenna j.
 * Definition, operation by operation (THIS project's own; tests/correlate_ref.py restates it, tests/golden/
 * reference_correlate.npz ties it to the reference's correlate / get_delays / fit_delays):
 *   inputs     X[a][p][t][c]: the in-band spectra of the batch that the last pb_process put into the selected buffer
 *              set -- antenna a, pol p (0 = VDIF thread 0), channel c = 0..4095, row t = seg * rows_per_seg + row counted
 *              through the batch, 0 <= t < nseg * rows_per_seg.  The values the coherence detection reads, i.e. after
 *              injection.  stream = PB_CORR_RAW or PB_CORR_KUR (the excised stream).
 *   baselines  all pairs i <= j, autos included, row-major over the upper triangle:
 *              bl = i * A - i * (i - 1) / 2 + (j - i), nbl = A (A + 1) / 2.
 *   products   index 2 p + q stands for X_i^p conj(X_j^q): nprod = 4.  For i == j all four are still computed; product 2
 *              is then the conjugate of product 1 and the imaginary parts of products 0 and 3 are +0.
 *   one term   with A = (ax, ay) the value of antenna i and B = (bx, by) that of antenna j, every line one binary32
 *              operation, left to right, no contraction (the lines of the coherence definition above, so product 1 of
 *              an auto is its un-normalised CR / CI):
 *                  re = ax*bx + ay*by          im = ay*bx - ax*by
 *   gates      a call carries ngate gates; gate g has a first row per channel, row0[g][c], and all gates share one
 *              length nrows.  The value for (g, bl, prod, c) starts from acc_re = acc_im = +0.0f and adds the terms of
 *              rows row0[g][c] .. row0[g][c] + nrows - 1 IN ROW ORDER, acc = acc + term, in binary32.  A window may
 *              cross segment boundaries; one that leaves [0, nseg * rows_per_seg) is refused (PB_EINVAL).
 *   rows_used  int32 per (g, bl, c).  Raw stream: nrows.  Excised stream: the number of rows of the window whose row
 *              weight (after apply_kurtosis, as pb_fetch's `weights` of npol = 2) is > 0 for both antenna i and antenna
 *              j.  Rows of weight 0 are still added -- their spectra are zero; the definition has no skip.
 * The sum order is fixed, so the parallelism comes from gates x channels x baseline tiles and nothing splits a gate's
 * rows: callers keep gates at or below one segment and add gates in double on the host (correlate.py does).
 * Outputs (host memory, either may be NULL): vis float32 [ngate][nbl][4][4096][2] (re, im); rows_used int32
 * [ngate][nbl][4096].
 *   pb_correlate        the gated call with ngate = nseg * rows_per_seg / int_rows and row0[g][c] = g * int_rows;
 *                       int_rows must divide nseg * rows_per_seg and need not divide rows_per_seg.  *ngate (may be
 *                       NULL) receives the number of gates.
 *   pb_correlate_gated  row0 is int32 [ngate][4096] on the host.
 *   pb_correlate_info   nbl and nprod (= 4) of the handle.
 *   pb_correlate_timers device time of the last call in ms: the kernels; the copy to the host.
 * Both run the same kernel on the SELECTED set (pb_select_set), on a stream of their own behind that set's channeliser
 * and detect, and return when their outputs have arrived -- so before anything that refills the set can be queued.  The
 * library owns and grows the device buffers and frees them in pb_destroy; pb_query's device_bytes grows by them (the
 * visibilities, rows_used, the first rows and, on the excised stream, the row counts).  No other state of the handle
 * changes: what pb_fetch returns afterwards is what it returns without the call.
 * Refused, with a pb_last_error text: PB_EINVAL for coherence = 0, a stream the handle's rfi_mode does not produce,
 * int_rows / nrows / ngate / nseg <= 0, int_rows not dividing the batch, a window out of range, nant > 8; PB_ESTATE for
 * nseg above what the set's last pb_process processed, or no pb_process on the set yet. */
#define PB_CORR_RAW 0
#define PB_CORR_KUR 1
int pb_correlate_info(const pb_handle *h, int *nbl, int *nprod);
int pb_correlate(pb_handle *h, int stream, int nseg, int int_rows, float *vis, int32_t *rows_used, int *ngate);
int pb_correlate_gated(pb_handle *h, int stream, int nseg, const int32_t *row0, int ngate, int nrows,
                       float *vis, int32_t *rows_used);
int pb_correlate_timers(const pb_handle *h, float *ms2);

/* ---- correlator with fringe stopping: pb_correlate_gated on spectra that each antenna's model has turned first.  A
 * geometric delay changes while a batch lasts (on a 36 km baseline by about a sample, and three turns of phase, per
 * second), so gates of more than a few tens of milliseconds lose the longer baselines unless every antenna's spectrum
 * is turned by a phase that follows the row BEFORE the products are added over the rows.
 * Definition (THIS project's own; tests/correlate_track_ref.py restates it): pb_correlate_tracked is pb_correlate_gated
 * with every X[a][p][t][c] replaced by X'[a][p][t][c] before the term lines.
 *   model      host binary64 [nant][4] = delay0, delay_rate, psi0, psi_rate: samples LATE at 128 MS/s, samples per row,
 *              turns, turns per row.  row_base (int64): the batch's row 0 counted from the model's epoch, so that one
 *              model continues over successive batches (batch k of T rows: row_base = k T).
 *   per (a, t) on the host in binary64, t = 0 .. T - 1, every operation rounded once, none contracted:
 *                  tau = (double)(row_base + t)
 *                  d   = delay0 + delay_rate * tau          p = psi0 + psi_rate * tau
 *                  s   = d / 12500.0
 *              The two tables s[a][t] and p[a][t] are what the device receives (at most 8 x 10240 doubles each).
 *   per (a, t, c) with k = 2155 + c, in binary64 on the device (the imager's phase):
 *                  turn = p + (double)k * s       (a multiply, then an add)        r = (float)(turn - rint(turn))
 *              (cr, sr) = the imager's rotation polynomial of r (the lines and coefficients above), then the
 *              beamformer's voltage lines with w = (cr, sr), every line one binary32 operation, no contraction; both
 *              pols of an antenna share the rotation:
 *                  x'r = xr*cr - xi*sr          x'i = xi*cr + xr*sr
 *              i.e. x exp(+2 pi i r): an antenna that is d late is aligned by its true delay (pb_beamform's sign).
 *              The model's drift within a row is ignored (about 3 10^-4 turn on 36 km).
 *   term, gates, sum order, rows_used, outputs: word for word those of pb_correlate_gated, applied to X'.
 *   pb_correlate_tracked         row0 int32 [ngate][4096] on the host, or NULL: uniform gates of nrows rows, row0[g][c] =
 *                                g * nrows; nrows must then divide the batch's rows and ngate equal their quotient.
 *   pb_correlate_tracked_timers  device time of the last call in ms: the uploads with the prefix kernel; the kernels;
 *                                the copy to the host.
 * Runs on the SELECTED set on a stream of its own behind that set's channeliser and detect and returns when its outputs
 * have arrived, as pb_correlate_gated does; its device buffers (the visibilities, rows_used, the first rows, the tables
 * and, on the excised stream, the row counts) are its own, grow on demand, count in pb_query's device_bytes and are freed
 * in pb_destroy.  No other state of the handle changes: what pb_fetch and pb_correlate return afterwards is what they
 * return without the call.
 * Refused on the host before anything is queued, with a pb_last_error text: PB_EINVAL for everything pb_correlate_gated
 * refuses (with row0 == NULL: nrows not dividing the batch or ngate not the quotient), a NULL model, a model entry that
 * is not finite, |d| or |p| above 2^24 at either end of the batch (they are linear in the row, so the ends bound them),
 * a row_base within the batch's rows of the largest int64; PB_ESTATE as for the gated call. */
int pb_correlate_tracked(pb_handle *h, int stream, int nseg, const int32_t *row0, int ngate, int nrows,
                         const double *model, int64_t row_base, float *vis, int32_t *rows_used);
int pb_correlate_tracked_timers(const pb_handle *h, float *ms3);

/* ---- imager: gated visibilities summed over delay hypotheses (reference: analysis/loc_step2.py :91-120, the scan of
 * each baseline's cross power over fractional delays, and analysis/loc_step3.py :287-348, every baseline's delay on a
 * sky grid).  Both are one operation: for each hypothesis (a "pixel": one delay and one phase per baseline) rotate each
 * baseline's 4096-channel visibility by the hypothesis's delay slope, add the channels, combine the baselines.  The
 * object is independent of pb_handle (like pb_search): the caller's visibilities are uploaded once and stay on the
 * device while they are imaged on any number of grids.
 * Definition, operation by operation (THIS project's own; tests/image_ref.py restates it in binary32 and binary64):
 *   inputs     u[b][s][c] = (ur, ui): the caller's weighted visibility of baseline b = 0..nbl-1, product slot s = 0, 1,
 *              channel c = 0..4095 (bin k = 2155 + c of the 12500-point FFT).  dd[p][b]: the delay tried for baseline b
 *              at pixel p in samples at 128 MS/s -- how much LATER the second antenna of the baseline sees the signal;
 *              dpsi[p][b]: a phase in turns (NULL: 0).  Both binary64.
 *   phase      in binary64, every operation rounded once, none contracted:
 *                  t = dpsi[p][b] + (double)k * (dd[p][b] / 12500.0)        r64 = t - rint(t)   (rint: ties to even)
 *              and r = (float)r64, |r| <= 0.5 turns.
 *   rotation   (cr, sr) ~ (cos 2 pi r, sin 2 pi r) by a fixed polynomial, every line one binary32 operation (plain
 *              multiplies and adds, no fma), the hardware's sine and cosine are not used:
 *                  q  = rintf(4.0f * r)                  (-2 .. 2: the nearest quarter turn; exact)
 *                  f  = r - q * 0.25f                    (|f| <= 1/8; both operations exact)
 *                  f2 = f * f
 *                  sn = (((S3 * f2 + S2) * f2 + S1) * f2 + S0) * f
 *                  cs = (((C4 * f2 + C3) * f2 + C2) * f2 + C1) * f2 + 1.0f
 *                  S0 =  0x1.921fb6p+2f   S1 = -0x1.4abbbap+5f   S2 =  0x1.465ec4p+6f   S3 = -0x1.2d9b7cp+6f
 *                  C1 = -0x1.3bd3ccp+4f   C2 =  0x1.03c1dep+6f   C3 = -0x1.55c64ap+6f   C4 =  0x1.d9f188p+5f
 *                  (cr, sr) = (cs, sn), (-sn, cs), (-cs, -sn), (sn, -cs) for ((int)q & 3) = 0, 1, 2, 3
 *              Largest absolute error against binary64 over every multiple of 2^-20 in [-0.5, 0.5] and 10^6 random r:
 *              0.37 x 2^-22 (tests/test_image_ref_cpu.py holds it to 2^-22).
 *   one term   every line one binary32 operation, left to right (the shape of the correlator's term):
 *                  zr = ur*cr + ui*sr          zi = ui*cr - ur*sr
 *              i.e. u exp(-2 pi i r): with u = V_ij = X_i conj(X_j) of the correlator the sum peaks where dd is
 *              d_j - d_i, the delay of antenna j behind antenna i.
 *   channels   per (p, b, s): lane l = 0..63 starts from (+0.0f, +0.0f) and adds the terms of channels l, l + 64, ..,
 *              l + 4032 in that order, re and im separately; then P[l] = P[l] + P[l + o] for o = 32, 16, 8, 4, 2, 1
 *              (the __shfl_down tree); lane 0 holds z(p, b, s).  The order depends on nothing else.
 *   per_bl     the z values, float32 [npix][nbl][2][2] (re, im).
 *   image      image[p] starts from +0.0f and adds, for b ascending and s = 0 then 1, in binary32:
 *                  PB_IMAGE_DELAY   sqrtf(zr*zr + zi*zi)   (two multiplies, an add, the correctly rounded root)
 *                  PB_IMAGE_PHASE   zr
 *              No atomics anywhere: the order is the definition.
 *   pb_imager_create   1 <= nbl <= 256, max_pix >= 1: allocates the device buffers (the visibilities, and max_pix rows
 *                      of delays, phases, z values and image values).  No HIP device: PB_EHIP.
 *   pb_imager_set_vis  u: host float32 [nbl][2][4096][2]; returns when it has been copied.
 *   pb_imager_run      1 <= npix <= max_pix; dd, dpsi: host binary64 [npix][nbl]; image (host [npix]) and per_bl may be
 *                      NULL.  Returns when the outputs have arrived.
 *   pb_imager_timers   device time of the last run in ms: upload of dd and dpsi; the kernels; the copy back.
 * Refused with a message (pb_imager_last_error; of a failed create: pb_imager_last_error(NULL)): PB_EINVAL for nbl,
 * max_pix, npix or mode out of range, a missing dd, and -- checked on the host before anything is queued -- a dd or dpsi
 * that is not finite or a |dd| > 2^24; PB_ESTATE for a run before pb_imager_set_vis. */
typedef struct pb_imager pb_imager;
#define PB_IMAGE_DELAY 0
#define PB_IMAGE_PHASE 1
int pb_imager_create(int device, int nbl, int max_pix, pb_imager **out);
void pb_imager_destroy(pb_imager *m);
const char *pb_imager_last_error(const pb_imager *m);
int pb_imager_set_vis(pb_imager *m, const float *u);
int pb_imager_run(pb_imager *m, int mode, int npix, const double *dd, const double *dpsi, float *image, float *per_bl);
int pb_imager_timers(const pb_imager *m, float *ms3);

/* ---- beamformer: phased sums of a handle's antennas, detected (reference: analysis/beamforming.py, "classical
 * beamforming" of an on-pulse against an off-pulse window, :20-24, and analysis/baseband.py apply_filter: per-channel
 * linear combinations of the antennas' spectra, then detected).  Needs coherence = 1, like the correlator, and uses the
 * delays that the correlator and the imager measure.
 * Definition, operation by operation (THIS project's own; tests/beam_ref.py restates it):
 *   inputs     X[a][p][t][c] exactly as the correlator defines it: the selected set's last batch, stream = PB_CORR_RAW or
 *              PB_CORR_KUR, t = seg * rows_per_seg + row, 0 <= t < T = nseg * rows_per_seg, bin k = 2155 + c.
 *              Per beam b = 0..nbeam-1 and antenna a (arrays [nbeam][nant], row-major):
 *                  delay[b][a]   binary64, samples at 128 MS/s that antenna a is LATE (the convention of
 *                                correlate.fit_delays' delay_samples and localise.antenna_delays)
 *                  psi[b][a]     binary64, turns; NULL: 0
 *                  gain[b][a]    binary32; NULL: 1.0f.  0 drops the antenna; a one-hot row is a single-antenna beam.
 *              Per channel: shift[c], int32 >= 0, the first row of output sample 0 (NULL: 0) -- output samples may follow
 *              a dispersed pulse (correlate.dm_row0).  tscr >= 1 rows per output sample, nout >= 1 output samples.
 *   weight     one per (b, a, c), the same for every row.  The phase is the imager's, in binary64, every operation
 *              rounded once:
 *                  t = psi[b][a] + (double)k * (delay[b][a] / 12500.0)      r = (float)(t - rint(t))
 *              (cr, sr) = the imager's rotation polynomial of r (the lines and coefficients above; the hardware's sine
 *              and cosine are not used), then, each one binary32 operation:
 *                  wr = gain * cr              wi = gain * sr
 *   voltage    per (b, p, t, c): Yr = Yi = +0.0f, then for a = 0 .. nant-1 ascending, with x = X[a][p][t][c], every line
 *              one binary32 operation, no contraction:
 *                  tr = xr*wr - xi*wi          ti = xi*wr + xr*wi
 *                  Yr = Yr + tr                Yi = Yi + ti
 *              i.e. x exp(+2 pi i r): an antenna that is d samples late carries exp(-2 pi i k d / 12500), so the true
 *              delays align the antennas.  Antennas of gain 0 are still added; their terms are +-0.
 *   detection  per (b, t, c), with A = (Ar, Ai) the voltage of pol 0 and B that of pol 1: the correlator's term lines in
 *              the order AA BB CR CI, no normalisation:
 *                  AA = Ar*Ar + Ai*Ai    BB = Br*Br + Bi*Bi    CR = Ar*Br + Ai*Bi    CI = Ai*Br - Ar*Bi
 *   integration out[b][s][q][c], q = 0..3, starts from +0.0f and adds the rows shift[c] + s * tscr + (0 .. tscr - 1) IN
 *              ROW ORDER, in binary32.  A window may cross segment boundaries; nothing splits a window's rows; no
 *              atomics: the order is the definition and depends on neither nbeam nor the launch.
 *   rows_used  int32 per (b, s, c).  Raw stream: tscr.  Excised stream: the number of the window's rows whose row weight
 *              (as pb_fetch's `weights`) is > 0 for every antenna with gain[b][a] != 0.  Rows of weight 0 are still
 *              added -- their spectra are zero.
 * Outputs (host memory, either may be NULL): beams float32 [nbeam][nout][4][4096] -- one beam's block has the layout of a
 * `nifs 4` filterbank at fp32 --; rows_used int32 [nbeam][nout][4096].
 *   pb_beamform         runs on the SELECTED set, on a stream of its own behind that set's channeliser and detect, and
 *                       returns when its outputs have arrived.  The library owns and grows its device buffers (the
 *                       weights, the outputs, the row counts) and frees them in pb_destroy; pb_query's device_bytes grows
 *                       by them.  No other state of the handle changes: what pb_fetch returns afterwards is what it
 *                       returns without the call.
 *   pb_beamform_timers  device time of the last call in ms: the uploads, weights and row counts; the beam kernel; the
 *                       copy to the host.
 * Refused, with a pb_last_error text, on the host before anything is queued: PB_EINVAL for coherence = 0, nant > 8, a
 * stream the handle's rfi_mode does not produce, nseg / tscr / nout <= 0, nbeam outside 1..64, a NULL delay, a delay, psi
 * or gain that is not finite, |delay| > 2^24, a shift < 0, a window that leaves the batch (max(shift) + nout * tscr > T),
 * outputs beyond 2 GiB; PB_ESTATE for nseg above what the set's last pb_process processed, or no pb_process on the set
 * yet. */
int pb_beamform(pb_handle *h, int stream, int nseg, int nbeam, const double *delay, const double *psi,
                const float *gain, const int32_t *shift, int tscr, int nout, float *beams, int32_t *rows_used);
int pb_beamform_timers(const pb_handle *h, float *ms3);

/* ---- projecting beamformer: pb_beamform with a free complex weight per (beam, pol, antenna, channel), given as the
 * beam's steering weights put through a matrix per (pol, channel) (reference: analysis/baseband.py apply_filter,
 * :859-908, and do_filter, :1015-1067: per channel the antennas' spectra through P = I - v v^H / (v^H v), v the
 * dominant eigenvector of their correlation matrix, i.e. an interferer's direction projected out; the reference filters
 * one VDIF thread, i.e. one pol, at a time, and so does this).  vlite-fast_amd/nulling.py makes such P from the
 * correlator's visibilities; any per-pol, per-channel calibration of the beams is the same call.
 * Definition, operation by operation (THIS project's own; tests/beamproj_ref.py restates it).  Everything pb_beamform
 * defines -- inputs, delay, psi, gain, shift, tscr, nout, the output layout -- holds here; in addition
 *   proj       host float32 [2][4096][nant][nant][2]: pol p, channel c, row a, column j, (re, im).  Any finite complex
 *              matrix per (pol, channel); it need be neither Hermitian nor a projector.
 *   steering   s[b][a][c] = (sr, si) is exactly pb_beamform's weight (wr, wi): the binary64 phase, the rotation
 *              polynomial's (cos, sin), sr = gain * cos, si = gain * sin.
 *   weight     one per (b, p, j, c): (ur, ui) = (+0.0f, +0.0f), then for a = 0 .. nant-1 ascending, with
 *              (pr, pi) = proj[p][c][a][j], every line one binary32 operation, no contraction:
 *                  tr = sr*pr - si*pi          ti = si*pr + sr*pi
 *                  ur = ur + tr                ui = ui + ti
 *              i.e. w' = s^T P, so that the beam voltage sum_j w'_j x_j is s^T (P x): apply_filter's
 *              einsum('ij,jk->ik', P, x) followed by the beam.  With P the unit matrix w' equals s as a number (signs of
 *              zero may differ), and the beams are pb_beamform's.
 *   voltage    pb_beamform's lines for antennas j = 0 .. nant-1 ascending, pol p with (wr, wi) = w'[b][p][j][c].
 *   detection, integration   pb_beamform's lines.
 *   rows_used  int32 per (b, s, c).  Raw stream: tscr.  Excised stream: the number of the window's rows whose row weight
 *              is > 0 for EVERY antenna of the handle: a matrix mixes the antennas, so a gain of 0 no longer takes an
 *              antenna out of the count (pb_beamform counts the antennas of non-zero gain only).  The same for every beam.
 * Outputs as pb_beamform's (host memory, either may be NULL).
 *   pb_beamform_proj         runs on the SELECTED set as pb_beamform does and returns when its outputs have arrived.  The
 *                            library owns and grows its device buffers (the matrices, the weights, the outputs, the row
 *                            counts: its own, not pb_beamform's) and frees them in pb_destroy; pb_query's device_bytes
 *                            grows by them.  No other state of the handle changes.
 *   pb_beamform_proj_timers  device time of the last call in ms: the uploads, weights and row counts; the beam kernel;
 *                            the copy to the host.
 * Refused, with a pb_last_error text under this call's name, on the host before anything is queued: everything
 * pb_beamform refuses, and PB_EINVAL for a NULL proj or a proj value that is not finite. */
int pb_beamform_proj(pb_handle *h, int stream, int nseg, int nbeam, const double *delay, const double *psi,
                     const float *gain, const float *proj, const int32_t *shift, int tscr, int nout,
                     float *beams, int32_t *rows_used);
int pb_beamform_proj_timers(const pb_handle *h, float *ms3);

/* ---- beam planes: the beams as filterbank planes that stay on the device, ready for pb_search_push_f32 (reference:
 * the filterbank's own fp32 plane is pow / bandpass - 1 scaled to unit variance, src/pb_kernels.cu
 * detect_and_normalize3, and the search quantises such a plane with the 8-bit rule; the rest is THIS project's own;
 * tests/beam_plane_ref.py restates it).
 * Definition, operation by operation.  Every line is one binary32 operation unless marked binary64; none is contracted
 * with another.
 *   inputs     out[b][s][q][c]: pb_beamform's block for the same arguments, bit for bit; with a non-NULL proj,
 *              pb_beamform_proj's.  used[b][s][c]: that call's rows_used (tscr on the raw stream, the respective call's
 *              count on the excised stream).  Neither leaves the device.
 *   power      per (b, s, c):   I = AA + BB      ratio = (float)tscr / (float)used      J = I * ratio
 *              At used == tscr the ratio is 1 and J = I exactly.  At used == 0 the sample has no J.
 *   level      L[b][c].  Output samples are taken in chunks of 32 consecutive s (the last chunk may be short).  Within a
 *              chunk a binary64 sum, starting from 0.0, adds (double)J in ascending s over the samples with used > 0; the
 *              chunk sums are then added in binary64, starting from 0.0, in ascending chunk order.  With n the number of
 *              samples with used > 0:
 *                  L = n > 0 ? (float)(sum / (double)n) : 0.0f               (the division in binary64)
 *              No atomics: the order is the definition and depends on neither nbeam nor the launch.
 *   plane      Le = level_in ? level_in[b][c] : L           g = sqrtf((float)(2 * tscr))
 *                  plane[b][s][c] = (used > 0 && Le > 0) ? (J / Le - 1.0f) * g : +0.0f
 *              (a division, a subtraction, a multiplication).  AA + BB over tscr rows of Gaussian voltages has
 *              std / mean = 1 / sqrt(2 tscr), so a noise plane has zero mean and unit variance: the convention of the
 *              filterbank's fp32 plane, which pb_search_push_f32 quantises with scale = 1.  The quantiser saturates at
 *              3.77 sigma, so nothing is clipped here; a sample without a valid row sits on the mean.
 * level_in   host float32 [nbeam][4096] or NULL: a level of the caller's, e.g. a running mean of earlier calls' level_out,
 *            so that batches share one scale.
 * Outputs: level_out host float32 [nbeam][4096] or NULL: L, whether or not level_in is given; planes host float32
 * [nbeam][nout][4096] or NULL; *d_planes (d_planes may be NULL): the device address of [nbeam][nout][4096] float32,
 * 16-byte aligned, as every beam's block in it is, valid until the next pb_beamform / pb_beamform_proj / pb_beam_planes
 * call on the handle or pb_destroy.
 *   pb_beam_planes         runs as pb_beamform does: on the SELECTED set, on the beam call's stream behind that set's
 *                          channeliser and detect.  The four-product block and the row counts are never copied.  It
 *                          returns with its stream drained, so the planes at *d_planes are complete: the caller meets
 *                          pb_search_push_f32's contract that the producer is synchronised.  The library owns and grows
 *                          the buffers (pb_beamform's, or pb_beamform_proj's with a proj, and the planes, levels and
 *                          chunk sums) and frees them in pb_destroy; pb_query's device_bytes follows them.  No other
 *                          state of the handle changes: pb_fetch, pb_beamform, pb_beamform_proj and their timers return
 *                          what they returned before.
 *   pb_beam_planes_timers  device time of the last call in ms: the uploads, weights and row counts; the beam kernel; the
 *                          level and plane kernels; the copies to the host.
 * Refused, with a pb_last_error text under this call's name, on the host before anything is queued: everything
 * pb_beamform refuses; with a non-NULL proj everything pb_beamform_proj refuses; PB_EINVAL for a level_in value that is
 * not finite or is negative. */
int pb_beam_planes(pb_handle *h, int stream, int nseg, int nbeam, const double *delay, const double *psi,
                   const float *gain, const float *proj, const int32_t *shift, int tscr, int nout,
                   const float *level_in, float *level_out, float *planes, const float **d_planes);
int pb_beam_planes_timers(const pb_handle *h, float *ms4);

int pb_profile(pb_handle *h, int enable);
int pb_get_timers(pb_handle *h, pb_timers *out, int reset);
int pb_debug_fetch(pb_handle *h, int what, int ant, int seg, void *dst, size_t nbytes);

/* Test hook for the flag decision (src/pb_kernels.cu:109-134, DAG_THRESH): the kernels decide "score > 3" from the
 * cube root's ARGUMENT against crossings located at pb_create and evaluate the score itself only in the few-float
 * bands around them.  For every binary32 kurtosis in [kur_lo, kur_hi] the device compares that decision with the
 * score; *nmismatch must come back 0.  bands4 (may be NULL): t_lo_sure, t_lo_clear, t_hi_clear, t_hi_sure. */
int pb_debug_dag_check(pb_handle *h, float kur_lo, float kur_hi, uint64_t *nchecked, uint64_t *nmismatch,
                       float *bands4);

/* channeliser alone, for the taps=4 parity test against polyphase_filterbank
 * (analysis/baseband.py:1207): x is nrows+taps-1 rows of 12500 float32 on the host,
 * out is nrows x 6251 complex64 (interleaved re,im). */
int pb_channelize_f32(pb_handle *h, const float *x, int nrows, int taps, float *out);

/* ---- downstream search (replaces the external heimdall for BASELINE config 5) ----
 * Brute-force incoherent dedispersion over a linear DM grid + boxcar matched filter on a block of
 * filterbank codes (SIGPROC order [time][channel], 8/4/2 bit).  Delay constant 4.148808e3 MHz^2 s
 * (src/candidate.py:33); reference = top of the band.  zap_ranges: nzap pairs [lo, hi) of channels
 * to ignore (heimdall's -zap_chans).  Parity with heimdall: unpinned (third-party, absent).
 * The band, the sample time and the DM grid are binary32 in this interface (SIGPROC headers carry doubles: the caller
 * rounds); the delays are floor(x + 0.5) of the formula evaluated in DOUBLE from those rounded values, DM i of the grid
 * being (double)dm_min + i * (double)dm_step -- a checker must round its parameters the same way, or a delay within
 * 1e-7 of a half sample lands on the other side (tests/test_gpu_search.py: random geometries). */
typedef struct pb_search pb_search;
int pb_search_create(int device, int nchan, int max_samples, float fch1_mhz, float foff_mhz, float tsamp_s,
                     float dm_min, float dm_max, float dm_step, int boxcar_max, const int *zap_ranges,
                     int nzap, pb_search **out);
/* The same over an explicit, strictly ascending list of trial DMs (e.g. search.dedisp_dm_list). */
int pb_search_create_list(int device, int nchan, int max_samples, float fch1_mhz, float foff_mhz, float tsamp_s,
                          const float *dm_list, int ndm, int boxcar_max, const int *zap_ranges, int nzap,
                          pb_search **out);
void pb_search_destroy(pb_search *s);
const char *pb_search_last_error(const pb_search *s);
int pb_search_info(const pb_search *s, int *ndm, int *nbox, int *max_delay);
/* outputs (host; any may be NULL): snr / width_log2 / series are [ndm][tout], tout = nsamp - max_delay;
 * stats is [ndm][2] = level and rms of each dedispersed series (defined under pb_search_set_baseline below).
 * codes_on_device (pb_search_run and pb_search_peaks alike): 0 = `codes` is host memory and is copied to the device
 * first; 1 = `codes` is a device address on the search's device (e.g. pb_output_dev's, or a coadder's code buffer) and
 * is read where it lies, nsamp * nchan * nbit / 8 bytes from `codes` on, by the unpacking transpose and by nothing
 * after it.  The contract of 1:
 *   - The search runs on a non-blocking stream of its own, which waits for no other stream, the null stream
 *     included: whatever produced the bytes must have finished before the call -- the caller synchronises the
 *     producer's stream (pb_sync for a pb_handle, a stream or device synchronise for anything else).  The search
 *     queues no wait of its own.
 *   - The address needs no alignment: the transpose reads single bytes, so a block may start at any byte (any time
 *     sample of a longer buffer; with 4 or 2 bits the first sample is the low bits of the first byte).
 *   - The bytes must stay valid and unchanged until the call returns.  Both entry points synchronise the search's stream
 *     before they return, so the caller may overwrite or free the buffer afterwards; the later stages (cutouts,
 *     refinement, giants, pb_search_fetch_clean) act on the search's own channel-major copy, not on `codes`.
 * The results do not depend on codes_on_device (tests/test_gpu_chain.py). */
int pb_search_run(pb_search *s, const void *codes, int codes_on_device, int nsamp, int nbit, float *snr,
                  uint8_t *width_log2, uint32_t *series, float *stats, int *tout);
/* Running baseline: the mean over `window_samples` samples around each sample is removed from every
 * dedispersed series before it is normalised (heimdall smooths its baseline over 2 s); 0 (default) = one
 * clipped mean per series. */
int pb_search_set_baseline(pb_search *s, int window_samples);
/* The normalisation, operation by operation (THIS project's own definition; heimdall's is third-party and absent).
 * For one series x[0 .. n) of exact integers (a trial DM's D[dm][.] with n = tout, or the zero-DM series z of the broad
 * RFI pass with n = nsamp) and the baseline window W = window_samples:
 *   prefix sums   P[0] = 0, P[t + 1] = P[t] + x[t], exact 64-bit integers.
 *   baseline      W > 0: the window of sample t is [lo, hi) = [t - W/2, t - W/2 + W) (W/2 rounds down).  If lo < 0 the
 *                 window is [0, min(W, n)); then, if hi > n, it is [max(0, n - W), n).  b(t) = (P[hi] - P[lo]) / (hi - lo),
 *                 the quotient of the two integers in double, rounded to binary32.
 *                 W = 0: one constant for the series, g = P[n] / n in double, rounded to binary32.
 *   residuals     v(t) = x[t] - b(t) (W > 0) or x[t] - g (W = 0), in double from the binary32 value.
 *   first pass    over all n samples: m1 = sum v / n, var1 = sum v^2 / n - m1^2, r1 = sqrt(max(var1, 0)).
 *   second pass   over the samples with |v(t) - m1| <= 3 r1 (there are cn of them; r1 = 0 keeps every sample):
 *                 m2 = sum v / cn, var2 = sum (v - m2)^2 / cn, rms = sqrt(var2 / 0.97330) -- a Gaussian clipped at
 *                 3 sigma keeps 0.9733 of its variance.  One clip, no iteration.
 *   stats[dm][0]  the level: m2 + g for W = 0 (the clipped mean of the series itself), m2 for W > 0 (what is left to
 *                 subtract on top of the running baseline; near zero).  stats[dm][1] = rms.  Both rounded to binary32.
 *   The sums are accumulated in double in an unspecified order; the values above are those of exact sums, which the
 *   double sums of at most a few 10^4 terms reproduce far below a binary32 ulp.  Where the second pass keeps only
 *   equal samples (a constant block; a blanked block with one glitch; W = 1) every v - m2 is 0 and rms is exactly 0.
 *   S/N           of the boxcar of width w = 2^k (k = 0 .. log2 boxcar_max) starting at t, defined when t + w <= n:
 *                 base = b(t + w/2) + level (W > 0: the baseline under the boxcar's middle sample) or level (W = 0);
 *                 S/N(t, w) = ((P[t + w] - P[t]) - w base) / (rms sqrt(w)), evaluated in binary32 from the binary32
 *                 level, rms and b (the integer sum is rounded to binary32 first).
 *   planes        snr[dm][t] = the largest S/N(t, w) over the widths that fit, width_log2[dm][t] = its k; of equal
 *                 S/N the narrower width wins.  When rms is not positive, snr = 0 at every t, and width_log2 is the
 *                 smallest k whose numerator (P[t + w] - P[t]) - w base is positive, 0 if none is.
 * tests/search_stats_ref.py restates this in exact / double arithmetic; tests/test_gpu_search_stats.py holds the
 * kernels to it (level and rms to 1 binary32 ulp, the planes to the rounding of the binary32 operands). */
/* The same search returning only the points at or above `threshold`: peaks[4 i ..] = DM index, sample,
 * S/N (float bits), log2 width, at most max_out of them; *npeaks = how many there were. */
int pb_search_peaks(pb_search *s, const void *codes, int codes_on_device, int nsamp, int nbit, float threshold,
                    int32_t *peaks, int max_out, int *npeaks, int *tout);
/* device time of the last run's stages in ms: H2D, transpose, dedisperse, prefix + statistics, boxcar, D2H
 * (a run with RFI cleaning: the cleaning is in none of the six, see pb_search_rfi_info) */
int pb_search_timers(const pb_search *s, float *ms6);

/* RFI cleaning before dedispersion, heimdall's narrow and broad stages (its flags -rfi_no_narrow, -rfi_no_broad,
 * -rfi_tol).  heimdall's own algorithm is third-party and absent: what follows is THIS project's deterministic
 * definition, and parity with heimdall's candidate list stays unpinned.  Off by default; when off nothing of it is
 * launched and every output is what it is without this call.
 * It runs on the channel-major u8 block xt[c][t] (after unpacking 8/4/2-bit codes), every sample t in [0, nsamp) of
 * the block, the unzapped channels only, in place; dedispersion and everything after it read the cleaned codes.
 *   narrow: per unzapped channel c, the 256-bin histogram of its nsamp codes; med_c = the smallest v whose cumulative
 *           count is >= ceil(nsamp/2); mad_c = the smallest d for which #{x : |x - med_c| <= d} >= ceil(nsamp/2).
 *           A sample is flagged when (float)|x - med_c| > tol * 1.4826f * (float)max(mad_c, 1) (binary32, left to
 *           right, no contraction) and replaced by med_c.  At 2 bits |x - med_c| <= 3 < 3 * 1.4826, so nothing is
 *           flagged with tol >= 3.
 *   broad (after narrow): z[t] = exact sum of xt[c][t] over the unzapped channels; its level and rms by the
 *           definition under pb_search_set_baseline (x = z, n = nsamp, W = the search's baseline window); the boxcar
 *           S/N and best width of widths 2^0 .. rfi_boxcar_max by the same definition.  Each t0 whose best S/N is >= tol flags [t0, t0 + its
 *           best width); every flagged t gets xt[c][t] = med_c in every unzapped channel (med_c of the narrow
 *           definition; replacing outliers by the median leaves the median unchanged).
 * Each block given to pb_search_run / pb_search_peaks is cleaned with its own statistics (heimdall cleans per gulp);
 * a stream searched in overlapping gulps has the overlap cleaned again, with the next block's statistics.
 * tol > 0 and finite (heimdall's -rfi_tol; 5 by default in search.py), rfi_boxcar_max a power of two in 1..64
 * (16 by default), else PB_EINVAL with nothing changed.  narrow = broad = 0 switches cleaning off. */
int pb_search_set_rfi(pb_search *s, int narrow, int broad, float tol, int rfi_boxcar_max);
/* the last run's cleaning: samples flagged by the narrow pass (over all channels), time samples flagged by the broad
 * pass, device time of the cleaning in ms (all 0 when the last run was not cleaned) */
int pb_search_rfi_info(const pb_search *s, uint64_t *n_narrow, int *n_broad_samples, float *ms);
/* the last run's channel-major block [nchan][nsamp] u8 after cleaning (zapped rows as transposed), for tests;
 * nbytes >= nchan * nsamp */
int pb_search_fetch_clean(pb_search *s, uint8_t *xt, size_t nbytes);

/* The cleaning's channel stage: channels that are noisy for the whole block.  A channel with persistent narrow-band
 * interference has an inflated MAD, so the narrow pass finds no outlier in it, and the broad pass looks at time samples;
 * such a channel enters every dedispersed sum at full weight.  This stage makes a per-block channel mask after IQRM
 * (inter-quartile range mitigation, Morello et al. 2022): each channel's spread is compared with its neighbours' at a
 * geometric sequence of lags, a channel whose spread is an outlier of the lagged differences is accused, and a vote
 * count keeps one abnormally quiet channel from convicting its neighbours.  The definition below is THIS project's own,
 * after IQRM; parity with any other implementation is not claimed.  Off until pb_search_set_rfi_chan; a pb_search on
 * which it was never switched on allocates nothing more, launches nothing more and returns the bytes it returns without
 * it.  Independent of pb_search_set_rfi: either, both or neither may be on.
 * Notation as under pb_search_set_cutouts: xt[c][t] the channel-major u8 block of nsamp samples, chans[0 .. nact) the
 * unzapped channels in ascending order.  The stage works on the compacted index a = 0 .. nact - 1, so a zapped range
 * simply brings its two neighbours next to each other.  Everything is exact integer arithmetic except the one
 * comparison marked binary64.
 *   moments   of the block as handed to the search, before the narrow and broad passes, over t in [0, nsamp), 64-bit:
 *             sum[a] = sum_t x, sq[a] = sum_t x^2, x = xt[chans[a]][t].
 *             S[a] = nsamp sq[a] - sum[a]^2: nsamp^2 times the variance; nsamp is the same for every channel, so the
 *             S[a] compare like variances without a division.
 *             fill[a] = (2 sum[a] + nsamp) / (2 nsamp), integer division: the rounded mean.
 *   lags      l = 1; while l <= radius: take +l, then -l; l = max(l * 3 / 2, l + 1), integer division.  radius = 0
 *             means max(1, nact / 10).
 *   outliers  of one signed lag L: j(a) = min(max(a - L, 0), nact - 1); d[a] = S[a] - S[j(a)], int64.  With the nact
 *             values of d sorted ascending: q1 = d_sorted[(nact - 1) / 4], med = d_sorted[(nact - 1) / 2],
 *             q3 = d_sorted[3 (nact - 1) / 4], integer division, no interpolation (only values are used, so ties are
 *             harmless).  Channel a is an outlier of lag L iff
 *                 (double)(d[a] - med) > (double)tol * ((double)(q3 - q1) / 1.349)
 *             -- the differences in int64 first, then one conversion each, one quotient and one product in binary64,
 *             none contracted; tol is the binary32 argument widened.  One-sided: high spread only.
 *   votes     for every (L, a) with a an outlier of L: recv[a] += 1 and cast[j(a)] += 1.  Integer counts over all lags,
 *             independent of any order.
 *   mask      flag[a] = 1 iff there is at least one such (L, a) with cast[j(a)] <= recv[a]: the accuser must not have
 *             accused more channels than the accused has accusers.  One pass, no iteration.
 *   fill      every flagged channel becomes xt[chans[a]][t] = fill[a] for t in [0, nsamp), in place, before the narrow
 *             and broad passes, which then run, if switched on, exactly as they do on any block (a constant channel has
 *             MAD 0 and no outlier).  Zapped channels and samples at or beyond nsamp are not touched.
 * Consequences.  Everything after the cleaning reads the filled block, as with the existing cleaning: dedispersion,
 * statistics, boxcars, giants, cutouts, refinement, the sub-band search, pb_search_fetch_clean.  With polarisation on
 * the stage changes xt only; the four product planes stay what the file held.  nact and the delay table are unchanged:
 * a flagged channel contributes a constant to every series.
 * Streaming.  A gulp call cleans the accumulated block in place once, under the rules of pb_search_gulp_peaks: the raw
 * tail is put aside first and handed on raw, a second call on the same block keeps the first call's mask, and the next
 * gulp makes its own mask from its own block.
 * pb_search_set_rfi_chan(s, radius, tol): tol > 0 switches the stage on (search.py's default: radius 0, tol 4), tol == 0
 * switches it off and frees its buffers.  PB_EINVAL with nothing changed for radius < 0 or radius > nact, for a tol that
 * is negative or not finite, and for a handle beyond what the kernels are built for: max_samples > 8 388 608 (a lane's
 * 32-bit partial sums of x^2, and 255^2 nsamp^2 < 2^63 for S) or nact > 8192 (the sort's 64 KiB of LDS).
 * tests/search_rfichan_ref.py restates the definition; tests/test_gpu_search_rfichan.py holds the kernels to it exactly. */
int pb_search_set_rfi_chan(pb_search *s, int radius, float tol);
/* the last block's channel stage (host, any pointer may be NULL): *nflag = flagged channels; mask u8 [nchan], sum and
 * stat (= S) i64 [nchan], recv and cast i32 [nchan], fill u8 [nchan], all in file channel numbering and 0 for zapped
 * channels; *ms = device time of the stage, from events of its own.  Everything is 0 when the last block did not go
 * through the stage.  pb_search_timers keeps its meaning (the stage lies inside the cleaning window that its third
 * entry excludes), and so does pb_search_rfi_info: its ms is the narrow and broad passes'. */
int pb_search_rfi_chan_info(pb_search *s, int *nflag, uint8_t *mask, int64_t *sum, int64_t *stat, int32_t *recv,
                            int32_t *cast, uint8_t *fill, float *ms);

/* Per-candidate cutouts of the LAST block given to pb_search_run / pb_search_peaks, taken from what is still on the
 * device: the dedispersed frequency-time image of an event and its DM-time "bow tie".  heimdall writes no such images:
 * the definition is THIS project's own, every value an exact integer.  Off until pb_search_set_cutouts; a pb_search on
 * which it was never called allocates nothing more, launches nothing more and returns what it returns without it.
 * Notation: nsamp samples in the block, tout = nsamp - max_delay; xt[c][t] the channel-major u8 block after unpacking
 * and, if switched on, after RFI cleaning; delay[dm][c] the integer delays of the unzapped channels as the search uses
 * them; D[dm][t] the dedispersed series (pb_search_run's `series`); nact the number of unzapped channels.
 * Geometry: nsub frequency subbands (nchan % nsub == 0; subband s = channels [s nchan/nsub, (s+1) nchan/nsub), zapped
 * channels in it contribute nothing), nt time bins (even), ndmrow DM rows (even).
 * A request is (dmi, t_pk, tscr): trial-DM index in [0, ndm), peak sample in block coordinates in [0, tout), time-scrunch
 * factor, a power of two in 1..64.  Bin j covers the block samples T(j) = [t_pk + (j - nt/2) tscr,
 * t_pk + (j - nt/2 + 1) tscr): a boxcar that starts at t_pk starts at the left edge of bin nt/2.
 *   ft[s][j]      = sum over the unzapped channels c of subband s and t in T(j) of xt[c][t + delay[dmi][c]], over the
 *                   terms with 0 <= t + delay[dmi][c] < nsamp only (t itself may lie outside [0, tout); bytes of the
 *                   buffer at or beyond nsamp, stale from earlier blocks, are never summed)
 *   ft_hits[s][j] = the number of such terms
 *   dt[k][j]      = sum over t in T(j) with 0 <= t < tout of D[dmi - ndmrow/2 + k][t]; 0 where that DM index is outside
 *                   [0, ndm)
 *   dt_hits[k][j] = the number of samples summed (0 for a row outside the grid)
 * all u32 (4096 channels x 64 samples x 255 < 2^32).  Means are ft / ft_hits and dt / (dt_hits nact), left to the
 * reader.  For a bin whose samples all lie in [0, tout): sum_s ft[s][j] == dt[ndmrow/2][j] and
 * sum_s ft_hits[s][j] == nact tscr; dt at tscr 1 is a crop of `series`.
 * pb_search_set_cutouts allocates the device and page-locked host buffers for up to max_cands requests per call;
 * max_cands = 0 frees them and switches cutouts off.  PB_EINVAL with nothing changed for nchan % nsub != 0, odd or
 * non-positive nt / ndmrow, nt * 64 > max_samples (or nt > 8192: the bins are kept in LDS), max_cands < 0, or buffers
 * beyond 2 GiB. */
int pb_search_set_cutouts(pb_search *s, int nsub, int nt, int ndmrow, int max_cands);
/* cands3: n triples (dmi, t_pk, tscr).  Outputs (host, any may be NULL): ft, ft_hits [n][nsub][nt]; dt, dt_hits
 * [n][ndmrow][nt].  Runs on the search's stream after the run it refers to; one device-to-host copy per call.
 * PB_EINVAL before anything is launched or written when cutouts are off, no block has been searched yet, n > max_cands
 * or a triple is out of range (message: pb_search_last_error). */
int pb_search_cutouts(pb_search *s, const int32_t *cands3, int n, uint32_t *ft, uint32_t *ft_hits, uint32_t *dt,
                      uint32_t *dt_hits);
/* device time of the last pb_search_cutouts in ms: the two kernels; the kernels and the copy to the host */
int pb_search_cutout_timers(const pb_search *s, float *ms2);

/* A candidate's DM, width and S/N refined on the device, from the LAST block given to pb_search_run / pb_search_peaks:
 * what the reference does after a trigger (analysis/loc_step0.py: optimize_pulse, refine_dm with analysis/utils.py's
 * tophat_smooth and qn), with the reference's own estimators, on fine trial DMs about the candidate.  Off until
 * pb_search_set_refine; a pb_search on which it was never called allocates nothing more, launches nothing more and
 * returns exactly what it returns without it.
 * Geometry: nstep fine trial DMs per request (32 by default in search.py), half_window H samples (128: the reference's
 * 0.2 s at 781.25 us), wmax (32; the width pass tries the nw = wmax / 2 odd widths 1, 3, .. wmax - 1; M = wmax / 2).
 * A request is (t_pk, width; dm_lo, dm_step): peak sample in block coordinates in [0, tout), width in 1 .. wmax -- an
 * even width becomes width + 1 before anything else, as tophat_smooth makes it, and that odd number is the `width` of
 * everything below (refine_dm itself would still scale by the even one; it is only ever given odd widths) -- and two
 * binary32 numbers.  Fine trial k = 0 .. nstep - 1 has DM (double)dm_lo + k * (double)dm_step and the delays the search
 * itself would give that DM: the formula in double, floor(d + 0.5), the unzapped channels, the top of the band as the
 * reference (one function makes both tables).  A trial whose DM is below 0 or above the grid's last trial DM is not
 * evaluated: its sn_dm is NaN, its series 0, and it cannot win.
 * Definition, T = tout of the last run, window [i0, i1) = [max(0, t_pk - H), min(T, t_pk + H)), n = i1 - i0:
 *   q_k[t]          exact sum over the unzapped channels c of xt[c][t + delay_k[c]], t in [0, T) (xt as the search
 *                   dedispersed it: cleaned if cleaning is on).
 *   smooth(q, t, w) (sum of q over [t - h, t + h]) / (2 h + 1), h = min(w / 2, t, T - 1 - t) (w / 2 rounds down): the
 *                   quotient of the integers in double.  tophat_smooth on the whole series, edge ramps included.
 *   med(x)          the median; the mean of the two middle values for an even count.  An integer or a half-integer.
 *   qn(x)           2.2219 x the 25th percentile of all N (N - 1) / 2 absolute pair differences, interpolated linearly as
 *                   np.percentile does: with the differences ascending, d[r] + (f / 4) (d[r + 1] - d[r]) where
 *                   N (N - 1) / 2 - 1 = 4 r + f, 0 <= f < 4.  A multiple of 1/4 (exact) times 2.2219 (one rounding).
 *   DM pass (refine_dm):   sn_dm[k] = (max over t in [i0, i1) of smooth(q_k, t, width) - med(q_k[i0:i1]))
 *                                     / (qn(q_k[i0:i1]) / sqrt(width)),   0 where that qn is 0 (THIS project's rule;
 *                   the reference divides by zero).  kbest = the first k with the largest sn_dm among the evaluated
 *                   trials; -1 (and NaN / -1 from the width pass) when no trial of the request was evaluated.
 *   width pass (optimize_pulse) on q = q_kbest: the off-pulse samples q[i0 : i0 + n/4] joined with q[i0 + 3n/4 : i1]
 *                   (both quotients round down) give med and qn.  For each odd w = 1, 3, .. wmax - 1 the plain w-sample
 *                   mean centred on t, (sum of q over [t - w/2, t + w/2]) / w, over t in [i0 + w, i1 - w); its first
 *                   maximum, at t*, gives opt_loc = t* - i0 and opt_sn = (mean - med) / qn * sqrt(w), 0 where qn is 0.
 *   Order statistics and sums are exact; the S/N are evaluated in double as written (IEEE, no contraction).
 *   status          0, or 1 when n < 4 wmax (a window clipped by the block's ends to less than that): nothing is
 *                   computed for that request, sn_dm and opt_sn are NaN, kbest and opt_loc -1, its series 0.
 * tests/search_refine_ref.py restates this in NumPy; tests/golden/reference_refine.npz holds what the reference's own
 * functions return on seeded planes, and tests/test_search_refine_cpu.py ties the two together.
 * pb_search_set_refine allocates the device and page-locked host buffers for up to max_cands requests per call;
 * max_cands = 0 frees them and switches refinement off.  PB_EINVAL with nothing changed for nstep outside 1..4096, wmax
 * odd or outside 2..64, half_window < 2 wmax, half_window + wmax / 2 > 1024 (the statistics hold a series in LDS),
 * max_cands < 0 or buffers beyond 1 GiB. */
int pb_search_set_refine(pb_search *s, int nstep, int half_window, int wmax, int max_cands);
/* req_i2: n pairs (t_pk, width); req_f2: n pairs (dm_lo, dm_step).  Outputs (host, any may be NULL): status [n],
 * sn_dm [n][nstep], kbest [n], opt_sn [n][nw], opt_loc [n][nw]; series (for tests) [n][nstep][2 (H + M)] u32 = q_k over
 * [t_pk - H - M, t_pk + H + M), 0 outside [0, T).  Runs on the search's stream after the run it refers to; one
 * device-to-host copy per call, through page-locked memory.  PB_EINVAL before anything is launched or written when
 * refinement is off, no block has been searched yet, n > max_cands or a request is out of range (t_pk outside [0, tout),
 * width outside 1..wmax, dm_lo or dm_step not finite; message: pb_search_last_error). */
int pb_search_refine(pb_search *s, const int32_t *req_i2, const float *req_f2, int n, int32_t *status, double *sn_dm,
                     int32_t *kbest, double *opt_sn, int32_t *opt_loc, uint32_t *series);
/* device time of the last pb_search_refine in ms: the three kernels; the kernels and the copy to the host */
int pb_search_refine_timers(const pb_search *s, float *ms2);

/* Polarisation of a candidate: the search on the four-product filterbank that pb_create's `coherence` writes (AA, BB, CR,
 * CI; SIGPROC nifs 4), and for the candidates of a block -- from what is still on the device -- the four frequency-time
 * images, the on- and off-pulse spectra and an RM synthesis over a grid of trial rotation measures.  The definition is
 * THIS project's own.  Off until pb_search_set_pol; a pb_search on which it was never called allocates nothing more,
 * launches nothing more and returns the bytes it returns without it.
 * Notation: nsamp, tout, delay[dm][c], the unzapped channels (nact of them) as under pb_search_set_cutouts;
 * f_c = fch1 + c foff in MHz (double, from the binary32 band of pb_search_create); lambda2_c = (299.792458 / f_c)^2 in m^2,
 * in double as written (one quotient, one product).
 * Input.  While the stage is on, every block given to pb_search_run / pb_search_peaks is [nsamp][4][nchan] 8-bit codes, the
 * four in the order AA, BB, CR, CI -- the row order of a nifs 4 SIGPROC file -- nsamp * 4 * nchan bytes, for host and device
 * pointers alike (the contract of codes_on_device = 1 holds; a device block whose address and nchan are multiples of 4 is
 * read with 4-byte loads, any other byte by byte, the result is the same).  Refused, PB_EINVAL with nothing launched or
 * written: nbit != 8 while the stage is on; pb_search_push, pb_search_push_f32 and the pb_search_gulp_* calls while it is on
 * (streaming cannot be on with it: pb_search_set_gulp is refused while this stage is on, and this stage while streaming
 * is).  Searching 4-IF data in the streaming path is left for later.
 * Planes.  k_transpose_pol turns the block into five channel-major u8 planes of the search's pitch: xa, xb, xcr, xci,
 * each [c][t], and the search plane xt[c][t] = (aa + bb + 1) >> 1, the rounded mean in integer arithmetic: total intensity
 * at 8-bit depth (255 and 255 give 255).  From xt on the search is byte for byte what it is on a 1-IF block of those
 * codes: RFI cleaning, dedispersion, statistics, boxcars, peaks, giants, cutouts and refinement all read xt.  RFI cleaning
 * changes xt ONLY: the four product planes are what the file held, flagged samples included.
 * Images.  Geometry (nsub, nt) and request (dmi, t_pk, tscr) of pb_search_set_cutouts.  pft[k][s][j], k = 0..3, is exactly
 * ft[s][j] of that definition with the plane of product k in place of xt; pft_hits[s][j] is ft_hits, the same for all four.
 * Spectra.  A request is (dmi, t_pk, w), w in 1..64.  The on window is T_on = [t_pk, t_pk + w); the off windows are
 * [t_pk - g - L, t_pk - g) and [t_pk + w + g, t_pk + w + g + L), guard g in 0..1024 and off length L in 1..1024 set with the
 * stage.  For every unzapped channel c and product k: on[k][c] = sum over t in T_on of plane_k[c][t + delay[dmi][c]], over the
 * terms with 0 <= t + delay < nsamp only; non[c] = the number of such terms; off[k][c], noff[c] the same over the two off
 * windows together.  All i32, exact.  Zapped channels give 0 in all four.
 * Stokes per channel, in double, each line one operation, left to right, none contracted:
 *     m_k = on[k] / non - off[k] / noff        (two quotients, one difference)
 *     i_c = m_AA + m_BB      q_c = m_AA - m_BB      u_c = 1.4142135623730951 m_CR      v_c = 1.4142135623730951 m_CI
 * The sqrt 2 undoes the one that the coherence detection puts on CR and CI, so U = 2 Re(A B*) /
 * sqrt(bpA bpB) is in the units of AA' - BB'; the quantiser's offset cancels in on minus off.
 *     w_c = 1 where the channel is unzapped and non > 0 and noff > 0, else 0;   W = sum w_c
 * RM synthesis.  lambda0^2 = (sum_c w_c lambda2_c) / W.  Trials phi_k = rm_lo + k rm_step, k = 0 .. nrm - 1 (doubles; nrm in
 * 1..8192).
 *     F[k] = (1 / W) sum_c w_c (q_c + i u_c) exp(-2 i phi_k (lambda2_c - lambda0^2))
 * with theta = (2 phi_k) (lambda2_c - lambda0^2) (the doubling exact, one product), its sine and cosine the device
 * library's, re += q cos + u sin, im += u cos - q sin (two products and a sum, then the accumulation), the two sums divided
 * by W at the end.  Every sum over c is sequential in ascending c, in double.  kbest = the first k with the largest
 * re^2 + im^2.  F is [n][nrm][2], re then im.  summary[6] per request = W, lambda0^2, mean_c i_c, mean_c v_c (over the
 * channels with w_c = 1: the sequential sum, divided by W), |F[kbest]| = sqrt(re^2 + im^2), phi_kbest.  A request with
 * W = 0 gets NaN for F and for summary[1..5], and kbest = -1.  The reader gets L/I = summary[4] / summary[2],
 * V/I = summary[3] / summary[2], and the position angle at lambda0 = atan2(Im F[kbest], Re F[kbest]) / 2.
 * What it is NOT: calibrated.  The bandpass normalisation is per hand; leakage, cross-hand delay and phase, handedness and
 * the parallactic angle are left in; the sign of V is that of CI = Im(A conj B).  No significance of L
 * or of the RM peak is given.
 * tests/search_pol_ref.py restates this in NumPy; tests/test_gpu_search_pol.py holds the kernels to it (planes, images and
 * spectra exactly; F and summary to the rounding of double worked out there).
 * pb_search_set_pol allocates the four planes, the device staging of a host block and the device and page-locked buffers
 * for up to max_cands requests per call; max_cands = 0 frees them and returns the search to 1-IF input.  PB_EINVAL with
 * nothing changed for values out of range (off_len, guard, nrm as above; rm_lo, rm_step finite; max_cands >= 0), for
 * streaming being on, or for buffers beyond 2 GiB. */
int pb_search_set_pol(pb_search *s, int off_len, int guard, int nrm, double rm_lo, double rm_step, int max_cands);
/* req3: n triples (dmi, t_pk, w).  Outputs (host, any may be NULL): on, off [n][4][nchan] i32; non, noff [n][nchan] i32;
 * F [n][nrm][2] f64; kbest [n] i32; summary [n][6] f64.  Runs on the search's stream after the run it refers to; one
 * device-to-host copy per call, through page-locked memory.  PB_EINVAL before anything is launched or written when the stage
 * is off, no four-product block has been searched yet, n > max_cands or a request is out of range (dmi outside [0, ndm),
 * t_pk outside [0, tout), w outside 1..64; message: pb_search_last_error). */
int pb_search_pol(pb_search *s, const int32_t *req3, int n, int32_t *on, int32_t *non, int32_t *off, int32_t *noff, double *F,
                  int32_t *kbest, double *summary);
/* cands3: n triples (dmi, t_pk, tscr) as for pb_search_cutouts.  Outputs (host, either may be NULL): pft [n][4][nsub][nt],
 * pft_hits [n][nsub][nt] u32.  Needs both cutouts and this stage switched on, n <= the smaller of their max_cands; its
 * buffers are remade whenever either of the two set calls has changed.  Refused like pb_search_cutouts. */
int pb_search_pol_cutouts(pb_search *s, const int32_t *cands3, int n, uint32_t *pft, uint32_t *pft_hits);
/* plane `which` (0..3 = AA, BB, CR, CI) of the last block, [nchan][nsamp] u8, for tests; nbytes >= nchan * nsamp.
 * pb_search_fetch_clean keeps returning xt. */
int pb_search_pol_fetch(pb_search *s, int which, uint8_t *out, size_t nbytes);
/* device time in ms of the last transposition into the five planes, of the last pb_search_pol's kernels, and of those
 * kernels with the copy to the host */
int pb_search_pol_timers(const pb_search *s, float *ms3);

/* Giants and clusters of giants: the last run's S/N planes turned into candidates on the device, the step heimdall
 * takes after its matched filter (its giant finder and its labelling of giants over -cand_sep_time / -cand_sep_dm /
 * -cand_sep_filter).  heimdall's source is third-party and absent: what follows is THIS project's definition, exact,
 * independent of the order anything runs in, and bounded in memory; parity with heimdall's list stays unpinned.  Off
 * until pb_search_set_giants; a pb_search on which it was never called allocates nothing more, launches nothing more
 * and returns what it returns without it.
 * Inputs: the planes snr[d][t] (binary32) and wl[d][t] (log2 width, u8) of the last pb_search_run / pb_search_peaks (or of
 * pb_search_set_planes), d in [0, ndm), t in [0, tout); a threshold, binary32; a sample range 0 <= t_lo < t_hi <= tout;
 * sep_time in 1..64, sep_dm >= 0 (in trial-DM indices), sep_filter >= 0 (3 / 200 / 3 by default in search.py: heimdall's
 * defaults as far as known, unpinned).
 * Giants:
 *   1. A sample is hot when t_lo <= t < t_hi and snr[d][t] >= thresh, compared in binary32; a NaN is not hot.
 *   2. A giant is a maximal set of hot samples of one series in which consecutive hot samples are at most sep_time apart.
 *   3. Its fields: dmi; begin, the first hot sample; end, the last hot sample + 1; npts, the number of hot samples;
 *      peak, the hot sample with the largest S/N, the smallest t among equals (-0 equals +0); snr = snr[dmi][peak], bit
 *      for bit; tfilt = wl[dmi][peak].
 *   4. The giant list is in ascending (dmi, begin) order, whatever order the workgroups ran in.
 * Links and clusters:
 *   5. Giants a and b are linked when |dmi_a - dmi_b| <= sep_dm, |tfilt_a - tfilt_b| <= sep_filter,
 *      begin_a < end_b + sep_time and begin_b < end_a + sep_time.  Two giants of one series therefore never link directly.
 *   6. Clusters are the connected components of that relation.  A cluster's label is its smallest member index.
 * Candidates:
 *   7. One candidate per cluster.  The member with the largest S/N gives snr, peak, tfilt and dmi; ties go to the smallest
 *      giant index.
 *   8. members is the number of giants in the cluster, npoints the sum of their npts, i0 the smallest begin, i1 the largest
 *      end.
 *   9. The device table is in label order.  The host (search.py) sorts it strongest first, ties broken by (dmi, peak).
 * Overflow:
 *  10. If the number of giants G exceeds max_giants the call succeeds, reports G exactly and an overflow flag, and returns
 *      no candidates (heimdall's -max_giant_rate behaviour: the gulp is given up, deterministically).  G is known from a
 *      counting pass before anything is written.
 * Gulps:
 *  11. A run of hot samples cut by t_hi (or t_lo) is two giants in two calls: a call knows nothing of samples outside its
 *      range.
 * No floating-point arithmetic takes part, only comparisons of binary32 values: tests/search_giants_ref.py restates this
 * in NumPy and tests/test_gpu_search_giants.py holds the kernels to it field by field, exactly.
 * A giant is PB_GIANT_WORDS int32: dmi, begin, end, npts, peak, S/N bits, tfilt, label.  A candidate is PB_GIANT_WORDS
 * int32: S/N bits, peak, tfilt, dmi, members, npoints, i0, i1.
 * pb_search_set_giants allocates the device and page-locked host buffers for up to max_giants giants per call;
 * max_giants = 0 frees them and switches the stage off.  PB_EINVAL with nothing changed for sep_time outside 1..64, a
 * negative sep_dm or sep_filter, max_giants outside 0..2^22, or ndm x max_samples >= 2^31 (the counts are 32-bit). */
#define PB_GIANT_WORDS 8
int pb_search_set_giants(pb_search *s, int sep_time, int sep_dm, int sep_filter, int max_giants);
/* On the planes that are on the device: cands (host) receives min(*ncands, max_out) candidates in label order; *ngiants =
 * G, *overflow = 1 when G > max_giants (then *ncands = 0).  Runs on the search's stream; the host waits once for G (it
 * sizes the grids) and once per labelling sweep for the "a label changed" word; the results come back in one copy through
 * page-locked memory.  PB_EINVAL before anything is launched or written when the stage is off, there are no planes yet, the
 * range is bad, the threshold is a NaN or an output pointer is missing (message: pb_search_last_error). */
int pb_search_giants(pb_search *s, float thresh, int t_lo, int t_hi, int32_t *cands, int max_out, int *ncands, int *ngiants,
                     int *overflow);
/* the giants of the last pb_search_giants with their labels (none after an overflow): out receives min(*n, max_out) of
 * them; for tests and diagnostics */
int pb_search_giant_list(pb_search *s, int32_t *out, int max_out, int *n);
/* Replaces the planes on the device with host planes snr, width_log2 [ndm][tout], 1 <= tout <= max_samples: stored planes
 * can be clustered again, and tests put hand-made patterns in front of the kernels.  The block, its dedispersed series
 * and what cutouts and refinement read stay as the last run left them. */
int pb_search_set_planes(pb_search *s, const float *snr, const uint8_t *width_log2, int tout);
/* the last pb_search_giants: device time in ms of the giant pass (count, scan, write), of the labelling and the merge,
 * and of everything with the copy to the host; *nsweeps (may be NULL) = hook / jump sweeps of the labelling */
int pb_search_giant_timers(const pb_search *s, float *ms3, int *nsweeps);

/* Streaming: a gulp accumulated on the device from pieces of any length, and its dispersion tail handed on without
 * leaving the device.  In production the search stands behind the filterbank, which leaves one second of code bytes in
 * device memory at a time; heimdall gathers 30720 samples into a gulp and searches it together with the end of the
 * stream before it.  Off until pb_search_set_gulp; a pb_search on which it was never called allocates nothing more,
 * launches nothing more and gives the results it gave before.
 * The accumulated block IS the search's channel-major block xt[c][t] (u8, c in [0, nchan), pitch >= max_samples), the
 * one that pb_search_run / pb_search_peaks fill with their transpose; `fill` counts the samples per channel that it
 * holds.  Every entry below returns PB_EINVAL with a message (pb_search_last_error) and changes nothing when the stage
 * is off, when there is no handle ("no search handle"), or in the cases named with it.
 *   pb_search_set_gulp(s, keep_max)  switches the stage on with an empty block (fill = 0) and allocates the side buffer
 *           of nchan x keep_max bytes; keep_max = the most samples that pb_search_gulp_advance may hand on.  0 switches
 *           the stage off and frees the buffer.  Refused: keep_max < 0 or > max_samples.
 *   pb_search_push(s, codes, codes_on_device, nsamp, nbit, &fill)  appends nsamp samples in SIGPROC order
 *           [time][nchan], nbit in {8, 4, 2}, low bits first within a byte -- what pb_search_run accepts --:
 *           xt[c][fill + t] = sample (t, c) for t in [0, nsamp), then fill += nsamp; *fill (may be NULL) = the new fill.
 *           codes_on_device = 0: host bytes, staged through the buffer that pb_search_run stages its host blocks
 *           through.  1: device bytes read where they lie, under the contract of pb_search_run: the producer synchronised
 *           by the caller, any byte address, nothing read outside [codes, codes + nsamp * nchan * nbit / 8).  The call
 *           returns when the bytes have been consumed.  Successive pushes may differ in nbit and in where their bytes
 *           lie.  A source whose address and row length nchan * nbit / 8 are multiples of 16 bytes (pb_output_dev, a
 *           coadder's code buffer, the staging buffer) is read with 16-byte loads, any other byte by byte; the result
 *           is the same.  nsamp = 0 appends nothing.  Refused, appending nothing: a bad nbit; fill + nsamp >
 *           max_samples; nsamp * nchan * nbit not a multiple of 8 (a piece ends on a byte); a push onto a block that a
 *           gulp call has cleaned in place (see below: advance first).
 *   pb_search_gulp_peaks(s, threshold, peaks, max_out, &npeaks, &tout), pb_search_gulp_run(s, snr, width_log2, series,
 *           stats, &tout)  what pb_search_peaks / pb_search_run do on a block of nsamp = fill samples, from the RFI
 *           cleaning on (the same kernels), with the same outputs and the same refusals, fill - max_delay < 64 among
 *           them.  Afterwards cutouts, refinement, giants, pb_search_fetch_clean and pb_search_timers (its first two
 *           entries: nothing, and putting the raw tail aside) behave as after pb_search_peaks, block coordinates being
 *           positions in the accumulated block.  fill is unchanged, and a second call without a push in between returns
 *           the same bytes.  With cleaning on (pb_search_set_rfi) the block is cleaned in place, once: the raw samples
 *           [fill - min(keep_max, fill), fill) are first copied to the side buffer, a second call reads the block as the
 *           first one left it (the cleaning and its counts are the first call's; a pb_search_set_rfi in between takes
 *           effect after the next advance), and until pb_search_gulp_advance the raw block no longer exists:
 *           pb_search_push and pb_search_gulp_fetch are refused.
 *   pb_search_gulp_advance(s, keep)  the raw samples [fill - keep, fill) of every channel -- as pushed, not as cleaned --
 *           become the samples [0, keep), and fill = keep.  Refused: keep < 0, keep > fill, keep > keep_max.  Device
 *           copies only; where source and destination overlap (keep > fill - keep) or the block was cleaned, the samples
 *           go through the side buffer, so the move is exact whatever order a copy works in.
 *   pb_search_gulp_fetch(s, xt, nbytes, &fill)  the raw accumulated block [nchan][fill] -> host (tests, debugging a
 *           host); nbytes >= nchan * fill.
 *   pb_search_gulp_timers(s, ms3)  device time in ms of the last push's copy to the device (0 for device bytes) and
 *           append, and of the last advance.
 * pb_search_run / pb_search_peaks on a handle with the stage on overwrite the block as they always did, give their usual
 * results, and leave the stage empty (fill = 0).
 * tests/test_gpu_search_stream.py: the block equals the unpacked concatenation of the pieces however they are cut,
 * packed and placed, and a stream fed in pieces gives the candidates of the same stream searched in whole host gulps. */
int pb_search_set_gulp(pb_search *s, int keep_max);
/* The same append from an fp32 plane, quantised to 8 bits on the way: the search at 8-bit depth behind a filterbank that
 * writes 2 or 4 bits.  `plane` is nsamp samples in SIGPROC order [time][nchan] of binary32 -- pb_output_dev's `ave` at
 * npol = 1 (needs keep_ave; contiguous over a batch's segments), or a coadder's d_sum.  For t in [0, nsamp), c in
 * [0, nchan), every line one binary32 or binary64 operation, none contracted with another:
 *     v   = plane[t * nchan + c] * scale                      (binary32)
 *     tmp = (float)((double)v / 0.02957 + 127.5)              (binary64 quotient, binary64 sum, rounded to binary32)
 *     q   = tmp > 0 ? (tmp >= 255 ? 255 : (uint8_t)tmp) : 0   (the cast truncates)
 *     xt[c][fill + t] = q
 * then fill += nsamp; *fill (may be NULL) = the new fill.  For every v that is not a NaN this is sel_and_dig_8b
 * (src/pb_kernels.cu:711-735), the arithmetic of pb_coadd_digitise at 8 bits: with scale = 1 the block is the one that
 * an nbit = 8 handle's codes would have given, with scale = (float)(1 / sqrt(N)) the one that pb_coadd_finish's codes
 * would.  A NaN (a segment of dropped frames, tools/nan_codes_check.py) gives 0: the comparison is written `tmp > 0`.
 * scale must be finite and > 0 (1 is exact).
 * plane_on_device = 1: read where it lies under the contract of pb_search_run (the caller synchronises the producer;
 * valid until return; nothing read outside [plane, plane + nsamp * nchan)); the address must be a multiple of 4, and one
 * that is a multiple of 16 with nchan a multiple of 4 is read with 16-byte loads -- the result is the same.
 * plane_on_device = 0: host floats, staged through the buffer that pb_search_run stages its host blocks through
 * (max_samples * nchan bytes) in slices of max_samples / 4 samples; nothing more is allocated.  The call returns when the
 * plane has been consumed.  pb_search_gulp_timers reports it like a pb_search_push (the slices' times added up).
 * Pushes of planes and of codes of any depth may alternate within one gulp; a handle on which this is never called
 * allocates and launches what it did before.  Refused (PB_EINVAL, fill and block unchanged): what pb_search_push refuses
 * (the stage off, no handle, nsamp < 0, fill + nsamp > max_samples, a block cleaned in place); a scale that is not
 * finite or not > 0; a device plane at an address that is not a multiple of 4.
 * tests/test_gpu_search_plane.py: the block equals the NumPy restatement (tests/search_plane_ref.py, itself pinned to
 * the oracle's sel_and_dig_8b) for every alignment, source and scale. */
int pb_search_push_f32(pb_search *s, const float *plane, int plane_on_device, int nsamp, float scale, int *fill);
int pb_search_push(pb_search *s, const void *codes, int codes_on_device, int nsamp, int nbit, int *fill);
int pb_search_gulp_peaks(pb_search *s, float threshold, int32_t *peaks, int max_out, int *npeaks, int *tout);
int pb_search_gulp_run(pb_search *s, float *snr, uint8_t *width_log2, uint32_t *series, float *stats, int *tout);
int pb_search_gulp_advance(pb_search *s, int keep);
int pb_search_gulp_fetch(pb_search *s, uint8_t *xt, size_t nbytes, int *fill);
int pb_search_gulp_timers(const pb_search *s, float *ms3);

/* Sub-band search: band-limited bursts.  The search sums every unzapped channel before it looks for a pulse, so a burst
 * that lives in a quarter of the band reaches half the S/N it has in its own quarter and may never cross the threshold.
 * This stage searches runs of base sub-bands of the block that the last search left on the device and reports the cells
 * where a band beats the full band.  heimdall has no such stage: the definition is THIS project's own.  Off until
 * pb_search_set_subbands; a pb_search on which it was never called allocates nothing more, launches nothing more and
 * returns what it returns without it, byte for byte.  Not combined with pb_search_set_pol.
 * Notation: xt[c][t], delay[d][c], tout, the unzapped channels chans[] as under pb_search_set_cutouts; snr[d][t] the
 * full-band S/N planes on the device.
 *   1. Base sub-bands.  nsb of them, nsb in {2, 4, 8, 16}, nchan % nsb == 0.  Sub-band s is the unzapped channels with index
 *      in [s nchan/nsb, (s+1) nchan/nsb): the cutouts' convention, one run [first, last) of chans[]; it may be empty.
 *   2. Bands.  A band is a run of base sub-bands (first, count), count >= 1, first + count <= nsb.  This ABI takes an explicit
 *      list of nbands <= 64 of them, each with count < nsb (the whole band is the ordinary search and is refused).
 *      search.py's subband_list(nsb) makes the default, staggered dyadic, widest first: for c = nsb/2, nsb/4, .. 1 the bands
 *      (k max(c/2, 1), c), k = 0, 1, .. while they fit -- 2, 7, 18, 41 bands for nsb 2, 4, 8, 16.  The half-step stagger
 *      matters: a burst over the middle half of the band gains nothing from either aligned half.
 *   3. Sub-band series.  S[s][d][t] = sum over the channels c of sub-band s of xt[c][t + delay[d][c]], t in [0, tout): xt as
 *      the last search left it (cleaned in place if cleaning is on; the accumulated gulp when streaming), the main delay
 *      table, the last search's tout.  Exact u32; sum over s of S[s][d][t] == D[d][t], the search's own series.
 *   4. Band series.  B[b][d][t] = sum over the sub-bands s of band b of S[s][d][t].
 *   5. Band statistics.  Each band series gets its level, clipped rms, running baseline, S/N and log2-width plane by the
 *      text under pb_search_set_baseline, with the handle's baseline window and boxcars -- by the search's own kernels on
 *      the band rows, so a band's planes are bit for bit those of pb_search_run on a handle with everything outside the
 *      band zapped (and the same tout).  A band with no unzapped channel, or with rms not above 0, has S/N 0 everywhere.
 *   6. Best band per (d, t): the band with the largest S/N, compared in binary32; ties go to the smallest band index (-0
 *      equals +0); a NaN never wins (if every band's is a NaN the cell keeps band 0's).  Its S/N, log2 width and index are
 *      the cell's sub-band values.
 *   7. Points.  A cell is reported when t_lo <= t < t_hi, best S/N >= thresh, and best S/N > snr[d][t], all compared in
 *      binary32 (a NaN on either side reports nothing).  The last test keeps a broadband pulse from coming back once per
 *      band.  A point is PB_SUBPOINT_WORDS int32: dmi, t, S/N bits, log2 width, band index, full-band S/N bits.
 *   8. Point list.  Its order is unspecified (the host sorts it); *npoints is the exact count; when it exceeds the capacity
 *      (the smaller of max_points and max_out) the list is incomplete and *overflow = 1.
 *   9. DM chunks.  The trial DMs are processed dm_chunk rows at a time so that the stage's memory is bounded: dm_chunk = 0
 *      means the largest multiple of 4 that keeps the stage's buffers within 1 GiB, at least 4; any value is cut to ndm and
 *      to 65535 / nbands (the band rows of a pass are one grid dimension).  Results do not depend on dm_chunk.
 * Only exact integer sums and binary32 comparisons are new; tests/search_subband_ref.py restates them and
 * tests/test_gpu_search_subband.py holds the kernels to them exactly.
 * pb_search_set_subbands allocates the buffers; nbands = 0 frees them and switches the stage off.  PB_EINVAL with nothing
 * changed for a bad nsb, a bad band list, dm_chunk < 0, max_points outside 1..2^26, or polarisation being on. */
#define PB_SUBPOINT_WORDS 6
int pb_search_set_subbands(pb_search *s, int nsb, const int32_t *bands2, int nbands, int dm_chunk, int max_points);
/* On the block and planes of the last pb_search_run / pb_search_peaks / pb_search_gulp_*: points (host) receives
 * min(*npoints, max_out, max_points) points.  PB_EINVAL with a message (pb_search_last_error), nothing launched or written,
 * when the stage is off, no block has been searched, the planes were replaced by pb_search_set_planes (their tout is not the
 * last search's), the range is not 0 <= t_lo < t_hi <= tout, the threshold is a NaN, an output pointer is missing or
 * polarisation is on. */
int pb_search_subbands(pb_search *s, float thresh, int t_lo, int t_hi, int32_t *points, int max_out, int *npoints, int *overflow);
/* One trial DM of the current block recomputed through the same kernels, for tests and diagnostics.  Outputs (host, any may
 * be NULL): sub [nsb][tout] u32; band_snr [nbands][tout], band_wid [nbands][tout], band_stats [nbands][2]; best_snr,
 * best_wid, best_band [tout]. */
int pb_search_subband_dm(pb_search *s, int dmi, uint32_t *sub, float *band_snr, uint8_t *band_wid, float *band_stats,
                         float *best_snr, uint8_t *best_wid, uint8_t *best_band);
/* the last pb_search_subbands: device time in ms of the sub-band dedispersion, of the band sums, prefix sums and statistics,
 * of the boxcars and the best band (each added up over the chunks), and of everything with the copy to the host */
int pb_search_subband_timers(const pb_search *s, float *ms4);

/* Periodicity search: trains of pulses that are each below the single-pulse threshold.  Every trial DM's series of the
 * block that the last search left on the device is folded at every trial period by the fast folding algorithm (FFA) and
 * each folded profile is searched with circular boxcars.  The definition is THIS project's own; parity with no pulsar
 * package is claimed.  Off until pb_search_set_periodic; a pb_search on which it was never called allocates nothing more,
 * launches nothing more and returns what it returns without it, byte for byte.
 * Inputs: the series D[dm][0 .. tout) and rms = stats[dm][1] of the last pb_search_run / pb_search_peaks / pb_search_gulp_*.
 * Parameters: B = bins in {32, 64, 128} -- a profile has p bins, B <= p < 2B -- and the octaves k_lo <= k <= k_hi,
 * 0 <= k_lo <= k_hi <= 12.  For each (dm, k):
 *   1. Downsampling.  x_k[j] = sum over u < 2^k of D[dm][j 2^k + u], j in [0, n_k), n_k = floor(tout / 2^k).  Exact.
 *   For each base period p in [B, 2B):
 *   2. Rows.  m = floor(n_k / p).  If m < 2 the base period is skipped.  M is the smallest power of two >= m, L = log2 M.
 *      Row r of stage 0 is x_k[r p .. r p + p) for r < m and zeros for m <= r < M; the samples from m p on are not used.
 *   3. Folding.  At stage s + 1 block b has 2^(s+1) trials, made from block 2b (head H) and block 2b + 1 (tail T) of stage
 *      s: trial i uses h = i >> 1 and sh = (i + 1) >> 1, out[i][j] = H[h][j] + T[h][(j + sh) mod p].  After L stages there
 *      are M profiles F[i][0 .. p); trial i stands for the period (p + i / (M - 1)) 2^k tsamp seconds.  In closed form
 *      F[i][j] = sum over r < m of x_k[r p + ((j + s_L(r, i)) mod p)] with s_0 = 0, s_L(r, i) = s_{L-1}(r, i >> 1) for
 *      r < 2^(L-1) and ((i + 1) >> 1) + s_{L-1}(r - 2^(L-1), i >> 1) otherwise: every bin is the sum of exactly m samples
 *      of x_k.
 *   4. Range.  Profiles are uint32: pb_search_set_periodic fails unless 255 nact ceil(max_samples / B) < 2^32.  Window
 *      sums and the profile total are 64-bit.
 *   5. Matched filter.  Widths w = 2^q, q = 0 .. Q, 2^Q = B / 2 (so w <= p / 2).  T = sum over j of F[i][j] (the same for
 *      every i).  S(j, w) = sum over u < w of F[i][(j + u) mod p]: the window is circular.  Smax_q = max over j of
 *      S(j, 2^q), j_q the smallest j that reaches it.  The S/N of (i, q) is evaluated in double and rounded once to
 *      binary32: (double)(p Smax_q - w T), an exact integer, over (double)rms * sqrt((double)(m 2^k) * w * (p - w) * p).
 *      The profile's own mean is removed; the noise is the series' clipped rms scaled to a sum of m 2^k w samples, with
 *      the factor 1 - w / p for the mean that was removed.  Where rms is not above 0 the S/N is 0.
 *   6. Best.  A trial's S/N is the largest over q, of equal values the smaller q; a base period's best trial is the largest
 *      over i, of equal values the smaller i.  Comparisons are made in binary32.
 *   7. DM chunks.  The trial DMs are processed dm_chunk at a time so that the two scratch buffers of [dm_chunk][sum over p
 *      of M p] uint32 stay bounded (sum over p of M p < 2 n_k B): dm_chunk = 0 means what keeps them within 1 GiB, at least
 *      1; any value is cut to ndm and to 65535.  Results do not depend on dm_chunk.
 * Limits.  The series are not detrended: a slow baseline leaks into the longest periods.  There is no acceleration search
 * and no harmonic summing: the boxcars over the folded profile are the matched filter.
 * tests/search_periodic_ref.py restates all of it; tests/test_gpu_search_periodic.py holds the kernels to it (profiles and
 * window positions exactly, the S/N to 1 binary32 ulp).
 * pb_search_set_periodic allocates the buffers; bins = 0 frees them and switches the stage off.  PB_EINVAL with nothing
 * changed (pb_search_last_error says why) for bins not 0, 32, 64 or 128, a bad octave range, dm_chunk < 0 or the range
 * condition of 4. */
int pb_search_set_periodic(pb_search *s, int bins, int k_lo, int k_hi, int dm_chunk);
/* The best trial of every (dm, k, p) of the last block searched: best (host) is [ndm][k_hi - k_lo + 1][bins][4] int32 --
 * S/N bits, i, q, j_q -- the entry of p at index p - bins; a skipped base period has the bits of 0.0f, i = -1, q = j = 0.
 * PB_EINVAL with a message when the stage is off, no block has been searched or the pointer is missing. */
int pb_search_periodic(pb_search *s, int32_t *best);
/* One (dm, k, p) in full, for tests and for the profile of a candidate: *m and *M, and for M >= 2 prof [M][p] the folded
 * profiles, snr [M][Q + 1] and jbest [M][Q + 1] the S/N and j_q of every (i, q).  Any pointer may be NULL; with prof, snr
 * and jbest all NULL nothing is launched (the sizes only).  A skipped base period returns *m < 2, *M = 0 and writes nothing
 * else.  PB_EINVAL as above, and for dmi outside [0, ndm), k outside
 * [k_lo, k_hi] or p outside [bins, 2 bins). */
int pb_search_periodic_fold(pb_search *s, int dmi, int k, int p, uint32_t *prof, float *snr, int32_t *jbest, int *m, int *M);
/* the last pb_search_periodic: device time in ms of the folding (downsampling and stages, added up over the passes and
 * octaves), of the last stage with the evaluation, and of everything with the copy to the host */
int pb_search_periodic_timers(const pb_search *s, float *ms3);

/* Page-locked host memory for the blocks handed to pb_submit_vdif(_at) (H2D copies from pageable memory are
 * staged and synchronous); the reference allocates its 1-s host buffer the same way (cudaMallocHost,
 * src/process_baseband.cu:579).  A host program above this ABI needs no HIP headers.  NULL on failure. */
void *pb_host_alloc(size_t nbytes);
void pb_host_free(void *p);

const char *pb_version(void);

#ifdef __cplusplus
}
#endif
#endif
