// Periodicity search of the series that a run leaves on the device, by the fast folding algorithm (definition:
// include/pb_hip.h, pb_search_set_periodic / pb_search_periodic): k_ffa_down, k_ffa_stage, k_ffa_eval and their host side.
// One launch per folding stage; the last stage is folded inside k_ffa_eval, which never writes the final profiles.
#include "search_internal.h"

#include <algorithm>

// A pass's scratch row of one trial DM and one octave holds, for every base period p = B .. 2B - 1 that is not skipped, the
// M(p) rows of p bins of the current stage, p's rows from word off(p) on: tab[p - B] = (off, m, L, M), M = 2^L = 0 for a
// skipped base period.  Two such buffers are written in turn: stage s is in buffer s & 1.
#define FFA_TAB 4
#define FFA_ROWS 8                      // rows of one base period per workgroup of k_ffa_down / k_ffa_stage, two per wave
#define FFA_MAXP 256                    // 2B - 1 <= 255 bins
#define FFA_BUDGET (1ull << 30)         // dm_chunk = 0: the two scratch buffers stay within this

// Downsampling and stage 0: grid (tile of FFA_ROWS rows, p - B, row of the chunk).  x_k[j] = P[(j + 1) 2^k] - P[j 2^k] from
// the search's own prefix sums of the series (P[0] = 0, P[t + 1] = D[0] + .. + D[t], 64-bit, t < tout), which is the sum
// of the 2^k samples exactly.  Row r < m of p is x_k[r p .. r p + p), rows m .. M - 1 are zeros.
//   Reads.  r < m and j < p: (r p + j + 1) 2^k <= m p 2^k <= n_k 2^k <= tout, the last entry of a row of P.
//   Writes.  r < M, j < p: word off + r p + j < off + M p <= the row's length (the host's table).
__global__ __launch_bounds__(256) void k_ffa_down(const uint64_t *__restrict__ P, const int32_t *__restrict__ tab,
                                                  uint32_t *__restrict__ out, int B, int k, int dm0, size_t ppitch, size_t spitch)
{
    const int p = B + blockIdx.y;
    const int32_t *e = tab + FFA_TAB * blockIdx.y;
    const int off = e[0], m = e[1], M = e[3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t *pp = P + (size_t)(dm0 + blockIdx.z) * ppitch;
    uint32_t *o = out + (size_t)blockIdx.z * spitch + off;
    for (int u = 0; u < FFA_ROWS / 4; ++u) {
        const int r = blockIdx.x * FFA_ROWS + u * 4 + wave;
        if (r >= M) return;                                                // no barrier in this kernel
        for (int j = lane; j < p; j += 64) {
            uint32_t v = 0u;
            if (r < m) {
                const size_t t = (size_t)(r * p + j) << k;
                v = (uint32_t)(pp[t + ((size_t)1 << k)] - pp[t]);
            }
            o[r * p + j] = v;
        }
    }
}

// One folding stage, s -> s + 1: grid as k_ffa_down.  Output row ro of p is trial i = ro mod 2^(s+1) of block
// b = ro >> (s + 1); its head is row h = i >> 1 of block 2b of stage s = row (b << (s + 1)) + h of p, its tail the same
// row of block 2b + 1 = 2^s rows further on, read from bin (j + sh) mod p on, sh = (i + 1) >> 1.  A base period whose
// last stage this is or was (s + 1 >= L: k_ffa_eval folds stage L - 1 -> L itself) is left alone.
//   Reads and writes.  ro < M, so b 2^(s+1) + h + 2^s <= ro | 2^s < M: every row is one of p's M rows; bins < p.
__global__ __launch_bounds__(256) void k_ffa_stage(const uint32_t *__restrict__ in, const int32_t *__restrict__ tab,
                                                   uint32_t *__restrict__ out, int B, int s, size_t spitch)
{
    const int p = B + blockIdx.y;
    const int32_t *e = tab + FFA_TAB * blockIdx.y;
    const int off = e[0], L = e[2], M = e[3];
    if (s + 1 >= L) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t *x = in + (size_t)blockIdx.z * spitch + off;
    uint32_t *o = out + (size_t)blockIdx.z * spitch + off;
    for (int u = 0; u < FFA_ROWS / 4; ++u) {
        const int ro = blockIdx.x * FFA_ROWS + u * 4 + wave;
        if (ro >= M) return;
        const int i = ro & ((2 << s) - 1);
        const int rh = (ro - i) + (i >> 1), rt = rh + (1 << s);
        const int sh = ((i + 1) >> 1) % p;
        const uint32_t *H = x + rh * p, *T = x + rt * p;
        for (int j = lane; j < p; j += 64) {
            int jt = j + sh;
            if (jt >= p) jt -= p;
            o[ro * p + j] = H[j] + T[jt];
        }
    }
}

// the larger of two (sum, bin) pairs; of equal sums the smaller bin
__device__ __forceinline__ void ffa_take(uint64_t &v, int &j, uint64_t v2, int j2)
{
    if (v2 > v || (v2 == v && j2 < j)) {
        v = v2;
        j = j2;
    }
}

// The last stage and the evaluation: grid (base periods from p0 on, row of the chunk), one workgroup per (trial DM, p), its
// four waves take the final rows i = wave, wave + 4, ..  A wave folds its row from stage L - 1 (buffer (L - 1) & 1) into its
// own LDS row as 64-bit values, doubles the circular window sums in place between two LDS rows (S_2w(j) = S_w(j) +
// S_w((j + w) mod p)), takes each width's largest sum and its smallest bin by a wave reduction, and evaluates the S/N once
// per (i, q) in double.  Each wave keeps its best (S/N, i, q, j) in registers; the four are merged through LDS and the
// workgroup writes best[dm][k][p - B].  With oprof .. oj (pb_search_periodic_fold, grid (1, 1)) every row is also written.
//   Reads.  Row i of stage L has h = i >> 1 < M / 2 and the tail row M / 2 + h < M; bins < p.
//   The loop bound M is the same for every wave of the workgroup, so the barriers are met by all of them.
__global__ __launch_bounds__(256) void k_ffa_eval(const uint32_t *__restrict__ bufA, const uint32_t *__restrict__ bufB,
                                                  const int32_t *__restrict__ tab, const float *__restrict__ stats,
                                                  int32_t *__restrict__ best, int B, int Q, int k, int p0, int dm0, int nk,
                                                  int ki, size_t spitch, uint32_t *__restrict__ oprof,
                                                  float *__restrict__ osnr, int32_t *__restrict__ oj)
{
    __shared__ uint64_t win[4][2][FFA_MAXP];
    __shared__ int32_t wbest[4][4];
    const int p = p0 + blockIdx.x;
    const int32_t *e = tab + FFA_TAB * (p - B);
    const int off = e[0], m = e[1], L = e[2], M = e[3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int32_t *bo = best + (((size_t)(dm0 + blockIdx.y) * nk + ki) * B + (p - B)) * 4;
    if (M == 0) {                                                          // skipped: the whole workgroup leaves
        if (threadIdx.x == 0 && !oprof) {
            bo[0] = 0;
            bo[1] = -1;
            bo[2] = 0;
            bo[3] = 0;
        }
        return;
    }
    const uint32_t *x = (((L - 1) & 1) ? bufB : bufA) + (size_t)blockIdx.y * spitch + off;
    const float rms = stats[2 * (dm0 + blockIdx.y) + 1];
    const double len = (double)((int64_t)m << k);
    float bs = -1.f;                                                       // below every S/N: the first row is taken
    int bi = 0, bq = 0, bj = 0;
    for (int i0 = 0; i0 < M; i0 += 4) {
        const int i = i0 + wave;
        const bool live = i < M;
        uint64_t tot = 0;
        if (live) {
            const int h = i >> 1, sh = ((i + 1) >> 1) % p;
            const uint32_t *H = x + h * p, *T = x + ((M >> 1) + h) * p;
            for (int j = lane; j < p; j += 64) {
                int jt = j + sh;
                if (jt >= p) jt -= p;
                const uint32_t v = H[j] + T[jt];
                win[wave][0][j] = v;
                tot += v;
                if (oprof) oprof[i * p + j] = v;
            }
            for (int d = 32; d; d >>= 1) tot += __shfl_xor(tot, d);
        }
        __syncthreads();
        float rs = 0.f;
        int rq = 0, rj = 0;
        for (int q = 0; q <= Q; ++q) {
            const int w = 1 << q, cur = q & 1;
            if (live) {
                uint64_t vmax = 0;
                int jmax = 0x7fffffff;
                for (int j = lane; j < p; j += 64) ffa_take(vmax, jmax, win[wave][cur][j], j);
                for (int d = 32; d; d >>= 1) {
                    const uint64_t v2 = __shfl_xor(vmax, d);
                    const int j2 = __shfl_xor(jmax, d);
                    ffa_take(vmax, jmax, v2, j2);
                }
                float sn = 0.f;
                if (rms > 0.f) {
                    const double num = (double)((int64_t)p * (int64_t)vmax - (int64_t)w * (int64_t)tot);
                    const double den = (double)rms * sqrt(len * (double)w * (double)(p - w) * (double)p);
                    sn = (float)(num / den);
                }
                if (q == 0 || sn > rs) {
                    rs = sn;
                    rq = q;
                    rj = jmax;
                }
                if (osnr && lane == 0) {
                    osnr[i * (Q + 1) + q] = sn;
                    oj[i * (Q + 1) + q] = jmax;
                }
                if (q < Q) {
                    for (int j = lane; j < p; j += 64) {
                        int jw = j + w;
                        if (jw >= p) jw -= p;
                        win[wave][cur ^ 1][j] = win[wave][cur][j] + win[wave][cur][jw];
                    }
                }
            }
            __syncthreads();
        }
        if (live && rs > bs) {                                             // rows ascend: of equal S/N the smaller i stays
            bs = rs;
            bi = i;
            bq = rq;
            bj = rj;
        }
    }
    if (oprof) return;
    if (lane == 0) {
        wbest[wave][0] = __float_as_int(bs);
        wbest[wave][1] = bi;
        wbest[wave][2] = bq;
        wbest[wave][3] = bj;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int bw = 0;
        for (int v = 1; v < 4; ++v) {
            const float a = __int_as_float(wbest[v][0]), b = __int_as_float(wbest[bw][0]);
            if (a > b || (a == b && wbest[v][1] < wbest[bw][1])) bw = v;
        }
        for (int c = 0; c < 4; ++c) bo[c] = wbest[bw][c];
    }
}

void search_periodic_free(pb_search *s)
{
    search_release({s->per.d_buf[0], s->per.d_buf[1], s->per.d_tab, s->per.d_best, s->per.d_fprof, s->per.d_fsnr, s->per.d_fj},
                   nullptr, s->per.ev.data(), (int)s->per.ev.size());
    s->per = {};
}

// the smallest L with 2^L >= m
static int ffa_log2_up(int m)
{
    int L = 0;
    while ((1 << L) < m) ++L;
    return L;
}

// n_k of octave k for tout samples
static int ffa_nk(int tout, int k) { return tout >> k; }

extern "C" int pb_search_set_periodic(pb_search *s, int bins, int k_lo, int k_hi, int dm_chunk)
{
    const char *fn = "pb_search_set_periodic";
    if (!s) return search_fail(s, fn, "no search handle");
    if (bins != 0) {
        if (!(bins == 32 || bins == 64 || bins == 128)) return search_fail(s, fn, "bins must be 0 (off), 32, 64 or 128");
        if (k_lo < 0 || k_hi < k_lo || k_hi > 12) return search_fail(s, fn, "need octaves 0 <= k_lo <= k_hi <= 12");
        if (dm_chunk < 0) return search_fail(s, fn, "dm_chunk must be >= 0");
        const uint64_t rows = ((uint64_t)s->max_samples + bins - 1) / bins;
        if (255ull * (uint64_t)s->nact * rows >= (1ull << 32))
            return search_fail(s, fn, "a profile bin could exceed 32 bits: 255 nact ceil(max_samples / bins) must be < 2^32");
    }
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(s->stream));
    search_periodic_free(s);
    if (bins == 0) return PB_OK;
    // the longest scratch row: sum over p of M p < 2 n_k bins, n_k at its largest (the shortest octave, the longest block)
    const int nmax = ffa_nk(s->max_samples, k_lo), nk = k_hi - k_lo + 1;
    const size_t spitch = ((size_t)2 * nmax * bins + 63) & ~(size_t)63;
    int chunk = dm_chunk;
    if (chunk == 0) chunk = (int)std::max<size_t>(1, std::min<size_t>(FFA_BUDGET / (2 * spitch * sizeof(uint32_t)), 65535));
    chunk = std::min(std::min(chunk, 65535), s->ndm);               // the chunk's rows are one grid dimension
    const int nchunk = (s->ndm + chunk - 1) / chunk;
    const int Mmax = 1 << ffa_log2_up(std::max(nmax / bins, 1));
    int Q = 0;
    while ((2 << Q) <= bins / 2) ++Q;
    hipError_t e = hipSuccess;
    for (int b = 0; b < 2 && e == hipSuccess; ++b) e = hipMalloc((void **)&s->per.d_buf[b], (size_t)chunk * spitch * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->per.d_tab, (size_t)nk * bins * FFA_TAB * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->per.d_best, (size_t)s->ndm * nk * bins * 4 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->per.d_fprof, (size_t)Mmax * (2 * bins - 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&s->per.d_fsnr, (size_t)Mmax * (Q + 1) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&s->per.d_fj, (size_t)Mmax * (Q + 1) * sizeof(int32_t));
    s->per.ev.assign(2 * (size_t)nchunk * nk + 2, nullptr);         // per chunk and octave: start, folded; then kernels done, copy done
    for (size_t i = 0; i < s->per.ev.size() && e == hipSuccess; ++i) e = hipEventCreate(&s->per.ev[i]);
    if (e != hipSuccess) {
        search_periodic_free(s);
        s->err = std::string(fn) + ": " + hipGetErrorString(e);
        return PB_EHIP;
    }
    s->per.k_lo = k_lo;
    s->per.k_hi = k_hi;
    s->per.Q = Q;
    s->per.chunk = chunk;
    s->per.spitch = spitch;
    s->per.bins = bins;                     // (last: the stage is on only once everything exists)
    return PB_OK;
}

// The table of every octave for the last search's tout, on the device (made again only when tout has changed).  h_tab keeps
// it for the host: (off, m, L, M) per (octave, p - B).
static int ffa_table(pb_search *s)
{
    const int tout = s->last_tout, B = s->per.bins, nk = s->per.k_hi - s->per.k_lo + 1;
    if (s->per.tab_tout == tout) return PB_OK;
    s->per.h_tab.assign((size_t)nk * B * FFA_TAB, 0);
    for (int ki = 0; ki < nk; ++ki) {
        const int n = ffa_nk(tout, s->per.k_lo + ki);
        int off = 0;
        for (int p = B; p < 2 * B; ++p) {
            int32_t *e = &s->per.h_tab[((size_t)ki * B + (p - B)) * FFA_TAB];
            const int m = n / p;
            e[0] = off;
            e[1] = m;
            if (m >= 2) {
                e[2] = ffa_log2_up(m);
                e[3] = 1 << e[2];
                off += e[3] * p;
            }
        }
        if ((size_t)off > s->per.spitch) return search_fail(s, "pb_search_periodic", "internal: a scratch row is too short");
    }
    SCHK(s, hipMemcpy(s->per.d_tab, s->per.h_tab.data(), s->per.h_tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    s->per.tab_tout = tout;
    return PB_OK;
}

// Octave ki of the nrow trial DMs from dm0 on, up to the last stage but one: k_ffa_down, then k_ffa_stage for s = 0 ..
// Lmax - 2 (a base period with fewer stages sits out the later launches).  Returns nothing to evaluate (false) when every
// base period of the octave is skipped.
static bool ffa_fold(pb_search *s, int ki, int dm0, int nrow)
{
    const int B = s->per.bins, k = s->per.k_lo + ki;
    const int32_t *t = &s->per.h_tab[(size_t)ki * B * FFA_TAB];
    int Lmax = 0;
    for (int c = 0; c < B; ++c) Lmax = std::max(Lmax, t[c * FFA_TAB + 2]);
    if (Lmax == 0) return false;
    const int32_t *dt = s->per.d_tab + (size_t)ki * B * FFA_TAB;
    dim3 g(((1 << Lmax) + FFA_ROWS - 1) / FFA_ROWS, B, nrow);
    k_ffa_down<<<g, 256, 0, s->stream>>>(s->d_P, dt, s->per.d_buf[0], B, k, dm0, s->ppitch(), s->per.spitch);
    for (int st = 0; st + 1 < Lmax; ++st)
        k_ffa_stage<<<g, 256, 0, s->stream>>>(s->per.d_buf[st & 1], dt, s->per.d_buf[(st + 1) & 1], B, st, s->per.spitch);
    return true;
}

static int per_enter(pb_search *s, const char *fn)
{
    return search_enter(s, fn, s && s->per.bins, "the periodicity search is not switched on (pb_search_set_periodic)",
                        s && s->last_nsamp, "no block searched yet");
}

extern "C" int pb_search_periodic(pb_search *s, int32_t *best)
{
    const char *fn = "pb_search_periodic";
    if (int rc = per_enter(s, fn)) return rc;
    if (!best) return search_fail(s, fn, "the output pointer is missing");
    SCHK(s, hipSetDevice(s->device));
    if (int rc = ffa_table(s)) return rc;
    const int B = s->per.bins, nk = s->per.k_hi - s->per.k_lo + 1, chunk = s->per.chunk;
    hipEvent_t *ev = s->per.ev.data();
    int n = 0;
    for (int dm0 = 0; dm0 < s->ndm; dm0 += chunk) {
        const int nrow = std::min(chunk, s->ndm - dm0);
        for (int ki = 0; ki < nk; ++ki, ++n) {
            SCHK(s, hipEventRecord(ev[2 * n], s->stream));
            ffa_fold(s, ki, dm0, nrow);
            SCHK(s, hipEventRecord(ev[2 * n + 1], s->stream));
            // (an octave with every base period skipped still gets its entries written)
            k_ffa_eval<<<dim3(B, nrow), 256, 0, s->stream>>>(s->per.d_buf[0], s->per.d_buf[1], s->per.d_tab + (size_t)ki * B * FFA_TAB,
                                                             s->d_stats, s->per.d_best, B, s->per.Q, s->per.k_lo + ki, B, dm0, nk,
                                                             ki, s->per.spitch, nullptr, nullptr, nullptr);
        }
    }
    SCHK(s, hipEventRecord(ev[2 * n], s->stream));
    SCHK(s, hipGetLastError());
    SCHK(s, hipMemcpyAsync(best, s->per.d_best, (size_t)s->ndm * nk * B * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    SCHK(s, hipEventRecord(ev[2 * n + 1], s->stream));
    SCHK(s, hipEventSynchronize(ev[2 * n + 1]));
    s->per.ms[0] = s->per.ms[1] = 0.f;
    for (int c = 0; c < n; ++c) {
        s->per.ms[0] += search_ms(ev[2 * c], ev[2 * c + 1]);
        s->per.ms[1] += search_ms(ev[2 * c + 1], ev[2 * c + 2]);
    }
    s->per.ms[2] = search_ms(ev[0], ev[2 * n + 1]);
    return PB_OK;
}

extern "C" int pb_search_periodic_fold(pb_search *s, int dmi, int k, int p, uint32_t *prof, float *snr, int32_t *jbest, int *m,
                                       int *M)
{
    const char *fn = "pb_search_periodic_fold";
    if (int rc = per_enter(s, fn)) return rc;
    const int B = s->per.bins, Q = s->per.Q;
    if (dmi < 0 || dmi >= s->ndm) return search_fail(s, fn, "the DM index must be in [0, ndm)");
    if (k < s->per.k_lo || k > s->per.k_hi) return search_fail(s, fn, "the octave must be in [k_lo, k_hi]");
    if (p < B || p >= 2 * B) return search_fail(s, fn, "the base period must be in [bins, 2 bins)");
    SCHK(s, hipSetDevice(s->device));
    if (int rc = ffa_table(s)) return rc;
    const int ki = k - s->per.k_lo, nk = s->per.k_hi - s->per.k_lo + 1;
    const int32_t *e = &s->per.h_tab[((size_t)ki * B + (p - B)) * FFA_TAB];
    if (m) *m = e[1];
    if (M) *M = e[3];
    if (e[3] == 0) return PB_OK;                                    // skipped: nothing else is written
    if (!prof && !snr && !jbest) return PB_OK;                      // the sizes only: nothing to launch
    ffa_fold(s, ki, dmi, 1);
    k_ffa_eval<<<dim3(1, 1), 256, 0, s->stream>>>(s->per.d_buf[0], s->per.d_buf[1], s->per.d_tab + (size_t)ki * B * FFA_TAB, s->d_stats,
                                                  s->per.d_best, B, Q, k, p, dmi, nk, ki, s->per.spitch, s->per.d_fprof,
                                                  s->per.d_fsnr, s->per.d_fj);
    SCHK(s, hipGetLastError());
    SCHK(s, hipStreamSynchronize(s->stream));
    const size_t rows = e[3];
    if (prof) SCHK(s, hipMemcpy(prof, s->per.d_fprof, rows * p * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (snr) SCHK(s, hipMemcpy(snr, s->per.d_fsnr, rows * (Q + 1) * sizeof(float), hipMemcpyDeviceToHost));
    if (jbest) SCHK(s, hipMemcpy(jbest, s->per.d_fj, rows * (Q + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PB_OK;
}

extern "C" int pb_search_periodic_timers(const pb_search *s, float *ms3) { return search_get_ms(s, s ? s->per.ms : nullptr, 3, ms3); }
