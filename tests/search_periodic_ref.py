"""NumPy restatement of the periodicity search (include/pb_hip.h, pb_search_set_periodic) for the tests, written from the
definition and not from the kernels: the downsampling, the fast-folding stage recursion AND the closed form with s_L (the
tests hold the two equal), the circular matched filter and the tie rules.  Everything up to the S/N is exact integer
arithmetic (Python ints / uint64); the S/N is one float64 division rounded once to binary32."""
import numpy as np


def downsample(series, k):
    """x_k[j] = sum of series[j 2^k .. (j + 1) 2^k), j < floor(len / 2^k); uint64"""
    x = np.asarray(series, np.uint64)
    n = x.size >> k
    return x[:n << k].reshape(n, 1 << k).sum(axis=1, dtype=np.uint64)


def rows_of(n, p):
    """(m, M, L) of a base period p over n samples; M = L = 0 where the base period is skipped (m < 2)"""
    m = n // p
    if m < 2:
        return m, 0, 0
    L = int(m - 1).bit_length()
    return m, 1 << L, L


def fold_stages(x, p):
    """the M profiles [M][p] of base period p by the stage recursion; None where it is skipped"""
    m, M, L = rows_of(len(x), p)
    if M == 0:
        return None
    cur = np.zeros((M, p), np.uint64)
    cur[:m] = np.asarray(x[:m * p], np.uint64).reshape(m, p)
    j = np.arange(p)
    for s in range(L):
        size = 2 << s                                   # trials per block of stage s + 1
        out = np.empty_like(cur)
        for b in range(M // size):
            H = cur[(2 * b) * (size // 2):(2 * b + 1) * (size // 2)]
            T = cur[(2 * b + 1) * (size // 2):(2 * b + 2) * (size // 2)]
            for i in range(size):
                h, sh = i >> 1, (i + 1) >> 1
                out[b * size + i] = H[h] + T[h][(j + sh) % p]
        cur = out
    return cur


def shift(L, r, i):
    """s_L(r, i): how far row r is rotated in trial i after L stages"""
    if L == 0:
        return 0
    half = 1 << (L - 1)
    if r < half:
        return shift(L - 1, r, i >> 1)
    return ((i + 1) >> 1) + shift(L - 1, r - half, i >> 1)


def fold_closed(x, p):
    """the same profiles by the closed form F[i][j] = sum over r < m of x[r p + (j + s_L(r, i)) mod p]"""
    m, M, L = rows_of(len(x), p)
    if M == 0:
        return None
    x = np.asarray(x, np.uint64)
    j = np.arange(p)
    F = np.zeros((M, p), np.uint64)
    for i in range(M):
        for r in range(m):
            F[i] += x[r * p + (j + shift(L, r, i)) % p]
    return F


def widths(B):
    """the matched filter's widths 2^0 .. 2^Q = B / 2"""
    return [1 << q for q in range(int(B // 2).bit_length())]


def snr_value(p, smax, w, total, m, k, rms):
    """the S/N of one (trial, width): evaluated in float64, rounded once to binary32; 0 where rms is not above 0"""
    if not float(rms) > 0:
        return np.float32(0)
    num = float(int(p) * int(smax) - int(w) * int(total))           # an exact integer below 2^53
    den = float(np.float64(np.float32(rms))) * np.sqrt(np.float64(float((int(m) << int(k)) * int(w) * (int(p) - int(w)) * int(p))))
    return np.float32(np.float64(num) / den)


def evaluate(F, B, m, k, rms):
    """(snr [M][Q + 1] f32, jbest [M][Q + 1] i32) of the profiles F [M][p]: circular windows, first bin of the largest sum"""
    M, p = F.shape
    ws = widths(B)
    snr = np.zeros((M, len(ws)), np.float32)
    jb = np.zeros((M, len(ws)), np.int32)
    F = np.asarray(F, np.uint64)
    total = F.sum(axis=1, dtype=np.uint64)
    for q, w in enumerate(ws):
        S = np.zeros_like(F)
        for u in range(w):                              # S[i][j] = sum over u < w of F[i][(j + u) mod p], term by term
            S += np.roll(F, -u, axis=1)
        jb[:, q] = np.argmax(S, axis=1)                 # (the first of equal values)
        for i in range(M):
            snr[i, q] = snr_value(p, S[i, jb[i, q]], w, total[i], m, k, rms)
    return snr, jb


def best_of(snr, jbest):
    """the tie rules on a base period's per-trial S/N [M][Q + 1]: (S/N, i, q, j) -- a trial's S/N the largest over q, of
    equal values the smaller q; the best trial the largest over i, of equal values the smaller i"""
    q = np.argmax(snr, axis=1)                          # (argmax returns the first of equal values)
    per = snr[np.arange(snr.shape[0]), q]
    i = int(np.argmax(per))
    return np.float32(per[i]), i, int(q[i]), int(jbest[i, q[i]])


def search_series(series, rms, B, k_lo, k_hi):
    """the best table of one series: dict(snr f32, i, q, j i32 -- [nk][B] --, m, M i32 [nk][B]); a skipped base period has
    S/N 0 and i = -1"""
    nk = k_hi - k_lo + 1
    out = dict(snr=np.zeros((nk, B), np.float32), i=np.full((nk, B), -1, np.int32), q=np.zeros((nk, B), np.int32),
               j=np.zeros((nk, B), np.int32), m=np.zeros((nk, B), np.int32), M=np.zeros((nk, B), np.int32))
    for ki in range(nk):
        x = downsample(series, k_lo + ki)
        for p in range(B, 2 * B):
            m, M, _ = rows_of(len(x), p)
            out["m"][ki, p - B], out["M"][ki, p - B] = m, M
            if M == 0:
                continue
            snr, jb = evaluate(fold_stages(x, p), B, m, k_lo + ki, rms)
            out["snr"][ki, p - B], out["i"][ki, p - B], out["q"][ki, p - B], out["j"][ki, p - B] = best_of(snr, jb)
    return out


def period_samples(p, i, M):
    """the period that trial i of base period p stands for, in samples of its octave"""
    return p + i / (M - 1.0)
