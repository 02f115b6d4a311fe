"""Restatement of the search's normalisation (include/pb_hip.h, under pb_search_set_baseline) for the tests: the
per-series level and rms, the running baseline and the boxcar S/N planes.

Written from the header's text.  It is meant to be MORE accurate than the kernels, not a copy of their reduction order:
  * the residuals v(t) = x[t] - b(t) are differences of an integer and a binary32 value, so 2^E v(t) is an integer for
    a suitable E; every sum of v and v^2 and the clip's membership test are evaluated on those integers with Python's
    unbounded ints -- exactly;
  * the S/N planes are evaluated in float64 from exact integer boxcar sums, and come with a bound on what the binary32
    evaluation of the definition may differ by, derived from np.spacing of its operands (no fitted constant).
tests/search_rfi_ref.py keeps its binary32 emulation of the S/N for the flag set of the broad pass;
tests/test_search_stats_cpu.py ties the two together."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
U = 2.0 ** -53                 # unit roundoff of binary64
CLIP = 3                       # the second pass keeps |v - m1| <= CLIP r1
KEPT = 0.97330                 # variance a Gaussian keeps when clipped at 3 sigma


def prefix(x):
    """P[0] = 0, P[t + 1] = P[t] + x[t]: exact integers (int64; a series sums to < 2^40)"""
    x = np.asarray(x)
    assert x.ndim == 1 and np.issubdtype(x.dtype, np.integer)
    return np.concatenate([[0], np.cumsum(x.astype(np.int64), dtype=np.int64)])


def window(t, W, n):
    """[lo, hi) of the baseline under sample t (arrays allowed), W > 0"""
    t = np.asarray(t, np.int64)
    lo = t - W // 2
    hi = lo + W
    before = lo < 0                                     # starts before the series: [0, min(W, n))
    lo = np.where(before, 0, lo)
    hi = np.where(before, min(W, n), hi)
    after = hi > n                                      # ends after it: [max(0, n - W), n)
    lo = np.where(after, max(0, n - W), lo)
    hi = np.where(after, n, hi)
    return lo, hi


def baseline(P, t, W, n):
    """b(t), binary32: the double quotient of the window's integer sum and its length, rounded.  W = 0: g = P[n] / n."""
    P = np.asarray(P, np.int64)
    if W <= 0:
        return np.full(np.shape(t), F32(float(P[n]) / float(n)), F32)
    lo, hi = window(t, W, n)
    return ((P[hi] - P[lo]).astype(np.float64) / (hi - lo).astype(np.float64)).astype(F32)


def _scaled_residuals(x, b):
    """(V, E): Python ints V[t] = 2^E (x[t] - b[t]) exactly.  A binary32 b is m 2^e with an integer m < 2^24, so
    E = 24 - (the smallest exponent frexp gives) makes every 2^E b an integer."""
    b64 = np.asarray(b, np.float64)
    nz = b64 != 0
    E = 0
    if nz.any():
        E = max(0, 24 - int(np.frexp(b64[nz])[1].min()))
    B = np.ldexp(b64, E)                               # exact: a power-of-two scaling
    assert np.all(B == np.floor(B))
    Bi = np.array([int(v) for v in B], object)
    V = np.array([int(v) << E for v in x], object) - Bi
    return V, E


def series_stats(x, W):
    """(level, rms, n_boundary) of one series: level and rms as binary32 (stats[dm][0..1] of the definition), and the
    number of samples so close to the clip's edge that an evaluation in double could put them on the other side.

    Exact: with V = 2^E v, S1 = sum V, S2 = sum V^2 (integers), m1 = S1 / (n 2^E) and var1 = (n S2 - S1^2) / (n 2^E)^2, so
    |v - m1| <= 3 r1  <=>  (n V - S1)^2 <= 9 (n S2 - S1^2): an integer comparison.

    n_boundary: a double evaluation forms fabs(v - m1) <= 3 r1 with m1 and r1 from sums of n terms.  A sum of n terms
    added in any order with at most d = ceil(n / 256) + 10 additions on the path of one term (256 lanes, each its
    stride, then a tree) is off by at most d U sum|term|, so
        |dm1| <= d U mean|v|,   |dvar1| <= (d + 2) U mean(v^2) + 2 |m1| |dm1| + 2 U m1^2,   |dr1| <= |dvar1| / (2 r1) + U r1,
    and the compared expression |v - m1| - 3 r1 is off by at most |dm1| + 3 |dr1| + 2 U (|v| + |m1| + 3 r1).  Samples
    within that of the edge are counted.  Where r1 is exactly 0 every v equals m1, `<=` keeps them all whatever the
    rounding, and n_boundary is 0 by definition."""
    x = np.asarray(x)
    n = x.size
    P = prefix(x)
    b = baseline(P, np.arange(n), W, n)
    V, E = _scaled_residuals(x, b)
    S1, S2 = int(V.sum()), int((V * V).sum())
    num1 = n * S2 - S1 * S1                             # var1 (n 2^E)^2, >= 0
    assert num1 >= 0
    dev = V * n - S1
    keep = np.array(dev * dev <= CLIP * CLIP * num1, bool)
    cn = int(keep.sum())
    assert cn > 0                                       # (at least 8/9 of any series lie within 3 rms)
    Vk = V[keep]
    C1, C2 = int(Vk.sum()), int((Vk * Vk).sum())
    num2 = cn * C2 - C1 * C1
    assert num2 >= 0
    scale = 1 << E
    var2 = float(Fraction(num2, (cn * scale) ** 2))
    rms = math.sqrt(var2 / KEPT)
    m2 = Fraction(C1, cn * scale)
    level = float(m2) if W > 0 else float(m2 + Fraction(float(b[0])))
    # samples a double evaluation could put on the other side of the clip
    n_boundary = 0
    if num1 > 0:
        v = np.array([float(Fraction(int(q), scale)) for q in V])
        m1 = float(Fraction(S1, n * scale))
        r1 = math.sqrt(float(Fraction(num1, (n * scale) ** 2)))
        d = -(-n // 256) + 10
        dm1 = d * U * float(np.mean(np.abs(v)))
        dvar = (d + 2) * U * float(np.mean(v * v)) + 2 * abs(m1) * dm1 + 2 * U * m1 * m1
        dr1 = dvar / (2 * r1) + U * r1
        tol = dm1 + CLIP * dr1 + 2 * U * (np.abs(v) + abs(m1) + CLIP * r1)
        n_boundary = int(np.sum(np.abs(np.abs(v - m1) - CLIP * r1) <= tol))
    return F32(level), F32(rms), n_boundary


def level_tolerance(x, W, level):
    """what stats[dm][0] may differ from series_stats' level by: 1 binary32 ulp of the level plus the summation bound
    n 2^-52 mean|v| of the double sums (for W > 0 the level is near zero and its own ulp means nothing)"""
    x = np.asarray(x)
    n = x.size
    v = x.astype(np.float64) - baseline(prefix(x), np.arange(n), W, n).astype(np.float64)
    return float(np.spacing(F32(abs(level)))) + n * 2.0 ** -52 * float(np.mean(np.abs(v)))


def _sp32(a):
    """binary32 spacing at |a| (float64 array in, float64 out)"""
    return np.spacing(np.abs(a).astype(F32)).astype(np.float64)


def boxcar_all(x, level, rms, nbox, W, dlevel=0.0, drms=0.0):
    """Every width's S/N in float64 and its bound: (sn [nbox][n], err [nbox][n]); NaN where t + w > n.  level, rms: the
    binary32 statistics.  With rms not positive sn holds the numerators (P[t+w] - P[t]) - w base and err their bounds.
    dlevel, drms: what the level and rms that the evaluation under test used may differ from the given ones by; their
    first-order effect, w dlevel / (rms sqrt(w)) + |S/N| drms / rms, is added to the bound (w dlevel to a numerator's).

    err: the binary32 evaluation rounds the integer sum (half a spacing of the sum), forms base = b + level (half a
    spacing of base, times w; w base itself is exact, w being a power of two), rounds the difference (half a spacing of
    the difference, taken at its magnitude plus the two errors before it, so that a difference carried into the next
    binade is covered); these are divided by rms sqrt(w).  The divisor rms sqrtf(w) carries two roundings (2^-24
    relative each) and the quotient one more (half a spacing of the S/N)."""
    x = np.asarray(x)
    n = x.size
    P = prefix(x)
    level64, rms64 = float(F32(level)), float(F32(rms))
    sn = np.full((nbox, n), np.nan)
    err = np.full((nbox, n), np.nan)
    for k in range(nbox):
        w = 1 << k
        if w > n:
            break
        t = np.arange(n - w + 1)
        S = (P[t + w] - P[t]).astype(np.float64)                        # exact: < 2^53
        if W > 0:
            base = baseline(P, t + w // 2, W, n).astype(np.float64) + level64
        else:
            base = np.full(t.size, level64)
        num = S - w * base
        e_num = 0.5 * _sp32(S) + 0.5 * w * _sp32(base)
        e_num = e_num + 0.5 * _sp32(np.abs(num) + e_num)
        if rms64 > 0:
            q = num / (rms64 * math.sqrt(w))
            sn[k, :t.size] = q
            err[k, :t.size] = (e_num / (rms64 * math.sqrt(w)) + np.abs(q) * 2.0 ** -23 + 0.5 * _sp32(np.abs(q) * (1 + 2.0 ** -22))
                               + math.sqrt(w) * dlevel / rms64 + np.abs(q) * drms / rms64)
        else:
            sn[k, :t.size] = num
            err[k, :t.size] = e_num + w * dlevel
    return sn, err


def boxcar_planes(x, level, rms, nbox, W):
    """(best [n] float64, bw [n] log2 width, err_bound [n]): the planes of the definition from a given binary32 level
    and rms.  Ties go to the narrower width.  rms not positive: best = 0, bw = the narrowest width whose numerator is
    positive (0 if none), err_bound = the bound of that numerator (of the width-1 numerator if none)."""
    sn, err = boxcar_all(x, level, rms, nbox, W)
    n = sn.shape[1]
    if not float(F32(rms)) > 0:
        pos = np.nan_to_num(sn, nan=-1.0) > 0
        bw = np.where(pos.any(axis=0), pos.argmax(axis=0), 0)
        return np.zeros(n), bw, err[bw, np.arange(n)]
    s = np.where(np.isnan(sn), -np.inf, sn)
    bw = s.argmax(axis=0)                                               # argmax returns the first (narrowest) maximum
    return s[bw, np.arange(n)], bw, err[bw, np.arange(n)]


def compare_planes(got_snr, got_bw, sn, err):
    """An evaluation's planes against boxcar_all's (rms > 0).  A width k is `allowed` at t when its S/N plus its bound
    reaches the best S/N minus its bound: where only the best is allowed the width must be that one, elsewhere (a
    near-tie) one of the allowed; the S/N must lie within the bound of the float64 S/N at the width that was chosen.
    -> dict(tie [n] bool, width_ok [n] bool, value_ok [n] bool, excess [n] = |difference| - bound)"""
    n = sn.shape[1]
    ar = np.arange(n)
    s = np.where(np.isnan(sn), -np.inf, sn)
    e = np.where(np.isnan(err), 0.0, err)
    bw = s.argmax(axis=0)
    allowed = s + e >= (s[bw, ar] - e[bw, ar])[None, :]
    got_bw = np.asarray(got_bw, np.int64)
    assert got_bw.max() < sn.shape[0]
    excess = np.abs(np.asarray(got_snr, np.float64) - s[got_bw, ar]) - e[got_bw, ar]
    return dict(tie=allowed.sum(axis=0) > 1, width_ok=allowed[got_bw, ar], value_ok=excess <= 0, excess=excess, bw=bw)
