"""NumPy restatement of the search's refinement (include/pb_hip.h under pb_search_set_refine): the reference's
refine_dm and optimize_pulse (analysis/loc_step0.py) with tophat_smooth and qn (analysis/utils.py), on exact integer
series, the S/N in float64 as the header writes them.  tests/test_search_refine_cpu.py holds it to what the reference's
own functions returned (tests/golden/reference_refine.npz); tests/test_gpu_search_refine.py holds the kernels to it."""
import numpy as np

QN_CONST = 2.2219


def odd(width):
    """an even width becomes width + 1 (tophat_smooth)"""
    return int(width) | 1


def window(t_pk, H, T):
    return max(0, t_pk - H), min(T, t_pk + H)


def smooth(q, w):
    """tophat_smooth of the whole integer series q at odd width w: sum over [t - h, t + h] / (2 h + 1),
    h = min(w // 2, t, T - 1 - t) -> (float64 values, the integer sums, the counts 2 h + 1)"""
    q = np.asarray(q, np.int64)
    T = q.size
    t = np.arange(T)
    h = np.minimum(w // 2, np.minimum(t, T - 1 - t))
    c = np.concatenate([[0], np.cumsum(q)])
    s = c[t + h + 1] - c[t - h]
    return s.astype(np.float64) / (2 * h + 1).astype(np.float64), s, 2 * h + 1


def med2(x):
    """twice the median of integers: an exact integer"""
    s = np.sort(np.asarray(x, np.int64))
    n = s.size
    return int(s[(n - 1) // 2] + s[n // 2])


def qn_quarters(x):
    """four times the 25th percentile of the N (N - 1) / 2 absolute pair differences with np.percentile's linear
    interpolation: position (Np - 1) / 4 = r + f / 4 -> 4 d[r] + f (d[r + 1] - d[r]), an exact integer"""
    x = np.asarray(x, np.int64)
    iu = np.triu_indices(x.size, k=1)
    d = np.sort(np.abs(x[iu[0]] - x[iu[1]]))
    r, f = divmod(d.size - 1, 4)
    return int(4 * d[r] + (f * (d[r + 1] - d[r]) if f else 0))


def qn(x):
    return QN_CONST * (qn_quarters(x) / 4.0)


def sn_bound(sn, mean, num, std):
    """How far two float64 evaluations of (mean - med) / std [* sqrt(w)] from the same exact integers may differ, from the
    rounding of the operands (every operation correctly rounded, relative error 2^-53 <= spacing(x) / |x|):
      * the mean (a quotient of integers, or the reference's product with a rounded 1 / n: two roundings) is off by at most
        1 + 2 spacings of itself over the two evaluations; the subtraction of the exact median adds one spacing of the
        difference each -> (3 spacing(mean) + 2 spacing(num)) / std on the S/N;
      * std (2.2219 x quarters, sqrt(w), their quotient or product), the final quotient and the product with sqrt(w): at
        most five relative roundings per evaluation -> 10 spacing(sn)."""
    sn, mean, num = np.abs(np.asarray(sn, np.float64)), np.abs(np.asarray(mean, np.float64)), np.abs(np.asarray(num, np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (3 * np.spacing(mean) + 2 * np.spacing(num)) / std + 10 * np.spacing(sn)


def dm_pass(q, valid, t_pk, width, H):
    """q: [nstep][T] exact integer series of the fine trials, valid: [nstep] bool -> dict(sn_dm, kbest, err, mx, med, qn)"""
    q = np.asarray(q, np.int64)
    nstep, T = q.shape
    w = odd(width)
    i0, i1 = window(t_pk, H, T)
    sn = np.full(nstep, np.nan)
    err = np.full(nstep, np.nan)
    mx, med, sig = np.full(nstep, np.nan), np.full(nstep, np.nan), np.full(nstep, np.nan)
    for k in range(nstep):
        if not valid[k]:
            continue
        med[k] = med2(q[k, i0:i1]) / 2.0
        sig[k] = qn(q[k, i0:i1])
        mx[k] = smooth(q[k], w)[0][i0:i1].max()
        if sig[k] > 0:
            std = sig[k] / np.sqrt(float(w))
            sn[k] = (mx[k] - med[k]) / std
            err[k] = sn_bound(sn[k], mx[k], mx[k] - med[k], std)
        else:
            sn[k], err[k] = 0.0, 0.0
    kbest = int(np.nanargmax(sn)) if np.any(valid) else -1
    return dict(sn_dm=sn, kbest=kbest, err=err, mx=mx, med=med, qn=sig)


def width_pass(q, t_pk, H, wmax):
    """q: [T] one exact integer series -> dict(widths, opt_sn, opt_loc, err, med, qn, tie): tie[iw] is True where the
    largest running sum is not unique over the positions (the first one is reported either way)"""
    q = np.asarray(q, np.int64)
    T = q.size
    i0, i1 = window(t_pk, H, T)
    n = i1 - i0
    off = np.append(q[i0:i0 + int(n * 0.25)], q[i0 + int(n * 0.75):i1])
    med, sig = med2(off) / 2.0, qn(off)
    widths = np.arange(1, wmax, 2)
    c = np.concatenate([[0], np.cumsum(q)])
    sns, locs, err = np.zeros(widths.size), np.zeros(widths.size, np.int64), np.zeros(widths.size)
    for iw, w in enumerate(widths):
        t = np.arange(i0 + w, i1 - w)
        s = c[t + w // 2 + 1] - c[t - w // 2]
        a = int(np.argmax(s))
        locs[iw] = a + w
        mean = float(s[a]) / float(w)
        if sig > 0:
            sns[iw] = (mean - med) / sig * np.sqrt(float(w))
            err[iw] = sn_bound(sns[iw], mean, mean - med, sig / np.sqrt(float(w)))
    return dict(widths=widths, opt_sn=sns, opt_loc=locs, err=err, med=med, qn=sig)


def refine(q, valid, t_pk, width, H, wmax):
    """one request -> dict(status, sn_dm, kbest, opt_sn, opt_loc, err_dm, err_opt, near_tie): near_tie is True where the
    two largest sn_dm of DIFFERENT value lie within their bounds of each other (kbest is then not pinned)"""
    q = np.asarray(q, np.int64)
    nstep, T = q.shape
    nw = wmax // 2
    i0, i1 = window(t_pk, H, T)
    if i1 - i0 < 4 * wmax:
        return dict(status=1, sn_dm=np.full(nstep, np.nan), kbest=-1, opt_sn=np.full(nw, np.nan),
                    opt_loc=np.full(nw, -1, np.int64), err_dm=np.zeros(nstep), err_opt=np.zeros(nw), near_tie=False)
    d = dm_pass(q, valid, t_pk, width, H)
    if d["kbest"] < 0:
        return dict(status=0, sn_dm=d["sn_dm"], kbest=-1, opt_sn=np.full(nw, np.nan), opt_loc=np.full(nw, -1, np.int64),
                    err_dm=d["err"], err_opt=np.zeros(nw), near_tie=False)
    kb = d["kbest"]
    other = np.array([k for k in range(nstep) if valid[k] and d["sn_dm"][k] != d["sn_dm"][kb]], int)
    near = bool(other.size and np.any(d["sn_dm"][kb] - d["sn_dm"][other] <= d["err"][kb] + d["err"][other]))
    wp = width_pass(q[kb], t_pk, H, wmax)
    return dict(status=0, sn_dm=d["sn_dm"], kbest=kb, opt_sn=wp["opt_sn"], opt_loc=wp["opt_loc"], err_dm=d["err"],
                err_opt=wp["err"], near_tie=near, dm=d, wp=wp)


def trial_dms(dm_lo, dm_step, nstep):
    """the fine trials' DMs as the interface makes them from two binary32 numbers"""
    return float(np.float32(dm_lo)) + np.arange(nstep) * float(np.float32(dm_step))


def fine_series(xt, chans, delays, tout, lo=0, hi=None):
    """xt: [nchan][nsamp] u8 block as the search saw it; delays: [nstep][nchan] -> [nstep][tout] exact sums over `chans`
    (only the samples [lo, hi) are formed, the others left 0: a refinement reads a window and its margins)"""
    lo, hi = max(0, lo), tout if hi is None else min(tout, hi)
    q = np.zeros((delays.shape[0], tout), np.int64)
    for k in range(delays.shape[0]):
        for c in chans:
            q[k, lo:hi] += xt[c, delays[k, c] + lo:delays[k, c] + hi]
    return q


def series_window(q, t_pk, H, M):
    """the ABI's `series` of one request: q over [t_pk - H - M, t_pk + H + M), 0 outside [0, T)"""
    nstep, T = q.shape
    out = np.zeros((nstep, 2 * (H + M)), np.int64)
    t = t_pk - H - M + np.arange(2 * (H + M))
    ok = (t >= 0) & (t < T)
    out[:, ok] = q[:, t[ok]]
    return out
