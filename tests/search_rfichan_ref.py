"""NumPy restatement of the cleaning's channel stage (include/pb_hip.h, pb_search_set_rfi_chan) for the tests: Python
ints or int64 throughout, and the one binary64 comparison written as the header writes it."""
import numpy as np


def lags(radius):
    """the signed lags of a radius: +l, -l for l = 1, max(l * 3 // 2, l + 1), .. while l <= radius"""
    out, l = [], 1
    while l <= radius:
        out += [l, -l]
        l = max(l * 3 // 2, l + 1)
    return out


def moments(rows):
    """rows [nact][nsamp] u8 -> (sum, S, fill) as int64 arrays; S = nsamp sq - sum^2, fill the rounded mean"""
    x = np.asarray(rows, np.uint8).astype(np.int64)
    n = x.shape[1]
    s = x.sum(axis=1)
    sq = (x * x).sum(axis=1)
    assert 65025 * n * n < 1 << 63
    return s, n * sq - s * s, (2 * s + n) // (2 * n)


def outliers(S, L, tol):
    """(outlier flags [nact] of the signed lag L, j [nact])"""
    S = np.asarray(S, np.int64)
    nact = S.size
    j = np.clip(np.arange(nact) - L, 0, nact - 1)
    d = S - S[j]
    ds = np.sort(d)
    q1, med, q3 = int(ds[(nact - 1) // 4]), int(ds[(nact - 1) // 2]), int(ds[3 * (nact - 1) // 4])
    thr = float(np.float32(tol)) * (float(q3 - q1) / 1.349)        # one quotient, one product, binary64
    out = np.array([float(int(v) - med) > thr for v in d], bool)   # int -> binary64: one rounding, as the cast's
    return out, j


def votes(S, radius, tol):
    """(recv, cast, flag) over the lags of `radius` (0: max(1, nact // 10))"""
    S = np.asarray(S, np.int64)
    nact = S.size
    recv, cast = np.zeros(nact, np.int64), np.zeros(nact, np.int64)
    acc = []
    for L in lags(radius if radius > 0 else max(1, nact // 10)):
        o, j = outliers(S, L, tol)
        a = np.nonzero(o)[0]
        recv[a] += 1
        np.add.at(cast, j[a], 1)
        acc.append((a, j[a]))
    flag = np.zeros(nact, bool)
    for a, ja in acc:
        flag[a[cast[ja] <= recv[a]]] = True
    return recv, cast, flag


def stage(xt, chans, nsamp, radius, tol):
    """xt [nchan][>= nsamp] u8, chans: the unzapped channels ascending -> dict(xt: the filled copy, nflag, and mask, sum,
    stat, recv, cast, fill as [nchan] arrays in file numbering, 0 for zapped channels)"""
    xt = np.asarray(xt, np.uint8)
    chans = np.asarray(chans, np.int64)
    nchan = xt.shape[0]
    s, S, fill = moments(xt[chans, :nsamp])
    recv, cast, flag = votes(S, radius, tol)
    out = np.array(xt, np.uint8, copy=True)
    for a in np.nonzero(flag)[0]:
        out[chans[a], :nsamp] = fill[a]

    def full(v, dt):
        r = np.zeros(nchan, dt)
        r[chans] = v
        return r

    return dict(xt=out, nflag=int(flag.sum()), mask=full(flag, np.uint8), sum=full(s, np.int64), stat=full(S, np.int64),
                recv=full(recv, np.int32), cast=full(cast, np.int32), fill=full(fill, np.uint8))
