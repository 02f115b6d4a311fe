"""NumPy restatement of the search's RFI cleaning (include/pb_hip.h, pb_search_set_rfi) for the tests.

narrow(): integers throughout plus the one binary32 comparison of the definition.  broad_flags(): the zero-DM boxcar
S/N in binary32 exactly as k_boxcar evaluates it, from a GIVEN level and rms -- the tests pass the GPU's own, the way
oracle.boxcar_best takes the kernel's own."""
import numpy as np

F32 = np.float32


def unpack(codes, nsamp, nchan, nbit):
    """SIGPROC codes (nbit per sample, low bits first within a byte) -> u8 [nsamp][nchan]"""
    b = np.asarray(codes, np.uint8).ravel()
    if nbit == 8:
        return b[:nsamp * nchan].reshape(nsamp, nchan)
    per = 8 // nbit
    sh = (nbit * np.arange(per)).astype(np.uint8)
    v = (b[:, None] >> sh[None, :]) & np.uint8((1 << nbit) - 1)
    return v.ravel()[:nsamp * nchan].reshape(nsamp, nchan)


def pack(x, nbit):
    """u8 [nsamp][nchan] of values < 2^nbit -> SIGPROC codes"""
    v = np.asarray(x, np.uint8).ravel()
    if nbit == 8:
        return v.copy()
    per = 8 // nbit
    v = v.reshape(-1, per).astype(np.uint16)
    out = np.zeros(v.shape[0], np.uint16)
    for i in range(per):
        out |= v[:, i] << (nbit * i)
    return out.astype(np.uint8)


def med_mad(row):
    """(med, mad) of one channel's codes: the smallest v / d whose cumulative count reaches ceil(n/2)"""
    row = np.asarray(row, np.uint8)
    need = (row.size + 1) // 2
    h = np.bincount(row, minlength=256).astype(np.int64)
    med = int(np.searchsorted(np.cumsum(h), need))
    g = np.zeros(256, np.int64)
    g[0] = h[med]
    for d in range(1, 256):
        g[d] = (h[med - d] if med - d >= 0 else 0) + (h[med + d] if med + d < 256 else 0)
    mad = int(np.searchsorted(np.cumsum(g), need))
    return med, mad


def narrow(xt, chans, tol, replace=True):
    """xt [nchan][nsamp] u8, chans: the unzapped channels -> (cleaned copy, number of flags, {c: med_c})"""
    out = np.array(xt, np.uint8, copy=True)
    n, meds = 0, {}
    for c in chans:
        med, mad = med_mad(out[c])
        meds[c] = med
        if not replace:
            continue
        thr = F32(tol) * F32(1.4826) * F32(max(mad, 1))            # left to right, binary32
        f = np.abs(out[c].astype(np.int32) - med).astype(F32) > thr
        out[c, f] = med
        n += int(f.sum())
    return out, n, meds


def zero_dm(xt, chans):
    """z[t]: exact sum over the unzapped channels"""
    return np.asarray(xt, np.uint64)[list(chans)].sum(axis=0)


def _baseline(P, t, W, n):
    lo = t - W // 2
    hi = lo + W
    lo, hi = np.where(lo < 0, 0, lo), np.where(lo < 0, min(W, n), hi)
    over = hi > n
    lo, hi = np.where(over, max(0, n - W), lo), np.where(over, n, hi)
    return ((P[hi] - P[lo]).astype(np.float64) / (hi - lo).astype(np.float64)).astype(F32)


def zero_dm_snr(z, level, rms, nbox, W):
    """best boxcar S/N and log2 width per start sample of the zero-DM series, k_boxcar's binary32 arithmetic"""
    z = np.asarray(z, np.uint64)
    n = z.size
    P = np.concatenate([[np.uint64(0)], np.cumsum(z, dtype=np.uint64)])
    level, rms = F32(level), F32(rms)
    best = np.full(n, F32(-1e30), F32)
    bw = np.zeros(n, np.int64)
    t = np.arange(n)
    for k in range(nbox):
        w = 1 << k
        ok = t + w <= n
        tt = t[ok]
        s = (P[tt + w] - P[tt]).astype(F32)
        base = _baseline(P, tt + w // 2, W, n) + level if W > 0 else np.full(tt.size, level, F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            sn = (s - F32(w) * base) / (rms * np.sqrt(F32(w)))
        upd = np.zeros(n, bool)
        upd[ok] = sn > best[ok]
        best[upd] = sn[upd[ok]]
        bw[upd] = k
    if not rms > 0:
        best[:] = 0
    return best, bw


def broad_flags(best, bw, tol):
    """flagged time samples: [t0, t0 + 2^bw[t0]) for every t0 with best[t0] >= tol"""
    n = best.size
    f = np.zeros(n, bool)
    for t0 in np.nonzero(best >= F32(tol))[0]:
        f[t0:min(n, t0 + (1 << int(bw[t0])))] = True
    return f


def apply_broad(xt, chans, meds, flags):
    out = np.array(xt, np.uint8, copy=True)
    for c in chans:
        out[c, flags] = meds[c]
    return out
