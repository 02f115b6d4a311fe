"""NumPy restatement of the search's per-candidate cutouts (include/pb_hip.h, pb_search_set_cutouts) for the tests:
written from the definition, a loop over channels and DM rows with slices, integers throughout."""
import numpy as np


def delays(dms, fch1, foff, nchan, tsamp):
    """[ndm][nchan] integer delays as pb_search_create documents them: the formula in double from the binary32-rounded
    band and sample time, floor(x + 0.5); the top of the band is the reference"""
    fch1, foff, tsamp = float(np.float32(fch1)), float(np.float32(foff)), float(np.float32(tsamp))
    f = fch1 + np.arange(nchan) * foff
    ftop = fch1 if foff < 0 else fch1 + (nchan - 1) * foff
    out = np.empty((len(dms), nchan), np.int64)
    for i, dm in enumerate(dms):
        out[i] = np.floor(4.148808e3 * float(dm) * (1.0 / (f * f) - 1.0 / (ftop * ftop)) / tsamp + 0.5).astype(np.int64)
    return out


def zap_mask(nchan, zap):
    m = np.zeros(nchan, bool)
    for lo, hi in zap:
        m[lo:hi] = True
    return m


def cutout(xt, delay, zapped, series, nsub, nt, ndmrow, dmi, t_pk, tscr):
    """xt [nchan][nsamp] u8 (the block as the search saw it), delay [ndm][nchan], zapped [nchan] bool, series
    [ndm][tout] -> (ft, ft_hits [nsub][nt], dt, dt_hits [ndmrow][nt]) as int64.  Bin j covers the block samples
    t_pk + (j - nt/2) tscr ... + tscr."""
    nchan, nsamp = xt.shape
    ndm, tout = series.shape
    per = nchan // nsub
    t = t_pk - (nt // 2) * tscr + np.arange(nt * tscr, dtype=np.int64)         # every sample of every bin, bin-major
    ft = np.zeros((nsub, nt), np.int64)
    fth = np.zeros((nsub, nt), np.int64)
    for c in range(nchan):
        if zapped[c]:
            continue
        src = t + int(delay[dmi, c])
        ok = (src >= 0) & (src < nsamp)
        v = np.zeros(t.size, np.int64)
        v[ok] = xt[c, src[ok]]
        ft[c // per] += v.reshape(nt, tscr).sum(axis=1)
        fth[c // per] += ok.reshape(nt, tscr).sum(axis=1)
    dt = np.zeros((ndmrow, nt), np.int64)
    dth = np.zeros((ndmrow, nt), np.int64)
    ok = (t >= 0) & (t < tout)
    for k in range(ndmrow):
        dm = dmi - ndmrow // 2 + k
        if dm < 0 or dm >= ndm:
            continue
        v = np.zeros(t.size, np.int64)
        v[ok] = series[dm, t[ok]]
        dt[k] = v.reshape(nt, tscr).sum(axis=1)
        dth[k] = ok.reshape(nt, tscr).sum(axis=1)
    return ft, fth, dt, dth


def cutouts(xt, delay, zapped, series, nsub, nt, ndmrow, reqs):
    """the same for a list of (dmi, t_pk, tscr): dict of stacked arrays, keys as Searcher.cutouts"""
    r = [cutout(xt, delay, zapped, series, nsub, nt, ndmrow, *q) for q in reqs]
    return {k: np.stack([x[i] for x in r]) for i, k in enumerate(("ft", "ft_hits", "dt", "dt_hits"))}


def series_of(xt, delay, zapped, max_delay):
    """the dedispersed series [ndm][nsamp - max_delay] of a block, by the search's definition"""
    nchan, nsamp = xt.shape
    tout = nsamp - max_delay
    out = np.zeros((delay.shape[0], tout), np.int64)
    for i in range(delay.shape[0]):
        for c in range(nchan):
            if not zapped[c]:
                out[i] += xt[c, delay[i, c]:delay[i, c] + tout]
    return out
