"""NumPy restatement of the sub-band search (include/pb_hip.h, pb_search_set_subbands) for the tests, written from the
definition's numbered rules: integer sums (rules 3, 4), the default band list (rule 2) and the binary32 comparisons that
pick the best band and the points (rules 6, 7).  The band statistics of rule 5 are tests/search_stats_ref.py's."""
import numpy as np

from search_cutout_ref import delays, zap_mask  # noqa: F401  (the delay table and the zap mask are the search's own)

F32 = np.float32


def band_list(nsb):
    """rule 2's default list: for c = nsb/2, nsb/4, .. 1 the bands (k max(c/2, 1), c) for k = 0, 1, .. while they fit"""
    assert nsb in (2, 4, 8, 16)
    out, c = [], nsb // 2
    while c >= 1:
        k = 0
        while k * max(c // 2, 1) + c <= nsb:
            out.append((k * max(c // 2, 1), c))
            k += 1
        c //= 2
    return out


def sub_series(xt, delay_d, zapped, nsb, tout):
    """rule 3 for one trial DM: S [nsb][tout] (int64) from xt [nchan][nsamp], the DM's delays [nchan] and the zap mask"""
    nchan = xt.shape[0]
    per = nchan // nsb
    S = np.zeros((nsb, tout), np.int64)
    for c in range(nchan):
        if not zapped[c]:
            d = int(delay_d[c])
            S[c // per] += xt[c, d:d + tout]
    return S


def band_series(S, bands):
    """rule 4: B [nbands][tout]"""
    return np.stack([S[f:f + n].sum(axis=0) for f, n in bands])


def best_band(band_snr, band_wid):
    """rule 6 on band planes [nbands][n] (binary32, u8): (best S/N f32, its log2 width, its band index), each [n].  Band 0
    unless a later band is larger (a tie, -0 against +0 too, keeps the smaller index) or the best so far is a NaN and the
    later one is not."""
    snr = np.asarray(band_snr, F32)
    best = snr[0].copy()
    bi = np.zeros(snr.shape[1], np.int64)
    for b in range(1, snr.shape[0]):
        v = snr[b]
        with np.errstate(invalid="ignore"):
            take = (v > best) | (np.isnan(best) & ~np.isnan(v))
        best = np.where(take, v, best)
        bi = np.where(take, b, bi)
    return best, np.asarray(band_wid)[bi, np.arange(snr.shape[1])], bi


def points(band_snr, band_wid, full_snr, thresh, t_lo, t_hi, dmi=0):
    """rule 7 for one trial DM: the set of (dmi, t, S/N bits, log2 width, band, full-band S/N bits)"""
    best, wid, bi = best_band(band_snr, band_wid)
    full = np.asarray(full_snr, F32)
    t = np.arange(best.size)
    with np.errstate(invalid="ignore"):
        hot = (t >= t_lo) & (t < t_hi) & (best >= F32(thresh)) & (best > full)
    return {(int(dmi), int(i), int(best[i:i + 1].view(np.int32)[0]), int(wid[i]), int(bi[i]), int(full[i:i + 1].view(np.int32)[0]))
            for i in np.nonzero(hot)[0]}
