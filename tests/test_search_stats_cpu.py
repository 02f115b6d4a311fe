"""The restatement of the search's normalisation (tests/search_stats_ref.py) held to something independent of it, so
that a misreading of include/pb_hip.h cannot sit in the reference and in the kernel alike: the baseline against a brute
force mean of an explicit slice, the statistics on series whose answers are known, the float64 planes against the
binary32 emulation of tests/search_rfi_ref.py inside the derived bound, and that bound at the production scale (sums
above 2^24).  No GPU."""
import math

import numpy as np
import pytest

import search_rfi_ref as R
import search_stats_ref as S

F32 = np.float32


@pytest.mark.parametrize("tout", [64, 71, 300])
def test_baseline_is_the_mean_of_the_clamped_window(tout):
    rng = np.random.default_rng(900 + tout)
    x = rng.integers(0, 65000, tout)
    P = S.prefix(x)
    assert P[0] == 0 and P.size == tout + 1 and all(int(P[t + 1]) == int(x[:t + 1].sum()) for t in range(tout))
    for W in (1, 2, 3, 64, 777, tout - 1, tout, tout + 5):
        got = S.baseline(P, np.arange(tout), W, tout)
        assert got.dtype == F32
        for t in range(tout):
            lo = t - W // 2                              # the window as the header words it, sample by sample
            hi = lo + W
            if lo < 0:
                lo, hi = 0, min(W, tout)
            if hi > tout:
                lo, hi = max(0, tout - W), tout
            assert 0 <= lo < hi <= tout and hi - lo == min(W, tout)
            assert got[t] == F32(x[lo:hi].mean(dtype=np.float64)), (W, t)
        # both restatements agree (search_rfi_ref's is the one the broad pass's flag set is checked with)
        assert np.array_equal(got, R._baseline(P.astype(np.uint64), np.arange(tout), W, tout))
    g = S.baseline(P, np.arange(tout), 0, tout)
    assert np.all(g == F32(x.sum() / tout))


def test_statistics_of_series_with_known_answers():
    # constant: level the constant, rms 0, no boundary sample, whatever the window
    for W in (0, 1, 7, 5000):
        lvl, rms, nb = S.series_stats(np.full(300, 977), W)
        assert (float(lvl), float(rms), nb) == (977.0 if W == 0 else 0.0, 0.0, 0)
    # W = 1: the baseline is the sample itself
    rng = np.random.default_rng(11)
    lvl, rms, nb = S.series_stats(rng.integers(0, 60000, 3001), 1)
    assert (float(lvl), float(rms), nb) == (0.0, 0.0, 0)
    # two levels, half and half: nothing is clipped (|v - m| = d/2 = r1 < 3 r1), mean a + d/2, var d^2/4
    x = np.where(np.arange(1000) % 2 == 0, 1000, 1060)
    lvl, rms, nb = S.series_stats(x, 0)
    assert float(lvl) == 1030.0 and rms == F32(math.sqrt(900.0 / 0.97330)) and nb == 0
    # one huge outlier among the two levels: the second pass drops it and the answer is the same
    y = x.copy()
    y[123] = 1000000
    lvl2, rms2, nb = S.series_stats(y, 0)
    mean_rest = (x.sum() - x[123]) / 999.0
    var_rest = (np.delete(x, 123).astype(np.float64) ** 2).mean() - mean_rest ** 2
    assert abs(float(lvl2) - mean_rest) <= np.spacing(F32(mean_rest)) and nb == 0
    assert abs(float(rms2) - math.sqrt(var_rest / 0.97330)) <= np.spacing(F32(rms2))
    assert float(rms2) < 40 < y.std()                     # (with it: 31 600)
    # all zero but one sample: what the clip leaves is constant -> rms exactly 0, level exactly 0
    z = np.zeros(3000, np.int64)
    z[1500] = 255
    lvl, rms, nb = S.series_stats(z, 0)
    assert float(rms) == 0.0 and abs(float(lvl)) <= 1e-9 and nb == 0


def test_rms_of_clipped_gaussian_samples_lands_on_sigma():
    """What the 0.97330 is for.  n Gaussian samples of sigma 50 (rounded to integers: + 1/12 of variance, 3e-5
    relative): the rms estimate of n samples scatters by sigma / sqrt(2 n) (the clipped estimator's fourth moment is a
    little below the Gaussian's, so this overstates it slightly); the band is 5 of those.  n is chosen so that the band,
    0.56 %, is well inside the 1.34 % by which the uncorrected clipped rms (sqrt(0.9733) = 0.98656) falls short."""
    n, sigma = 400000, 50.0
    rng = np.random.default_rng(2024)
    x = np.rint(100000 + sigma * rng.standard_normal(n)).astype(np.int64)
    lvl, rms, nb = S.series_stats(x, 0)
    band = 5.0 / math.sqrt(2 * n)
    true = math.sqrt(sigma * sigma + 1.0 / 12)
    assert band < 0.006 and nb == 0
    assert abs(float(rms) / true - 1) < band
    assert abs(float(rms) * math.sqrt(0.97330) / true - 1) > band        # the uncorrected value does not
    assert abs(float(lvl) - 100000) < 5 * sigma / math.sqrt(n)


def _noise_series(seed, n, nchan, drift=0.0):
    """a dedispersed-series look-alike: the sum of nchan 8-bit codes of mean 127.5, sigma 33.8"""
    rng = np.random.default_rng(seed)
    x = nchan * 127.5 + math.sqrt(nchan) * 33.8 * rng.standard_normal(n) + drift * nchan * np.sin(np.arange(n) / 600.0)
    return np.rint(x).astype(np.int64)


@pytest.mark.parametrize("n,nchan,W,nbox", [(71, 64, 0, 5), (300, 256, 0, 7), (2056, 256, 512, 7), (3000, 64, 777, 5),
                                            (3000, 256, 2560, 7), (2048, 512, 1, 3), (257, 64, 266, 7)])
def test_float64_planes_against_the_binary32_emulation(n, nchan, W, nbox):
    x = _noise_series(n + W, n, nchan, drift=3.0)
    x[n // 2:n // 2 + 6] += int(6 * math.sqrt(nchan) * 33.8)            # something to find
    lvl, rms, _ = S.series_stats(x, W)
    if W == 1:
        lvl, rms = F32(0.25), F32(math.sqrt(nchan) * 33.8)                # (rms 0 of W = 1 is test_rms_zero's)
    best32, bw32 = R.zero_dm_snr(x, lvl, rms, nbox, W)
    sn, err = S.boxcar_all(x, lvl, rms, nbox, W)
    c = S.compare_planes(best32, bw32, sn, err)
    assert c["value_ok"].all(), float(c["excess"].max())
    assert c["width_ok"].all()
    assert np.array_equal(bw32[~c["tie"]], c["bw"][~c["tie"]]) and c["tie"].mean() <= 1e-3
    best, bw, eb = S.boxcar_planes(x, lvl, rms, nbox, W)
    assert np.array_equal(bw, c["bw"]) and np.all(np.abs(best32[~c["tie"]] - best[~c["tie"]]) <= eb[~c["tie"]])
    # the bound is a bound, not slack: it is of the order of the binary32 spacing of the operands
    assert float(np.nanmax(err)) < 64 * float(np.spacing(F32(x.max()))) / float(rms) + 1e-4


def test_rms_zero_planes():
    """rms not positive: S/N 0 everywhere; the width is the narrowest whose numerator is positive, else 0"""
    best, bw, _ = S.boxcar_planes(np.full(100, 500), F32(500), F32(0), 4, 0)
    assert not best.any() and not bw.any()
    x = np.array([5, 5, 9, 5, 5, 5, 5, 5] * 8)
    best, bw, _ = S.boxcar_planes(x, F32(0), F32(0), 3, 1)               # W = 1: base = x[t + w/2]
    b32, w32 = R.zero_dm_snr(x, F32(0), F32(0), 3, 1)
    assert not best.any() and not b32.any() and np.array_equal(bw, w32)
    # t = 0: 0, 10 - 2*5, 24 - 4*9: none positive; t = 1: 0, 14 - 2*9, 24 - 4*5 > 0; t = 2: 0, 14 - 2*5 > 0
    assert (bw[0], bw[1], bw[2]) == (0, 2, 1)


def test_bound_at_the_production_scale():
    """3850 unzapped 8-bit channels, a 30 720-sample gulp, W = 2560, widths to 64: a 64-sample sum is 3.1e7 > 2^24, so
    the binary32 evaluation rounds both terms before they cancel.  The emulation stays inside the derived bound, and
    the bound stays small against an S/N of order 1."""
    n, nchan, W, nbox = 30720, 3850, 2560, 7
    x = _noise_series(5, n, nchan, drift=0.05)
    x[9000:9004] += int(10 * math.sqrt(nchan) * 33.8 / 2)
    lvl, rms, nb = S.series_stats(x, W)
    assert nb == 0 and x[:64].sum() > 2 ** 24
    best32, bw32 = R.zero_dm_snr(x, lvl, rms, nbox, W)
    sn, err = S.boxcar_all(x, lvl, rms, nbox, W)
    c = S.compare_planes(best32, bw32, sn, err)
    print("worst emulated error / bound at width 64: %.3g / %.3g; near-ties %d of %d" % (
        float(np.nanmax(np.abs(R.F32(0) + best32[bw32 == 6] - sn[6][bw32 == 6]))) if (bw32 == 6).any() else 0.0,
        float(np.nanmax(err[6])), int(c["tie"].sum()), n))
    assert c["value_ok"].all(), float(c["excess"].max())
    assert c["width_ok"].all() and np.array_equal(bw32[~c["tie"]], c["bw"][~c["tie"]])
    assert c["tie"].mean() <= 1e-3
    assert float(np.nanmax(err)) < 1e-3
