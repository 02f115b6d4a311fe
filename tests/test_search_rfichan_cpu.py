"""The cleaning's channel stage without a GPU: the NumPy restatement (tests/search_rfichan_ref.py) against answers worked
out by hand, the refusals of pb_search_set_rfi_chan that need no handle, and the CLI flags."""
import ctypes as C
import importlib

import numpy as np
import pytest

import search_rfichan_ref as R
from helpers import libpb

search = importlib.import_module("vlite-fast_amd.search")
EINVAL = -22          # PB_EINVAL


def test_lag_lists():
    assert R.lags(1) == [1, -1]
    assert R.lags(2) == [1, -1, 2, -2]
    assert R.lags(10) == [1, -1, 2, -2, 3, -3, 4, -4, 6, -6, 9, -9]
    pos = [1, 2, 3, 4, 6, 9, 13, 19, 28, 42, 63, 94, 141, 211, 316]
    assert R.lags(385) == [v for l in pos for v in (l, -l)]         # the 30 signed lags of 3850 channels
    assert R.lags(0) == []


def test_moments_by_hand():
    """[0, 255]: sum 255, sq 65025, S = 2 x 65025 - 255^2 = 65025, fill = (510 + 2) // 4 = 128; [7, 7, 7]: S = 0, fill 7;
    [1, 2]: sum 3, sq 5, S = 10 - 9 = 1, fill = (6 + 2) // 4 = 2 (a mean of 1.5 rounds up)"""
    s, S, f = R.moments(np.array([[0, 255]], np.uint8))
    assert (int(s[0]), int(S[0]), int(f[0])) == (255, 65025, 128)
    s, S, f = R.moments(np.array([[7, 7, 7]], np.uint8))
    assert (int(s[0]), int(S[0]), int(f[0])) == (21, 0, 7)
    s, S, f = R.moments(np.array([[1, 2]], np.uint8))
    assert (int(s[0]), int(S[0]), int(f[0])) == (3, 1, 2)


def test_one_channel_flags_nothing():
    recv, cast, flag = R.votes([12345], 0, 4.0)                      # radius 0 -> max(1, 1 // 10) = 1: lags +1, -1; d = 0
    assert recv.tolist() == [0] and cast.tolist() == [0] and not flag.any()


def test_one_loud_channel_among_eight():
    """S = 10 everywhere but S[3] = 1000, radius 2 (lags +1, -1, +2, -2), tol 4.
    L = +1: j(a) = max(a - 1, 0); d = [0, 0, 0, 990, -990, 0, 0, 0]; sorted [-990, 0, 0, 0, 0, 0, 0, 990]; the ranks 7 // 4 = 1,
            7 // 2 = 3, 21 // 4 = 5 give q1 = med = q3 = 0, the threshold is 4 x 0 / 1.349 = 0, and d - med > 0 holds for
            a = 3 alone: recv[3] = 1, cast[2] = 1.
    L = -1: j(a) = min(a + 1, 7); d = [0, 0, -990, 990, 0, 0, 0, 0]: again a = 3 alone: recv[3] = 2, cast[4] = 1.
    L = +2: d[3] = 990, d[5] = -990: recv[3] = 3, cast[1] = 1.    L = -2: d[1] = -990, d[3] = 990: recv[3] = 4, cast[5] = 1.
    Every accuser has cast 1 <= recv[3] = 4: channel 3 is flagged, nobody else."""
    S = [10, 10, 10, 1000, 10, 10, 10, 10]
    o, j = R.outliers(S, 1, 4.0)
    assert o.tolist() == [a == 3 for a in range(8)] and j.tolist() == [0, 0, 1, 2, 3, 4, 5, 6]
    o, j = R.outliers(S, -1, 4.0)
    assert o.tolist() == [a == 3 for a in range(8)] and j.tolist() == [1, 2, 3, 4, 5, 6, 7, 7]
    recv, cast, flag = R.votes(S, 2, 4.0)
    assert recv.tolist() == [0, 0, 0, 4, 0, 0, 0, 0]
    assert cast.tolist() == [0, 1, 1, 0, 1, 1, 0, 0]
    assert flag.tolist() == [a == 3 for a in range(8)]


def test_one_quiet_channel_convicts_nobody():
    """S = 1000 everywhere but S[3] = 10, radius 1.  L = +1: d[3] = -990, d[4] = 990: a = 4 is the outlier, accused by
    j(4) = 3.  L = -1: d[2] = 990, d[3] = -990: a = 2, accused by j(2) = 3.  The quiet channel has cast one vote per signed
    lag, cast[3] = 2; each neighbour has received one; 2 <= 1 is false twice, nobody is flagged."""
    recv, cast, flag = R.votes([1000, 1000, 1000, 10, 1000, 1000, 1000, 1000], 1, 4.0)
    assert recv.tolist() == [0, 0, 1, 0, 1, 0, 0, 0]
    assert cast.tolist() == [0, 0, 0, 2, 0, 0, 0, 0]
    assert not flag.any()


def test_constant_channels_flag_nothing():
    x = np.full((12, 40), 9, np.uint8)
    r = R.stage(x, np.arange(12), 40, 0, 3.0)                        # S = 0, q3 - q1 = 0, 0 > 0 is false
    assert r["nflag"] == 0 and not r["mask"].any() and not r["stat"].any() and np.array_equal(r["xt"], x)
    assert r["fill"].tolist() == [9] * 12 and not r["recv"].any() and not r["cast"].any()


def test_stage_fills_the_flagged_rows_up_to_nsamp_only():
    rng = np.random.default_rng(3)
    x = rng.integers(120, 136, (40, 300)).astype(np.uint8)
    x[17] = rng.integers(0, 256, 300)
    x[5] = 0                                                         # zapped: not in the list, whatever it holds
    chans = np.array([c for c in range(40) if c != 5])
    r = R.stage(x, chans, 256, 0, 4.0)
    assert np.nonzero(r["mask"])[0].tolist() == [17] and r["nflag"] == 1
    assert (r["xt"][17, :256] == r["fill"][17]).all() and np.array_equal(r["xt"][17, 256:], x[17, 256:])
    keep = np.arange(40) != 17
    assert np.array_equal(r["xt"][keep], x[keep]) and r["stat"][5] == 0 and r["sum"][5] == 0


def test_set_rfi_chan_refuses_bad_arguments():
    L = libpb().load()

    def err():
        return L.pb_search_last_error(None).decode()

    for tol in (-1.0, float("nan"), float("inf")):
        assert L.pb_search_set_rfi_chan(None, 0, tol) == EINVAL and "tol" in err(), tol
    assert L.pb_search_set_rfi_chan(None, -1, 4.0) == EINVAL and "radius" in err()
    for radius, tol in ((0, 4.0), (5, 3.0), (0, 0.0)):
        assert L.pb_search_set_rfi_chan(None, radius, tol) == EINVAL and "no search handle" in err()
    n = C.c_int()
    assert L.pb_search_rfi_chan_info(None, C.byref(n), None, None, None, None, None, None, None) == EINVAL


def test_cli_flags():
    plain = search.parse_args(["-f", "x.fil"])
    assert vars(plain) == vars(search.arg_parser().parse_args(["-f", "x.fil"])) | dict(cutout_thresh=6.0, refine_thresh=6.0)
    assert not any(k.startswith("rfi_chan") for k in vars(plain))    # the namespace it gives today
    a = search.parse_args(["-f", "x.fil", "-rfi_chan"])
    assert (a.rfi_chan, a.rfi_chan_tol, a.rfi_chan_radius) == (True, 4.0, 0)
    a = search.parse_args(["-f", "x.fil", "-rfi_chan", "-rfi_chan_tol", "3.5", "-rfi_chan_radius", "40", "-rfi_clean"])
    assert (a.rfi_chan, a.rfi_chan_tol, a.rfi_chan_radius, a.rfi_clean) == (True, 3.5, 40, True)
    b = search.parse_args(["-f", "x.fil", "-rfi_clean"])
    assert {k: v for k, v in vars(a).items() if not k.startswith("rfi_chan")} == vars(b)
    for alone in (["-rfi_chan_tol", "5"], ["-rfi_chan_radius", "3"]):
        with pytest.raises(SystemExit):
            search.parse_args(["-f", "x.fil"] + alone)
    for bad in (["-rfi_chan_tol", "0"], ["-rfi_chan_tol", "-2"], ["-rfi_chan_tol", "nan"], ["-rfi_chan_radius", "-1"]):
        with pytest.raises(SystemExit):
            search.parse_args(["-f", "x.fil", "-rfi_chan"] + bad)
    f = search.parse_flags("-rfi_chan -rfi_chan_tol 5")
    assert (f.rfi_chan, f.rfi_chan_tol, f.rfi_chan_radius) == (True, 5.0, 0) and not hasattr(f, "fil")
    assert vars(search.parse_flags("-dm 2 100")) == {k: v for k, v in vars(search.parse_flags("-dm 2 100 -rfi_chan")).items()
                                                     if not k.startswith("rfi_chan")}
