"""The search's per-candidate cutouts without a GPU: the ABI's declarations and exports, argument refusals that need no
device, the new kernels' compiled resources, the NumPy restatement (tests/search_cutout_ref.py) against numbers worked
out by hand, and the CLI flags and the .cutouts.npz file."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import search_cutout_ref as R
from helpers import ROOT, libpb
from test_kernel_resources import _usage

search = importlib.import_module("vlite-fast_amd.search")
EINVAL = -22          # PB_EINVAL
NAMES = ("pb_search_set_cutouts", "pb_search_cutouts")


def test_header_declares_and_library_exports_the_cutout_functions():
    hdr = open(os.path.join(ROOT, "include", "pb_hip.h")).read()
    assert re.search(r"\bint\s+pb_search_set_cutouts\(pb_search \*s, int nsub, int nt, int ndmrow, int max_cands\);", hdr)
    assert re.search(r"\bint\s+pb_search_cutouts\(pb_search \*s, const int32_t \*cands3, int n, uint32_t \*ft, "
                     r"uint32_t \*ft_hits, uint32_t \*dt,\s+uint32_t \*dt_hits\);", hdr)
    lp = libpb()
    L = lp.load()
    for n in NAMES:
        assert n in lp.EXPORTS
        assert getattr(L, n).restype is C.c_int and getattr(L, n).argtypes


def test_refusals_that_need_no_device():
    L = libpb().load()
    assert L.pb_search_set_cutouts(None, 64, 256, 64, 32) == EINVAL
    assert "no search handle" in L.pb_search_last_error(None).decode()
    req = (C.c_int32 * 3)(0, 0, 1)
    assert L.pb_search_cutouts(None, req, 1, None, None, None, None) == EINVAL
    assert "no search handle" in L.pb_search_last_error(None).decode()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_cutout_kernels_use_no_scratch():
    u = _usage("search_cutout.hip")
    for name in ("k_cutout_ft", "k_cutout_dt"):
        k = next(v for sym, v in u.items() if name in sym)
        assert k["ScratchSize"] == 0 and k["Occupancy"] >= 4, (name, k)
    # every kernel of the search stays scratch-free: the other three translation units as well
    for src in ("search_run.hip", "search_refine.hip", "search_giants.hip"):
        u.update(_usage(src))
    assert len(u) == 20 and all(v["ScratchSize"] == 0 for v in u.values()), u


# the hand-made block: 4 channels x 40 samples, xt[c][t] = 40 c + t; two trial DMs with delays 0,0,0,0 and 0,1,2,4:
# max_delay 4, tout 36; two subbands of two channels, four time bins, two DM rows
XT = (40 * np.arange(4)[:, None] + np.arange(40)[None, :]).astype(np.uint8)
DELAY = np.array([[0, 0, 0, 0], [0, 1, 2, 4]])
NOZAP = np.zeros(4, bool)
SERIES = R.series_of(XT, DELAY, NOZAP, 4)


def test_restatement_by_hand_in_the_middle_of_the_block():
    assert SERIES.shape == (2, 36) and SERIES[0, 6] == 240 + 4 * 6 and SERIES[1, 0] == 0 + 41 + 82 + 124
    # (dmi 1, t_pk 10, tscr 2): bins [6,8) [8,10) [10,12) [12,14)
    ft, fth, dt, dth = R.cutout(XT, DELAY, NOZAP, SERIES, 2, 4, 2, 1, 10, 2)
    # subband 0, bin 0: xt[0][6] + xt[0][7] + xt[1][7] + xt[1][8] = 6 + 7 + 47 + 48; each later bin adds 2 to all four terms
    assert ft[0].tolist() == [108, 116, 124, 132]
    # subband 1, bin 0: xt[2][8] + xt[2][9] + xt[3][10] + xt[3][11] = 88 + 89 + 130 + 131
    assert ft[1].tolist() == [438, 446, 454, 462]
    assert fth.tolist() == [[4, 4, 4, 4], [4, 4, 4, 4]]
    # DM rows: k = 0 is DM index 0 (D[0][t] = 240 + 4 t: 264 + 268 in bin 0), k = 1 the candidate's own
    assert dt[0].tolist() == [532, 548, 564, 580] and dt[1].tolist() == [546, 562, 578, 594]
    assert dth.tolist() == [[2, 2, 2, 2], [2, 2, 2, 2]]
    # the identities: band-summed ft is the centre row of dt, hits are nact tscr
    assert np.array_equal(ft.sum(axis=0), dt[1]) and np.all(fth.sum(axis=0) == 4 * 2)
    # tscr 1: dt is a crop of the series
    ft, fth, dt, dth = R.cutout(XT, DELAY, NOZAP, SERIES, 2, 4, 2, 1, 10, 1)
    assert np.array_equal(dt, SERIES[:, 8:12]) and np.all(dth == 1) and np.array_equal(ft.sum(axis=0), dt[1])


def test_restatement_clips_at_both_edges_of_the_block():
    # t_pk 0: bins [-4,-2) [-2,0) [0,2) [2,4).  Channel 0 (delay 0) has bins 2, 3; channel 1 (delay 1) also sample 0 of
    # bin 1; channel 2 (delay 2) bins 1-3; channel 3 (delay 4) all four
    ft, fth, dt, dth = R.cutout(XT, DELAY, NOZAP, SERIES, 2, 4, 2, 1, 0, 2)
    assert fth.tolist() == [[0, 1, 4, 4], [2, 4, 4, 4]]
    assert ft[0, 1] == 40 and ft[1, 0] == 120 + 121          # xt[1][0]; xt[3][0] + xt[3][1]
    assert dth.tolist() == [[0, 0, 2, 2], [0, 0, 2, 2]] and dt[:, :2].tolist() == [[0, 0], [0, 0]]
    assert dt[1, 2] == SERIES[1, 0] + SERIES[1, 1]
    # t_pk 35 = tout - 1: bins [31,33) [33,35) [35,37) [37,39); nsamp 40.  Channel 2 (delay 2) loses sample 40 of bin 3;
    # channel 3 (delay 4) reads 39, (40) in bin 2 and nothing in bin 3
    ft, fth, dt, dth = R.cutout(XT, DELAY, NOZAP, SERIES, 2, 4, 2, 1, 35, 2)
    assert fth.tolist() == [[4, 4, 4, 4], [4, 4, 3, 1]]
    assert ft[1, 3] == 80 + 39 and ft[1, 2] == (80 + 37) + (80 + 38) + (120 + 39)
    assert dth.tolist() == [[2, 2, 1, 0], [2, 2, 1, 0]] and dt[1, 2] == SERIES[1, 35] and dt[1, 3] == 0
    # the identities hold in the bins that lie inside [0, tout)
    assert np.array_equal(ft.sum(axis=0)[:2], dt[1, :2]) and np.all(fth.sum(axis=0)[:2] == 8)


def test_restatement_zapped_subband_and_rows_off_the_grid():
    zap = np.array([False, False, True, True])
    ser = R.series_of(XT, DELAY, zap, 1)                       # the largest delay of an unzapped channel is 1
    ft, fth, dt, dth = R.cutout(XT, DELAY, zap, ser, 2, 4, 2, 1, 10, 2)
    assert fth.tolist() == [[4, 4, 4, 4], [0, 0, 0, 0]] and ft[1].tolist() == [0, 0, 0, 0]
    assert ft[0].tolist() == [108, 116, 124, 132] and np.array_equal(ft.sum(axis=0), dt[1])
    # dmi 0: row k = 0 is DM index -1; with four rows at dmi 1, rows -1 and 2 are off the grid
    ft, fth, dt, dth = R.cutout(XT, DELAY, NOZAP, SERIES, 2, 4, 2, 0, 10, 2)
    assert dth.tolist() == [[0, 0, 0, 0], [2, 2, 2, 2]] and dt[0].tolist() == [0, 0, 0, 0]
    assert dt[1].tolist() == [532, 548, 564, 580]
    ft, fth, dt, dth = R.cutout(XT, DELAY, NOZAP, SERIES, 2, 4, 4, 1, 10, 2)
    assert dth[:, 0].tolist() == [0, 2, 2, 0] and np.array_equal(dt[2], ft.sum(axis=0))


def test_restatement_delays_follow_the_documented_rounding():
    d = R.delays([0.0, 100.0], 361.94, -0.16, 8, search.TSAMP)
    assert d[0].tolist() == [0] * 8 and d[1, 0] == 0 and np.all(np.diff(d[1]) > 0)
    f = float(np.float32(361.94)) + np.arange(8) * float(np.float32(-0.16))
    x = 4.148808e3 * 100.0 * (1.0 / (f[7] * f[7]) - 1.0 / (f[0] * f[0])) / float(np.float32(search.TSAMP))
    assert d[1, 7] == int(np.floor(x + 0.5))


def test_cli_cutout_flags(capsys):
    a = search.parse_args(["-f", "x.fil"])
    assert (a.output_dir, a.cutouts, a.cutout_thresh, a.cutout_max) == (None, False, 6.0, 32)
    a = search.parse_args(["-f", "x.fil", "-detect_thresh", "8", "-output_dir", "/tmp/c"])
    assert (a.output_dir, a.cutouts, a.cutout_thresh) == ("/tmp/c", False, 8.0)
    a = search.parse_args(["-f", "x.fil", "-output_dir", "d", "-cutouts", "-cutout_thresh", "9.5", "-cutout_max", "4"])
    assert (a.cutouts, a.cutout_thresh, a.cutout_max) == (True, 9.5, 4)
    with pytest.raises(SystemExit):
        search.parse_args(["-f", "x.fil", "-cutouts"])
    assert "-cutouts needs -output_dir" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        search.parse_args(["-f", "x.fil", "-output_dir", "d", "-cutouts", "-cutout_max", "0"])
    assert search.gulp_stem("2016-07-01-01:00:00", 0, search.TSAMP, 8) == "2016-07-01-01:00:00_08"
    assert search.gulp_stem("2016-07-01-23:59:59", 30720, search.TSAMP, 12) == "2016-07-02-00:00:23_12"   # + 24 s


def test_cutouts_npz_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    nsub, nt, nrow = 4, 6, 2

    def cand(i, with_cutout):
        c = dict(snr=10.0 - i, peak_idx=1000 + i, peak_time=0.1 * i, tfilt=i, dmi=3 + i, dm=20.5 + i, ngiant=5, i0=990, i1=1010)
        if with_cutout:
            c["cutout"] = dict(ft=rng.integers(0, 1 << 32, (nsub, nt), dtype=np.uint64).astype(np.uint32),
                               ft_hits=rng.integers(0, 99, (nsub, nt)).astype(np.uint32),
                               dt=rng.integers(0, 1 << 32, (nrow, nt), dtype=np.uint64).astype(np.uint32),
                               dt_hits=rng.integers(0, 64, (nrow, nt)).astype(np.uint32),
                               dm_rows=np.array([np.nan, 20.5 + i]), sub_freqs=np.linspace(360, 330, nsub), tscr=1 << i)
        return c

    cands = [cand(0, True), cand(1, False), cand(2, True)]
    path = str(tmp_path / "g.cutouts.npz")
    assert search.write_cutouts_npz(path, cands, search.TSAMP) == 2
    z = np.load(path)
    assert set(z.files) == {"ft", "ft_hits", "dt", "dt_hits", "dm_rows", "sub_freqs", "peak_idx", "dm", "snr", "tfilt",
                            "tscr", "tsamp"}
    for i, c in enumerate((cands[0], cands[2])):
        for k in ("ft", "ft_hits", "dt", "dt_hits"):
            assert z[k].dtype == np.uint32 and np.array_equal(z[k][i], c["cutout"][k]), k
        assert np.array_equal(z["dm_rows"][i], c["cutout"]["dm_rows"], equal_nan=True)
    assert z["peak_idx"].tolist() == [1000, 1002] and z["tfilt"].tolist() == [0, 2] and z["tscr"].tolist() == [1, 4]
    assert z["dm"].tolist() == [20.5, 22.5] and z["snr"].tolist() == [10.0, 8.0] and float(z["tsamp"]) == search.TSAMP
    assert np.array_equal(z["sub_freqs"], np.linspace(360, 330, nsub))
    # no candidate with a cutout: no file
    assert search.write_cutouts_npz(str(tmp_path / "none.npz"), [cand(1, False)], search.TSAMP) == 0
    assert not (tmp_path / "none.npz").exists()
