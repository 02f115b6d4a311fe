"""The periodicity search without a GPU: the NumPy restatement (tests/search_periodic_ref.py) -- the stage recursion against
the closed form, both against answers made by hand, the S/N against a direct float64 evaluation, the tie rules --, the
detection case that the GPU test runs (tests/search_periodic_cases.py), and the host side: the harmonic grouping, the octave
arithmetic, the flags, the .periodic file, the ABI's declarations and the refusals that need no device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import search_periodic_cases as CASE
import search_periodic_ref as R
from helpers import ROOT, libpb

search = importlib.import_module("vlite-fast_amd.search")
EINVAL = -22          # PB_EINVAL
NAMES = ("pb_search_set_periodic", "pb_search_periodic", "pb_search_periodic_fold", "pb_search_periodic_timers")


@pytest.mark.parametrize("p,m,extra", [(37, 18, 5), (32, 16, 0), (63, 17, 62), (40, 2, 3), (45, 3, 0), (33, 9, 1)])
def test_recursion_equals_closed_form(p, m, extra):
    x = np.random.default_rng(p * m).integers(0, 1 << 20, p * m + extra)
    a, b = R.fold_stages(x, p), R.fold_closed(x, p)
    mm, M, L = R.rows_of(len(x), p)
    assert mm == m and M == 1 << L and M >= m > M // 2 and a.shape == (M, p)
    assert np.array_equal(a, b)
    assert np.array_equal(a.sum(axis=1), np.full(M, x[:m * p].sum()))       # every trial holds every used sample once
    assert np.array_equal(a[0], x[:m * p].reshape(m, p).sum(axis=0))        # trial 0 rotates nothing


def test_shift_by_hand():
    # L = 2, four rows: trial i rotates row r by s_2(r, i); i = 3 is the steepest, one more bin per row but the last pair
    assert [[R.shift(2, r, i) for r in range(4)] for i in range(4)] == [[0, 0, 0, 0], [0, 0, 1, 1], [0, 1, 1, 2], [0, 1, 2, 3]]
    assert [R.shift(3, r, 7) for r in range(8)] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert [R.shift(3, r, 0) for r in range(8)] == [0] * 8


def test_downsample_by_hand():
    x = np.arange(11)
    assert R.downsample(x, 0).tolist() == list(range(11))
    assert R.downsample(x, 1).tolist() == [1, 5, 9, 13, 17]
    assert R.downsample(x, 2).tolist() == [6, 22]
    assert R.downsample(x, 4).tolist() == []


def test_one_every_fortieth_sample():
    x = np.zeros(40 * 16 + 7, np.uint32)
    x[5::40] = 1
    F = R.fold_stages(x, 40)
    m, M, L = R.rows_of(len(x), 40)
    assert (m, M, L) == (16, 16, 4)
    want = np.zeros(40, np.uint64)
    want[5] = 16
    assert np.array_equal(F[0], want)
    snr, jb = R.evaluate(F, 32, m, 0, 0.25)
    s, i, q, j = R.best_of(snr, jb)
    assert (i, q, j) == (0, 0, 5)
    # p Smax - w T = 40 x 16 - 16 over rms sqrt(m w (p - w) p) = 0.25 sqrt(16 x 39 x 40)
    assert s == np.float32(624.0 / (0.25 * np.sqrt(16.0 * 39.0 * 40.0)))
    # the steepest trial smears the 16 pulses over 16 bins
    assert F[15].max() == 1 and F[15].sum() == 16


def test_period_forty_and_a_half():
    n = 40 * 32
    x = np.zeros(n, np.uint32)
    x[np.floor(np.arange(0, n - 1, 40.5)).astype(int)] = 1
    F = R.fold_stages(x, 40)
    m, M, _ = R.rows_of(n, 40)
    assert (m, M) == (32, 32)
    snr, jb = R.evaluate(F, 32, m, 0, 1.0)
    _, i, q, _ = R.best_of(snr, jb)
    assert i in (15, 16), i                                                 # (M - 1) / 2 = 15.5
    assert abs(R.period_samples(40, i, M) - 40.5) <= 0.5 / (M - 1) + 1e-12


def test_constant_series_and_skipped():
    x = np.full(500, 7, np.uint32)
    b = R.search_series(x, np.float32(1.0), 32, 0, 3)
    for ki in range(4):
        for p in range(32, 64):
            m = (500 >> ki) // p
            assert b["m"][ki, p - 32] == m
            if m >= 2:
                assert (b["snr"][ki, p - 32], b["i"][ki, p - 32], b["q"][ki, p - 32], b["j"][ki, p - 32]) == (0.0, 0, 0, 0)
                assert b["M"][ki, p - 32] == 1 << int(m - 1).bit_length()
            else:
                assert (b["snr"][ki, p - 32], b["i"][ki, p - 32], b["M"][ki, p - 32]) == (0.0, -1, 0)
    assert (b["i"][3] == -1).all() and (b["i"][0] == 0).all()              # 62 samples at octave 3: m < 2 for every p
    assert R.fold_stages(np.arange(63), 32) is None and R.fold_closed(np.arange(63), 32) is None
    # rms not above 0: S/N 0 whatever the profile
    F = R.fold_stages(np.arange(200), 33)
    assert not R.evaluate(F, 32, 6, 0, 0.0)[0].any() and not R.evaluate(F, 32, 6, 0, -1.0)[0].any()


def test_snr_against_direct_float64():
    rng = np.random.default_rng(5)
    for p, m, k, B in ((37, 18, 0, 32), (127, 5, 3, 64), (255, 2, 12, 128), (64, 300, 1, 64)):
        x = rng.integers(0, 255 * 60, p * m)
        F = R.fold_stages(x, p)
        rms = np.float32(rng.uniform(50, 500))
        snr, jb = R.evaluate(F, B, m, k, rms)
        assert snr.shape == (F.shape[0], int(np.log2(B))) and R.widths(B)[-1] == B // 2
        f = F.astype(np.float64)
        for q, w in enumerate(R.widths(B)):
            S = np.stack([np.take(f, (np.arange(p) + u) % p, axis=1) for u in range(w)]).sum(axis=0)
            # mean removed, noise of a sum of m 2^k w samples with the factor 1 - w / p
            direct = (S.max(axis=1) - w * f.mean(axis=1)) / (float(rms) * np.sqrt(m * 2.0 ** k * w * (1.0 - w / p)))
            assert np.array_equal(jb[:, q], S.argmax(axis=1))
            ulp = np.spacing(np.abs(direct).astype(np.float32)).astype(np.float64)
            assert (np.abs(snr[:, q].astype(np.float64) - direct) <= ulp).all(), (p, q)


def test_circular_window():
    # a pulse in bins p - 1 and 0: the window of width 2 that holds both starts at p - 1
    F = np.zeros((2, 35), np.uint64)
    F[:, 34] = F[:, 0] = 10
    snr, jb = R.evaluate(F, 32, 2, 0, 1.0)
    # widths 1 (the first of two equal bins), 2 (only the window from p - 1 holds both), 4, 8, 16 (the smallest start of
    # the windows that hold both: p - 1 - (w - 2))
    assert jb[0].tolist() == [0, 34, 32, 28, 20]
    assert snr[0, 1] > snr[0, 0] and snr[0, 1] > snr[0, 2]


def test_tie_rules():
    snr = np.array([[1, 3, 3], [3, 3, 0], [2, 5, 5], [5, 5, 1], [5, 0, 0]], np.float32)
    jb = np.arange(15, dtype=np.int32).reshape(5, 3)
    assert R.best_of(snr, jb) == (np.float32(5), 2, 1, 7)                   # smaller q within a trial, smaller i between trials
    assert R.best_of(snr[:2], jb[:2]) == (np.float32(3), 0, 1, 1)
    assert R.best_of(np.zeros((4, 3), np.float32), jb[:4]) == (np.float32(0), 0, 0, 0)


def test_detection_case_in_the_restatement():
    """What tests/test_gpu_search_periodic.py's detection test relies on: seed 0 gives single-pulse S/N 3.95 at most, a
    periodic S/N of 15.82 at DM index 2 (p 41, i 48 of 128: 41.378 samples) and at most 5.04 at the other DMs."""
    r = CASE.restated()
    b = r["best"][2]
    k = int(np.argmax(b["snr"][0]))
    print("single %.3f; periodic per DM %s; p %d i %d M %d" % (r["single"], [float(x["snr"].max()) for x in r["best"]],
                                                              32 + k, b["i"][0, k], b["M"][0, k]))
    assert r["single"] < 6
    assert b["snr"][0, k] >= 10 and 32 + k == 41
    m, M, i, q = int(b["m"][0, k]), int(b["M"][0, k]), int(b["i"][0, k]), int(b["q"][0, k])
    assert abs(R.period_samples(41, i, M) / CASE.PERIOD - 1) <= ((1 << q) + 1.0) / (m * 41)
    assert all(float(r["best"][d]["snr"].max()) < b["snr"][0, k] for d in (0, 1, 3, 4))


# ---- the host side ----
def _table(entries, ndm=3, nk=2, B=32, tout=4096, tsamp=1e-3):
    """a Searcher.periodic() result with the given {(dmi, ki, p): (snr, i, q, j)} and zeros elsewhere"""
    res = dict(snr=np.zeros((ndm, nk, B), np.float32), i=np.zeros((ndm, nk, B), np.int32), q=np.zeros((ndm, nk, B), np.int32),
               j=np.zeros((ndm, nk, B), np.int32), octaves=np.arange(nk), p=np.arange(B, 2 * B))
    m = np.array([[(tout >> k) // p for p in range(B, 2 * B)] for k in range(nk)], np.int32)
    M = np.array([[1 << int(v - 1).bit_length() for v in row] for row in m], np.int32)
    res["m"], res["M"] = np.broadcast_to(m, (ndm, nk, B)).copy(), np.broadcast_to(M, (ndm, nk, B)).copy()
    for (d, ki, p), (s, i, q, j) in entries.items():
        res["snr"][d, ki, p - B], res["i"][d, ki, p - B], res["q"][d, ki, p - B], res["j"][d, ki, p - B] = s, i, q, j
    res["period_s"] = (res["p"][None, None, :] + res["i"] / (res["M"] - 1.0)) * (2.0 ** res["octaves"])[None, :, None] * tsamp
    return res


def test_harmonic_grouping():
    dms = [0.0, 20.0, 40.0]
    # the candidate: p 41, i 48 of 128 at octave 0: 41.378 ms; m = 99, q = 1: tolerance 3 / (99 x 41) = 7.4e-4
    res = _table({(2, 0, 41): (17.0, 48, 1, 6),
                  (1, 0, 41): (12.0, 47, 2, 5),         # the next trial at another DM: 41.370, ratio 1/1
                  (2, 0, 62): (11.0, 9, 1, 3),          # 62.0709 = 3/2 x 41.3806: inside
                  (0, 0, 50): (10.0, 0, 0, 0),          # 50 ms = 1.2084 x: 6/5 is 7e-3 away, no ratio of 1..8 within 7.4e-4
                  (1, 1, 41): (9.0, 24, 0, 1),          # octave 1, i 24 of 64: 82.762 ms, ratio 2/1
                  (0, 1, 50): (7.9, 1, 0, 0)})          # below the threshold
    c = search.candidates_from_periodic(res, dms, 1e-3, 8.0)
    assert [(x["dmi"], x["k"], x["p"]) for x in c] == [(2, 0, 41), (0, 0, 50)]
    a = c[0]
    assert (a["snr"], a["i"], a["q"], a["j"], a["m"], a["M"], a["dm"]) == (17.0, 48, 1, 6, 99, 128, 40.0)
    assert a["period_s"] == pytest.approx((41 + 48 / 127.0) * 1e-3, rel=1e-12) and a["width_s"] == 2e-3 and a["phase"] == 6 / 41.0
    assert a["nabsorbed"] == 3 and a["nharm"] == "1/1"                      # the strongest absorbed entry is the 12.0 one
    assert c[1]["nabsorbed"] == 0 and c[1]["nharm"] == "1/1"
    assert search.harmonic_ratio(62.0709, 41.378, 7.4e-4) == (3, 2) and search.harmonic_ratio(50.0, 41.378, 7.4e-4) is None
    # without the 1/1 entry the 3/2 harmonic is the strongest absorbed
    res["snr"][1, 0, 41 - 32] = 0
    assert search.candidates_from_periodic(res, dms, 1e-3, 8.0)[0]["nharm"] == "3/2"
    # at most max_cands; a period range leaves out what lies outside it; skipped entries never come back
    assert len(search.candidates_from_periodic(res, dms, 1e-3, 8.0, max_cands=1)) == 1
    c = search.candidates_from_periodic(res, dms, 1e-3, 8.0, p_range=(0.045, 0.07))
    assert [(x["dmi"], x["k"], x["p"]) for x in c] == [(2, 0, 62), (0, 0, 50)]
    res["i"][0, 0, 50 - 32] = -1
    assert len(search.candidates_from_periodic(res, dms, 1e-3, 8.0)) == 1
    assert search.candidates_from_periodic(_table({}), dms, 1e-3, 8.0) == []


def test_octaves():
    ts = 781.25e-6
    assert search.periodic_octaves(0.025, 0.06, 32, ts) == (0, 1)           # 32 ts = 0.025 s exactly: octave 0 starts there
    assert search.periodic_octaves(0.05, 3.2, 64, ts) == (0, 6)
    assert search.periodic_octaves(0.001, 0.03, 32, ts) == (0, 0)           # a lower end below the shortest period is cut
    assert search.periodic_octaves(0.21, 0.21, 64, ts) == (2, 2)
    with pytest.raises(ValueError, match="shortest searchable period, 0.05 s"):
        search.periodic_octaves(0.01, 0.049, 64, ts)
    with pytest.raises(ValueError, match="longest searchable period"):
        search.periodic_octaves(1.0, 64 * ts * 8192, 64, ts)
    assert search.periodic_octaves(1.0, 64 * ts * 8191, 64, ts) == (4, 12)
    with pytest.raises(ValueError):
        search.periodic_octaves(0.5, 0.4, 64, ts)


def test_cli_periodic_flags(capsys):
    a = search.parse_args(["-f", "x.fil"])
    assert not any(hasattr(a, k) for k in ("periodic", "periodic_bins", "periodic_thresh", "periodic_max"))
    a = search.parse_args(["-f", "x.fil", "-periodic", "0.05", "3.2"])
    assert (a.periodic, a.periodic_bins, a.periodic_thresh, a.periodic_max) == ([0.05, 3.2], 64, 8.0, 64)
    a = search.parse_args(["-f", "x.fil", "-periodic", "0.025", "0.06", "-periodic_bins", "32", "-periodic_thresh", "9.5",
                           "-periodic_max", "3", "-subbands", "8"])
    assert (a.periodic, a.periodic_bins, a.periodic_thresh, a.periodic_max, a.subbands) == ([0.025, 0.06], 32, 9.5, 3, 8)
    a = search.parse_flags("-periodic 0.1 0.2 -periodic_bins 128")             # a host that feeds the search takes them too
    assert (a.periodic, a.periodic_bins) == ([0.1, 0.2], 128)
    for bad in (["-periodic_bins", "64"], ["-periodic_thresh", "7"], ["-periodic_max", "3"], ["-periodic", "0.05", "3.2", "-pol"],
                ["-periodic", "0.05", "3.2", "-periodic_bins", "48"], ["-periodic", "0.2", "0.1"], ["-periodic", "0", "1"],
                ["-periodic", "0.05", "3.2", "-periodic_max", "0"]):
        with pytest.raises(SystemExit):
            search.parse_args(["-f", "x.fil"] + bad)
        assert "-periodic" in capsys.readouterr().err


def test_periodic_line_and_file(tmp_path):
    res = _table({(2, 0, 41): (17.25, 48, 1, 6)})
    c = search.candidates_from_periodic(res, [0.0, 20.0, 40.0], 1e-3, 8.0)[0]
    line = search.periodic_line(c)
    col = line.split("\t")
    assert len(col) == 11 and col[0] == "17.2500" and col[2] == "40.0000" and col[5:] == ["2", "0", "41", "48", "99", "1/1"]
    assert float(col[1]) == pytest.approx(0.041377953, abs=1e-9) and float(col[3]) == 0.002 and float(col[4]) == pytest.approx(6 / 41.0, abs=1e-6)
    full = dict(snr=9.0, peak_idx=1, peak_time=0.001, tfilt=0, dmi=0, dm=0.0, ngiant=1, i0=1, i1=2)
    path = str(tmp_path / "g.periodic")
    assert search.write_periodic(path, [full, c]) == 1                      # only the candidates that carry a period
    assert open(path).read() == line + "\n"
    assert search.write_periodic(str(tmp_path / "none.periodic"), [full]) == 0 and not (tmp_path / "none.periodic").exists()


def test_header_declares_and_library_exports_the_periodic_functions():
    hdr = open(os.path.join(ROOT, "include", "pb_hip.h")).read()
    assert re.search(r"\bint\s+pb_search_set_periodic\(pb_search \*s, int bins, int k_lo, int k_hi, int dm_chunk\);", hdr)
    assert re.search(r"\bint\s+pb_search_periodic\(pb_search \*s, int32_t \*best\);", hdr)
    assert re.search(r"\bint\s+pb_search_periodic_fold\(pb_search \*s, int dmi, int k, int p, uint32_t \*prof, float \*snr, "
                     r"int32_t \*jbest, int \*m, int \*M\);", hdr)
    assert re.search(r"\bint\s+pb_search_periodic_timers\(const pb_search \*s, float \*ms3\);", hdr)
    lp = libpb()
    L = lp.load()
    for n in NAMES:
        assert n in lp.EXPORTS
        assert getattr(L, n).restype is C.c_int and getattr(L, n).argtypes


def test_refusals_that_need_no_device():
    L = libpb().load()
    assert L.pb_search_set_periodic(None, 64, 0, 0, 0) == EINVAL
    assert "no search handle" in L.pb_search_last_error(None).decode()
    assert L.pb_search_periodic(None, (C.c_int32 * 4)()) == EINVAL
    assert "no search handle" in L.pb_search_last_error(None).decode()
    assert L.pb_search_periodic_fold(None, 0, 0, 64, None, None, None, None, None) == EINVAL
    assert L.pb_search_periodic_timers(None, (C.c_float * 3)()) == EINVAL


class _FakeSearcher(object):
    """what GulpSearch's constructor reads of a searcher"""
    nbox, nchan, max_delay, _cut, _ref, _sub, _pol = 7, 256, 0, None, None, None, None

    def __init__(self, per=(32, 0, 1)):
        self._per = per

    def _nif(self):
        return 1


def test_gulp_search_wiring():
    with pytest.raises(ValueError, match="set_periodic"):
        search.GulpSearch(_FakeSearcher(per=None), periodic=dict(thresh=8.0))
    g = search.GulpSearch(_FakeSearcher(), threshold=6.0, periodic=dict(thresh=9.0, max_per_gulp=5, p_range=(0.1, 0.2)))
    assert g.per == (9.0, 5, (0.1, 0.2))
    assert search.GulpSearch(_FakeSearcher(), periodic={}).per == (8.0, 64, None)
    # the periodicity candidates come last and never reach the coincidencer leg
    sent = []
    g._send = lambda cands, first, nsamps: sent.append(list(cands))
    g.per_cands = ["per"]
    assert g._out(["full"], [], 0, 10) == ["full", "per"] and sent == [["full"]]
    assert g._out(["full"], [], 0, 10) == ["full"]                          # handed on once
    g = search.GulpSearch(_FakeSearcher(), threshold=6.0)
    assert g.per is None and g._out(["full"], [], 0, 10) == ["full"]
