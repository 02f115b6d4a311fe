"""The sub-band search without a GPU: the NumPy restatement (tests/search_subband_ref.py) against numbers worked out by
hand, the default band list, the candidates made from a point list, the CLI flags and the .subband file, the ABI's
declarations and the refusals that need no device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import search_subband_ref as R
from helpers import ROOT, libpb

search = importlib.import_module("vlite-fast_amd.search")
EINVAL = -22          # PB_EINVAL
NAMES = ("pb_search_set_subbands", "pb_search_subbands", "pb_search_subband_dm", "pb_search_subband_timers")

# the hand-made block: 4 channels x 40 samples, xt[c][t] = 40 c + t; delays 0, 1, 2, 4: max_delay 4, tout 36; two base
# sub-bands of two channels
XT = (40 * np.arange(4)[:, None] + np.arange(40)[None, :]).astype(np.uint8)
DELAY = np.array([0, 1, 2, 4])
T = np.arange(36)


def test_restatement_sub_band_and_band_sums_by_hand():
    S = R.sub_series(XT, DELAY, np.zeros(4, bool), 2, 36)
    # sub-band 0: xt[0][t] + xt[1][t + 1] = t + (41 + t); sub-band 1: xt[2][t + 2] + xt[3][t + 4] = (82 + t) + (124 + t)
    assert S[0].tolist() == (41 + 2 * T).tolist() and S[1].tolist() == (206 + 2 * T).tolist()
    # they add up to the search's series: 0 + 41 + 82 + 124 at t = 0, four more per sample
    assert S.sum(axis=0).tolist() == (247 + 4 * T).tolist()
    # the default list of nsb 2 is the two halves, so the band series are the sub-band series
    assert R.band_list(2) == [(0, 1), (1, 1)] and np.array_equal(R.band_series(S, R.band_list(2)), S)
    # a band of both (what the ABI refuses, but the sum is defined) and a zapped channel: channel 2 drops out of sub-band 1
    assert R.band_series(S, [(0, 2)])[0].tolist() == (247 + 4 * T).tolist()
    Z = R.sub_series(XT, DELAY, np.array([False, False, True, False]), 2, 36)
    assert Z[0].tolist() == S[0].tolist() and Z[1].tolist() == (124 + T).tolist()
    # an emptied sub-band is zero
    Z = R.sub_series(XT, DELAY, np.array([True, True, False, False]), 2, 36)
    assert not Z[0].any() and Z[1].tolist() == S[1].tolist()
    # four sub-bands of one channel, bands (1, 2) and (3, 1)
    S4 = R.sub_series(XT, DELAY, np.zeros(4, bool), 4, 36)
    B = R.band_series(S4, [(1, 2), (3, 1)])
    assert B[0].tolist() == (41 + 82 + 2 * T).tolist() and B[1].tolist() == (124 + T).tolist()


NAN = float("nan")
#                  tie 0/1  tie 1/2  -0 / +0  NaNs   equal to full  plain  all NaN  full NaN
BAND_SNR = np.array([[5.0,   8.0,    -0.0,    NAN,   9.0,           9.0,   NAN,     9.0],
                     [5.0,   9.0,     0.0,    7.0,   3.0,           9.5,   NAN,     1.0],
                     [4.0,   9.0,     0.0,    NAN,   2.0,           1.0,   NAN,     2.0]], np.float32)
BAND_WID = np.array([[1, 1, 1, 1, 1, 1, 1, 1], [2, 2, 2, 2, 2, 2, 2, 2], [3, 3, 3, 3, 3, 3, 3, 3]], np.uint8)
FULL = np.array([1.0, 9.0, -1.0, 1.0, 9.0, 2.0, 0.0, NAN], np.float32)


def bits(v):
    return int(np.array([v], np.float32).view(np.int32)[0])


def test_best_band_by_hand():
    best, wid, bi = R.best_band(BAND_SNR, BAND_WID)
    assert bi.tolist() == [0, 1, 0, 1, 0, 1, 0, 0]              # ties keep the smaller index, a NaN never wins
    assert wid.tolist() == [1, 2, 1, 2, 1, 2, 1, 1]
    assert best[:6].tolist() == [5.0, 9.0, 0.0, 7.0, 9.0, 9.5] and np.signbit(best[2])     # band 0's -0, bit for bit
    assert np.isnan(best[6]) and best[7] == 9.0


def test_points_by_hand():
    # threshold 5 over the whole range: the tie at 5 (>= is enough, and 5 > 1); not the cell equal to its full-band value,
    # not the zero, not the NaNs (neither a NaN best nor a NaN full band reports)
    got = R.points(BAND_SNR, BAND_WID, FULL, 5.0, 0, 8, dmi=3)
    assert got == {(3, 0, bits(5.0), 1, 0, bits(1.0)), (3, 3, bits(7.0), 2, 1, bits(1.0)), (3, 5, bits(9.5), 2, 1, bits(2.0))}
    # the range cuts: t_lo is inside, t_hi is not
    assert R.points(BAND_SNR, BAND_WID, FULL, 5.0, 3, 5) == {(0, 3, bits(7.0), 2, 1, bits(1.0))}
    assert R.points(BAND_SNR, BAND_WID, FULL, 5.0, 1, 3) == set()
    # a higher threshold; and the full band one ulp lower lets the equal cell through
    assert R.points(BAND_SNR, BAND_WID, FULL, 9.25, 0, 8) == {(0, 5, bits(9.5), 2, 1, bits(2.0))}
    full = FULL.copy()
    full[4] = np.nextafter(np.float32(9.0), np.float32(0.0))
    assert (0, 4, bits(9.0), 1, 0, bits(full[4])) in R.points(BAND_SNR, BAND_WID, full, 5.0, 0, 8)


NSB8 = [(0, 4), (2, 4), (4, 4), (0, 2), (1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (6, 2),
        (0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1)]


def test_subband_list():
    assert [len(search.subband_list(n)) for n in (2, 4, 8, 16)] == [2, 7, 18, 41]
    assert search.subband_list(8) == NSB8
    for n in (2, 4, 8, 16):
        got = search.subband_list(n)
        assert got == R.band_list(n) and len(set(got)) == len(got) and len(got) <= 64
        assert all(c >= 1 and c < n and f >= 0 and f + c <= n for f, c in got)
    # the stagger: the middle half of the band is a band of its own
    assert (2, 4) in search.subband_list(8) and (4, 8) in search.subband_list(16) and (1, 2) in search.subband_list(4)
    with pytest.raises(ValueError):
        search.subband_list(3)


def test_cli_subband_flags(capsys):
    a = search.parse_args(["-f", "x.fil"])
    assert not any(hasattr(a, k) for k in ("subbands", "subband_thresh", "subband_send"))     # the namespace it always gave
    a = search.parse_args(["-f", "x.fil", "-subbands", "0"])
    assert not hasattr(a, "subbands")
    a = search.parse_args(["-f", "x.fil", "-detect_thresh", "8", "-subbands", "8"])
    assert (a.subbands, a.subband_thresh, a.subband_send) == (8, 8.0, False)
    a = search.parse_args(["-f", "x.fil", "-subbands", "16", "-subband_thresh", "7.5", "-subband_send"])
    assert (a.subbands, a.subband_thresh, a.subband_send) == (16, 7.5, True)
    # the host that feeds the search itself takes them through the same parser
    a = search.parse_flags("-subbands 4 -subband_thresh 9")
    assert (a.subbands, a.subband_thresh, a.subband_send) == (4, 9.0, False)
    for bad in (["-subbands", "3"], ["-subband_thresh", "7"], ["-subband_send"], ["-subbands", "8", "-pol"]):
        with pytest.raises(SystemExit):
            search.parse_args(["-f", "x.fil"] + bad)
        assert "-subband" in capsys.readouterr().err


def hand_points():
    """three points of one event: the strongest at (DM index 2, sample 100) in band 5 of the nsb 8 list"""
    return dict(dmi=np.array([2, 3, 2]), t=np.array([101, 100, 100]), snr=np.array([8.0, 7.5, 9.0], np.float32),
                width_log2=np.array([1, 0, 1], np.uint8), band=np.array([3, 5, 5]), snr_full=np.array([3.5, 3.0, 4.0], np.float32))


def test_candidates_from_a_point_list():
    dms = np.array([0.0, 38.0, 40.0, 41.0])
    cands = search.candidates_from_subbands(hand_points(), dms, 1e-3, NSB8, 8, 384.0, -0.25, 256, sample0=1000)
    assert len(cands) == 1
    c = cands[0]
    assert (c["snr"], c["dmi"], c["dm"], c["peak_idx"], c["tfilt"], c["ngiant"]) == (9.0, 2, 40.0, 1100, 1, 3)
    assert (c["i0"], c["i1"]) == (1100, 1103)
    # the strongest point's band: base sub-bands 2 and 3 of 8 = channels [64, 128), whose outer edges are half a channel
    # beyond the centres 384 - 0.25 * 64 and 384 - 0.25 * 127
    assert c["band"] == (2, 2) and c["snr_full"] == 4.0
    assert (c["f_lo"], c["f_hi"]) == (352.125, 368.125)
    # an ascending band: the same channels, the edges the other way round
    c = search.candidates_from_subbands(hand_points(), dms, 1e-3, NSB8, 8, 320.0, 0.25, 256)[0]
    assert (c["f_lo"], c["f_hi"]) == (335.875, 351.875) and c["peak_idx"] == 100
    assert search.candidates_from_subbands({k: v[:0] for k, v in hand_points().items()}, dms, 1e-3, NSB8, 8, 384.0, -0.25, 256) == []


def test_subband_line_and_file(tmp_path):
    dms = np.array([0.0, 38.0, 40.0, 41.0])
    c = search.candidates_from_subbands(hand_points(), dms, 1e-3, NSB8, 8, 384.0, -0.25, 256, sample0=1000)[0]
    line = search.subband_line(c)
    assert line == search.candidate_line(c) + "\t2\t2\t352.1250\t368.1250\t4.0000"
    assert line == "9.000000\t1100\t1.100000\t1\t2\t40.0000\t3\t1100\t1103\t2\t2\t352.1250\t368.1250\t4.0000"
    full = dict(snr=10.0, peak_idx=5, peak_time=0.005, tfilt=0, dmi=1, dm=38.0, ngiant=1, i0=5, i1=6)
    path = str(tmp_path / "g.subband")
    assert search.write_subbands(path, [full, c]) == 1             # only the candidates that carry a band
    assert open(path).read() == line + "\n"
    assert search.write_subbands(str(tmp_path / "none.subband"), [full]) == 0 and not (tmp_path / "none.subband").exists()


def test_header_declares_and_library_exports_the_subband_functions():
    hdr = open(os.path.join(ROOT, "include", "pb_hip.h")).read()
    assert re.search(r"\bint\s+pb_search_set_subbands\(pb_search \*s, int nsb, const int32_t \*bands2, int nbands, int dm_chunk, "
                     r"int max_points\);", hdr)
    assert re.search(r"\bint\s+pb_search_subbands\(pb_search \*s, float thresh, int t_lo, int t_hi, int32_t \*points, int max_out, "
                     r"int \*npoints, int \*overflow\);", hdr)
    assert re.search(r"#define PB_SUBPOINT_WORDS 6\b", hdr)
    lp = libpb()
    L = lp.load()
    for n in NAMES:
        assert n in lp.EXPORTS
        assert getattr(L, n).restype is C.c_int and getattr(L, n).argtypes


def test_refusals_that_need_no_device():
    L = libpb().load()
    b = (C.c_int32 * 2)(0, 1)
    assert L.pb_search_set_subbands(None, 2, b, 1, 0, 16) == EINVAL
    assert "no search handle" in L.pb_search_last_error(None).decode()
    pts, n, ov = (C.c_int32 * 6)(), C.c_int(), C.c_int()
    assert L.pb_search_subbands(None, 7.0, 0, 1, pts, 1, C.byref(n), C.byref(ov)) == EINVAL
    assert "no search handle" in L.pb_search_last_error(None).decode()
    assert L.pb_search_subband_dm(None, 0, None, None, None, None, None, None, None) == EINVAL
    assert L.pb_search_subband_timers(None, (C.c_float * 4)()) == EINVAL


class _FakeSearcher(object):
    """what GulpSearch's constructor reads of a searcher"""
    nbox, nchan, max_delay, _cut, _ref = 7, 256, 0, None, None

    def __init__(self, sub=(8, NSB8, 16), pol=None):
        self._sub, self._pol = sub, pol

    def _nif(self):
        return 1


def test_gulp_search_wiring():
    with pytest.raises(ValueError, match="set_subbands"):
        search.GulpSearch(_FakeSearcher(sub=None), subbands=dict(thresh=7.0))
    with pytest.raises(ValueError, match="pol"):
        search.GulpSearch(_FakeSearcher(pol=(64, 8, (0.0, 1.0, 1), 4)), subbands=dict(thresh=7.0), pol=dict(thresh=7.0))
    # the batch is the full-band candidates followed by the sub-band ones; the coincidencer leg sees the latter only with send
    for send, seen in ((False, [["full"]]), (True, [["full", "sub"]])):
        g = search.GulpSearch(_FakeSearcher(), threshold=6.0, subbands=dict(thresh=7.0, send=send))
        assert g.sub == (7.0, send)
        sent = []
        g._send = lambda cands, first, nsamps: sent.append(list(cands))
        assert g._out(["full"], ["sub"], 0, 10) == ["full", "sub"] and sent == seen
    g = search.GulpSearch(_FakeSearcher(), threshold=6.0)
    assert g.sub is None and g._out(["full"], [], 0, 10) == ["full"] and g._pending_sub() == []
