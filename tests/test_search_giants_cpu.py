"""The NumPy restatement of the giants-and-clusters definition (tests/search_giants_ref.py) against answers worked out by
hand from the text in include/pb_hip.h, the command line's new flags, and the new entry points in the header and the
binding.  No GPU."""
import importlib
import re

import numpy as np
import pytest

import search_giants_ref as R
from helpers import ROOT, header_symbols, libpb

search = importlib.import_module("vlite-fast_amd.search")

ENTRY_POINTS = ("pb_search_set_giants", "pb_search_giants", "pb_search_giant_list", "pb_search_set_planes",
                "pb_search_giant_timers")


def planes(ndm=6, tout=400):
    return np.zeros((ndm, tout), np.float32), np.zeros((ndm, tout), np.uint8)


def giants_of(snr, wl, thresh=5.0, **kw):
    r = R.giants_ref(snr, wl, thresh, **kw)
    g = r["giants"]
    return r, [tuple(int(g[k][i]) for k in ("dmi", "begin", "end", "npts", "peak", "tfilt")) for i in range(g["dmi"].size)]


def test_gaps_of_exactly_sep_time_and_one_more():
    snr, wl = planes()
    snr[0, [10, 13, 16]] = 6.0                      # 3 apart twice: one giant
    snr[1, [10, 14]] = 6.0                          # 4 apart: two
    snr[2, [63, 127]] = 6.0                         # 64 apart
    snr[3, [63, 128]] = 6.0                         # 65 apart
    r, g = giants_of(snr, wl, sep_time=3, sep_dm=0)
    assert g == [(0, 10, 17, 3, 10, 0), (1, 10, 11, 1, 10, 0), (1, 14, 15, 1, 14, 0), (2, 63, 64, 1, 63, 0),
                 (2, 127, 128, 1, 127, 0), (3, 63, 64, 1, 63, 0), (3, 128, 129, 1, 128, 0)]
    r, g = giants_of(snr, wl, sep_time=64, sep_dm=0)
    assert g == [(0, 10, 17, 3, 10, 0), (1, 10, 15, 2, 10, 0), (2, 63, 128, 2, 63, 0), (3, 63, 64, 1, 63, 0),
                 (3, 128, 129, 1, 128, 0)]


def test_a_run_cut_by_t_lo_and_by_t_hi_is_cut():
    snr, wl = planes()
    snr[2, 100:120] = 6.0 + np.arange(20)           # the largest S/N at 119
    wl[2, 100:120] = np.arange(20) % 7
    _, g = giants_of(snr, wl)
    assert g == [(2, 100, 120, 20, 119, 19 % 7)]
    _, g = giants_of(snr, wl, t_lo=105, t_hi=400)
    assert g == [(2, 105, 120, 15, 119, 19 % 7)]
    _, g = giants_of(snr, wl, t_lo=0, t_hi=110)     # two giants in two calls: this one and the next range's
    assert g == [(2, 100, 110, 10, 109, 9 % 7)]
    _, g = giants_of(snr, wl, t_lo=110, t_hi=111)
    assert g == [(2, 110, 111, 1, 110, 10 % 7)]


def test_equal_snr_inside_a_giant_and_between_members():
    snr, wl = planes()
    snr[1, 50:60] = 7.0
    wl[1, 50:60] = np.arange(10) % 5
    snr[2, 52:55] = 7.0
    wl[2, 52] = 3
    snr[4, 40:70] = 6.5
    r, g = giants_of(snr, wl, sep_dm=2)
    assert g == [(1, 50, 60, 10, 50, 0), (2, 52, 55, 3, 52, 3), (4, 40, 70, 30, 40, 0)]
    assert list(r["label"]) == [0, 0, 0]
    c = r["cands"]
    assert (c["snr"][0], c["peak"][0], c["tfilt"][0], c["dmi"][0]) == (np.float32(7.0), 50, 0, 1)     # giant 0, not giant 1
    assert (c["members"][0], c["npoints"][0], c["i0"][0], c["i1"][0]) == (3, 43, 40, 70)


def test_dm_distance_filter_difference_and_time_windows():
    def pair(d_b, tf_b, begin_b, **kw):
        snr, wl = planes(ndm=12)
        snr[2, 100:110] = 6.0
        wl[2, 100:110] = 1
        snr[d_b, begin_b:begin_b + 5] = 7.0
        wl[d_b, begin_b:begin_b + 5] = tf_b
        r, g = giants_of(snr, wl, **kw)
        assert len(g) == 2
        assert R.linked(r["giants"], 0, 1, kw["sep_time"], kw["sep_dm"], kw["sep_filter"]) == (len(r["cands"]["snr"]) == 1)
        return len(r["cands"]["snr"])

    par = dict(sep_time=3, sep_dm=4, sep_filter=2)
    assert pair(6, 1, 100, **par) == 1              # DM distance sep_dm
    assert pair(7, 1, 100, **par) == 2              # sep_dm + 1
    assert pair(3, 3, 100, **par) == 1              # filter difference sep_filter
    assert pair(3, 4, 100, **par) == 2              # sep_filter + 1
    assert pair(3, 1, 112, **par) == 1              # begin_b = 112 < end_a + sep_time = 113: the windows touch
    assert pair(3, 1, 113, **par) == 2              # and miss by one sample
    assert pair(3, 1, 93, **par) == 1               # the other side: begin_a = 100 < end_b + sep_time = 101
    assert pair(3, 1, 92, **par) == 2
    assert pair(2, 1, 113, **par) == 2              # two giants of one series never link


def test_a_chain_is_one_cluster():
    snr, wl = planes()
    snr[0, 100:110] = 6.0                           # A
    snr[1, 108:120] = 9.0                           # B overlaps A and C
    snr[2, 118:130] = 7.0                           # C does not reach A
    r, g = giants_of(snr, wl, sep_time=1, sep_dm=1)
    assert R.linked(r["giants"], 0, 1, 1, 1, 3) and R.linked(r["giants"], 1, 2, 1, 1, 3) and not R.linked(r["giants"], 0, 2, 1, 1, 3)
    assert list(r["label"]) == [0, 0, 0] and list(r["cands"]["members"]) == [3]
    assert (r["cands"]["dmi"][0], r["cands"]["peak"][0], r["cands"]["i0"][0], r["cands"]["i1"][0]) == (1, 108, 100, 130)
    r, g = giants_of(snr, wl, sep_time=1, sep_dm=0)
    assert list(r["label"]) == [0, 1, 2]
    s = R.sort_strongest_first(r["cands"])
    assert list(s["dmi"]) == [1, 2, 0]


def test_nan_and_infinite_samples():
    snr, wl = planes()
    snr[:] = -3.0
    snr[1, 10:16] = [8, np.nan, np.inf, np.nan, -np.inf, 8]
    _, g = giants_of(snr, wl, thresh=8.0)
    assert g == [(1, 10, 16, 3, 12, 0)]             # 10, 12 and 15: the NaNs are not hot, the gaps are <= 3
    _, g = giants_of(snr, wl, thresh=8.0, sep_time=1)
    assert g == [(1, 10, 11, 1, 10, 0), (1, 12, 13, 1, 12, 0), (1, 15, 16, 1, 15, 0)]
    r, g = giants_of(snr, wl, thresh=float("-inf"), sep_time=1, sep_dm=0)
    assert r["ngiants"] == 6 + 2 and g[1] == (1, 0, 11, 11, 10, 0) and g[2] == (1, 12, 13, 1, 12, 0) and g[3] == (1, 14, 400, 386, 15, 0)


def test_the_overflow_rule():
    snr, wl = planes()
    snr[:, ::100] = 6.0
    assert R.giants_ref(snr, wl, 5.0, max_giants=24)["overflow"] is False
    r = R.giants_ref(snr, wl, 5.0, max_giants=23)
    assert r["overflow"] is True and r["ngiants"] == 24 and r["giants"]["dmi"].size == 0 and r["cands"]["snr"].size == 0
    assert r["label"].size == 0


def test_candidates_from_giants_are_the_search_s_dicts():
    res = dict(snr=np.array([6.5, 9.0, 9.0], np.float32), peak=np.array([5, 90, 40]), tfilt=np.array([0, 2, 3]),
               dmi=np.array([1, 4, 4]), members=np.array([1, 7, 2]), npoints=np.array([1, 30, 4]), i0=np.array([5, 80, 38]),
               i1=np.array([6, 99, 44]), ngiants=10, overflow=False)
    dms = 2.0 * np.arange(6)
    c = search.candidates_from_giants(res, dms, 0.001, sample0=1000)
    assert [x["peak_idx"] for x in c] == [1040, 1090, 1005]
    assert c[0] == dict(snr=9.0, peak_idx=1040, peak_time=1.04, tfilt=3, dmi=4, dm=8.0, ngiant=2, i0=1038, i1=1044, npoints=4)
    assert len(search.candidate_line(c[0]).split()) == 9
    assert search.candidates_from_giants(dict(res, snr=res["snr"][:0]), dms, 0.001) == []


def test_command_line_flags_and_refusals(capsys):
    a = search.parse_args(["-f", "x.fil"])
    assert (a.giants, a.cand_sep_time, a.cand_sep_dm, a.cand_sep_filter, a.max_giants) == (False, 3, 200, 3, 1 << 18)
    a = search.parse_args(["-f", "x.fil", "-giants", "-cand_sep_time", "64", "-cand_sep_dm", "0", "-cand_sep_filter", "0",
                           "-max_giants", "1000"])
    assert (a.giants, a.cand_sep_time, a.cand_sep_dm, a.cand_sep_filter, a.max_giants) == (True, 64, 0, 0, 1000)
    for bad in (["-cand_sep_time", "0"], ["-cand_sep_time", "65"], ["-cand_sep_dm", "-1"], ["-cand_sep_filter", "-1"],
                ["-max_giants", "0"], ["-max_giants", str((1 << 22) + 1)], ["-cand_sep_time", "1.5"]):
        with pytest.raises(SystemExit):
            search.parse_args(["-f", "x.fil", "-giants"] + bad)
    capsys.readouterr()


def test_header_and_binding_carry_the_entry_points():
    names = header_symbols()
    lp = libpb()
    for n in ENTRY_POINTS:
        assert n in names and n in lp.EXPORTS, n
    txt = open(ROOT + "/include/pb_hip.h").read()
    assert re.search(r"#define PB_GIANT_WORDS 8\b", txt)
    sec = txt[txt.index("Giants and clusters of giants"):txt.index("int pb_search_set_giants")]
    for word in ("hot", "maximal", "ascending (dmi, begin)", "connected components", "smallest member index", "max_giants",
                 "two giants in two calls"):
        assert word in sec, word
