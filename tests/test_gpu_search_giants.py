"""Giants and clusters of giants on the GPU (pb_search_set_giants / pb_search_giants, Searcher.giants,
GulpSearch(giants=...), search -giants) against the NumPy restatement of the definition (tests/search_giants_ref.py).
The criterion is exact equality: every field of every giant, every label, every candidate, in order.  No tolerance
anywhere: the definition holds no floating-point arithmetic, only comparisons."""
import importlib
import os

import numpy as np
import pytest

import search_cutout_ref as CR
import search_giants_ref as R
import search_rfi_ref as P

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")
libpb = importlib.import_module("vlite-fast_amd.libpb")

FCH1 = 361.94
DEFAULT = dict(sep_time=3, sep_dm=200, sep_filter=3)


def _bits(a):
    return np.asarray(a, np.float32).view(np.int32)


def _assert_equal(got, ref, what):
    """got: Searcher.giants(..., want_list=True); ref: R.giants_ref(...)"""
    assert got["ngiants"] == ref["ngiants"] and got["overflow"] == ref["overflow"], (what, got["ngiants"], ref["ngiants"])
    gl, rg = got["giant_list"], ref["giants"]
    for k in R.GIANT_FIELDS:
        a, b = (_bits(gl[k]), _bits(rg[k])) if k == "snr" else (gl[k].astype(np.int64), rg[k])
        assert a.shape == b.shape and np.array_equal(a, b), (what, "giant", k)
    assert np.array_equal(gl["label"].astype(np.int64), ref["label"]), (what, "label")
    for k in R.CAND_FIELDS:
        a, b = (_bits(got[k]), _bits(ref["cands"][k])) if k == "snr" else (got[k].astype(np.int64), ref["cands"][k])
        assert a.shape == b.shape and np.array_equal(a, b), (what, "candidate", k)


def _check(s, snr, wl, thresh, t_lo=0, t_hi=None, what=None, **par):
    par = dict(dict(DEFAULT, max_giants=1 << 14), **par)
    s.set_giants(**par)
    got = s.giants(thresh, t_lo, t_hi, want_list=True)
    ref = R.giants_ref(snr, wl, thresh, t_lo, t_hi, **par)
    _assert_equal(got, ref, (what, thresh, t_lo, t_hi, par))
    return got


# ---- planes from real runs ----

# nbit, zap, list of trial DMs?, ndm, tout
RUNS = [(8, ((0, 3), (60, 64)), False, 24, 601),
        (4, ((10, 14),), True, 33, 1337),
        (2, (), False, 40, 2999)]


def _run_case(case):
    nbit, zap, use_list, ndm, tout = RUNS[case]
    nchan, foff = 64, -40.0 / 64
    dms = np.cumsum(np.linspace(0.7, 2.1, ndm)).astype(np.float32) if use_list else 1.5 * np.arange(ndm)
    delay = CR.delays(np.asarray(dms, np.float64), FCH1, foff, nchan, search.TSAMP)
    zapped = CR.zap_mask(nchan, zap)
    maxd = int(delay[:, ~zapped].max())
    T = tout + maxd
    rng = np.random.default_rng(70 + case)
    top = (1 << nbit) - 1
    x = rng.normal(top / 2.0, top / 6.0, (T, nchan))
    for k, (d, t0, amp, w) in enumerate([(3, 100, 0.25, 1), (ndm // 2, tout // 2, 0.2, 6), (ndm - 2, tout - 50, 0.15, 20)]):
        rows = t0 + delay[d][None, :] + np.arange(w)[:, None]
        x[rows, np.arange(nchan)[None, :]] += amp * top
    x = np.clip(np.rint(x), 0, top).astype(np.uint8)
    kw = dict(nchan=nchan, fch1=FCH1, foff=foff, tsamp=search.TSAMP, boxcar_max=64, zap=zap, max_samples=T)
    kw.update(dict(dm_list=dms) if use_list else dict(dm_min=0.0, dm_max=1.5 * (ndm - 1), dm_step=1.5))
    return kw, P.pack(x, nbit), nbit, ndm, tout


@pytest.mark.parametrize("case", range(len(RUNS)))
def test_real_planes_equal_the_restatement(case):
    kw, codes, nbit, ndm, tout = _run_case(case)
    with search.Searcher(**kw) as s:
        r = s.run(codes, nbit=nbit)
        snr, wl = r["snr"], r["width_log2"]
        assert s.ndm == ndm and r["tout"] == tout and tout % 64 != 0 and tout % 256 != 0
        v = np.sort(snr.ravel())
        few, many = float(v[-12]), float(v[int(0.80 * v.size)])
        g = _check(s, snr, wl, few, what="few")
        assert 1 <= g["ngiants"] <= 12
        _check(s, snr, wl, float(v[-200]), what="pulses", sep_time=5, sep_dm=3, sep_filter=1)
        g = _check(s, snr, wl, many, what="many")
        print("case %d: %d giants in %d clusters at S/N %.2f" % (case, g["ngiants"], len(g["snr"]), many))
        assert g["ngiants"] > 50 and len(g["snr"]) < g["ngiants"]        # (a fifth of the samples are hot)
        _check(s, snr, wl, many, what="many, tight", sep_time=1, sep_dm=2, sep_filter=0)
        _check(s, snr, wl, many, 77, tout - 129, what="many, a range", sep_time=64, sep_dm=1, sep_filter=8)
        # below every sample: one giant per series spanning the range; with sep_dm = 1 a chain through every series
        g = _check(s, snr, wl, float(v[0]) - 1.0, 5, tout - 3, what="all hot", sep_time=2, sep_dm=1, sep_filter=8)
        assert g["ngiants"] == ndm and np.all(g["giant_list"]["npts"] == tout - 8) and np.all(g["giant_list"]["label"] == 0)
        assert list(g["members"]) == [ndm] and g["npoints"][0] == ndm * (tout - 8) and (g["i0"][0], g["i1"][0]) == (5, tout - 3)
        assert g["snr"][0] == snr[:, 5:tout - 3].max()


# ---- hand-made planes through set_planes ----

NDM, TOUT = 8, 700


@pytest.fixture(scope="module")
def small():
    with search.Searcher(nchan=64, fch1=FCH1, foff=-40.0 / 64, tsamp=search.TSAMP, boxcar_max=16, zap=(), dm_min=0.0,
                         dm_max=7.0, dm_step=1.0, max_samples=2100) as s:
        assert s.ndm == NDM
        yield s


def _blank(tout=TOUT, ndm=NDM):
    return np.zeros((ndm, tout), np.float32), np.zeros((ndm, tout), np.uint8)


def _put(snr, wl, d, lo, hi, rng, base=10.0):
    """hot samples [lo, hi) in series d with distinct S/N and random widths"""
    snr[d, lo:hi] = base + rng.permutation(hi - lo).astype(np.float32)
    wl[d, lo:hi] = rng.integers(0, 5, hi - lo)


def test_runs_at_chunk_edges_and_range_ends(small):
    rng = np.random.default_rng(1)
    snr, wl = _blank()
    for d, (lo, hi) in enumerate([(60, 64), (64, 71), (65, 90), (250, 256), (250, 257), (257, 300), (63, 65), (255, 258)]):
        _put(snr, wl, d, lo, hi, rng)
    _put(snr, wl, 6, 0, 3, rng)
    _put(snr, wl, 7, TOUT - 3, TOUT, rng)
    _put(snr, wl, 0, 511, 513, rng)
    small.set_planes(snr, wl)
    for sep_time in (1, 3, 64):
        g = _check(small, snr, wl, 5.0, what="edges", sep_time=sep_time, sep_dm=0)
        assert g["ngiants"] == (11 if sep_time < 64 else 10)
        # the range cuts runs: at t_lo and at t_hi - 1
        _check(small, snr, wl, 5.0, 62, 256, what="cut", sep_time=sep_time, sep_dm=1)
        _check(small, snr, wl, 5.0, 64, 65, what="one sample", sep_time=sep_time)
        _check(small, snr, wl, 5.0, 1, TOUT - 1, what="ends", sep_time=sep_time)


@pytest.mark.parametrize("sep_time", [1, 3, 64])
def test_gaps_of_sep_time_and_one_more_across_a_chunk_boundary(small, sep_time):
    snr, wl = _blank()
    starts = [63, 64 - sep_time, 127, 128 - sep_time, 191 - sep_time // 2, 255, 256 - sep_time, 300]
    for d, a in enumerate(starts):
        a = max(a, 0)
        snr[d, a] = snr[d, a + sep_time] = 9.0                          # one giant: exactly sep_time apart
        b = 575 - d % (sep_time + 1)                                    # ... across sample 576
        snr[d, b] = snr[d, b + sep_time + 1] = 9.0                      # two giants: sep_time + 1 apart
        wl[d, a], wl[d, a + sep_time] = 1, 2
    small.set_planes(snr, wl)
    g = _check(small, snr, wl, 9.0, what="gaps", sep_time=sep_time, sep_dm=0)
    assert g["ngiants"] == 3 * NDM and sorted(g["giant_list"]["npts"]) == [1] * (2 * NDM) + [2] * NDM
    assert np.all(g["giant_list"]["tfilt"][::3] == 1)                   # equal S/N: the earlier sample is the peak


def test_a_snake_carries_its_label_the_whole_length(small):
    tout = 2000
    snr, wl = _blank(tout)
    n = 190
    zig = list(range(NDM)) + list(range(NDM - 2, 0, -1))
    for k in range(n):
        snr[zig[k % len(zig)], 10 * k + 5:10 * k + 13] = 6.0 + (k % 7)
    small.set_planes(snr, wl)
    g = _check(small, snr, wl, 6.0, what="snake", sep_time=3, sep_dm=1, sep_filter=0)
    assert g["ngiants"] == n and list(g["members"]) == [n] and np.all(g["giant_list"]["label"] == 0)
    assert small.giant_timers()["sweeps"] >= 2                          # one sweep that hooks, one that finds nothing to do
    # one sample more between neighbours and nothing is linked
    g = _check(small, snr, wl, 6.0, what="no snake", sep_time=2, sep_dm=1, sep_filter=0)
    assert len(g["members"]) == n
    small.set_planes(*_blank())


def test_ties_nan_inf_and_signed_zero(small):
    snr, wl = _blank()
    snr[:] = -5.0
    snr[1, 100:140] = 7.0                                               # equal inside a giant: the first sample
    snr[2, 120:130] = 7.0                                               # equal between members: the smaller index
    snr[3, 125:128] = 7.0
    wl[1, 100], wl[2, 120], wl[3, 125] = 2, 3, 4
    snr[5, 300:310] = [8, np.nan, 8, np.nan, np.nan, np.nan, np.nan, 9, np.inf, np.inf]
    snr[6, 300] = -np.inf
    snr[7, 400:404] = [-0.0, 0.0, -0.0, 0.0]
    small.set_planes(snr, wl)
    g = _check(small, snr, wl, 7.0, what="ties")
    assert g["ngiants"] == 5 and list(g["peak"]) == [100, 300, 308] and list(g["tfilt"]) == [2, 0, 0]
    assert list(g["members"]) == [3, 1, 1] and list(g["npoints"]) == [53, 2, 3]
    _check(small, snr, wl, 7.0, what="ties, no links", sep_dm=0)
    g = _check(small, snr, wl, -1.0, what="zeros")
    assert _bits(g["giant_list"]["snr"])[-1] == _bits(np.float32(-0.0)) and g["giant_list"]["peak"][-1] == 400
    _check(small, snr, wl, float("-inf"), what="everything but the NaN", sep_dm=1)
    g = _check(small, snr, wl, float("inf"), what="only the infinities")
    assert g["ngiants"] == 1 and g["npoints"][0] == 2


def test_empty_plane_and_the_overflow_rule(small):
    rng = np.random.default_rng(4)
    snr, wl = _blank()
    small.set_planes(snr, wl)
    g = _check(small, snr, wl, 1.0, what="empty")
    assert g["ngiants"] == 0 and len(g["snr"]) == 0 and not g["overflow"]
    snr[:, ::50] = 2.0 + rng.random((NDM, 14), dtype=np.float32)
    small.set_planes(snr, wl)
    G = 14 * NDM
    for cap in (G - 1, G, G + 1):
        g = _check(small, snr, wl, 1.0, what=("cap", cap), max_giants=cap, sep_dm=1)
        assert g["ngiants"] == G and g["overflow"] == (cap < G) and len(g["snr"]) == (0 if cap < G else 14)
        assert len(g["giant_list"]["dmi"]) == (0 if cap < G else G)


def test_a_short_range_after_a_long_one_and_repeatability(small):
    rng = np.random.default_rng(5)
    snr = rng.standard_normal((NDM, TOUT)).astype(np.float32)
    wl = rng.integers(0, 5, (NDM, TOUT)).astype(np.uint8)
    small.set_planes(snr, wl)
    a = _check(small, snr, wl, 0.5, what="long")
    _check(small, snr, wl, 0.5, 100, 164, what="short after long")
    _check(small, snr, wl, 2.5, 300, 310, what="shorter")
    b = _check(small, snr, wl, 0.5, what="long again")
    c = small.giants(0.5, want_list=True)
    for x, y in ((a, b), (b, c)):
        assert all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in R.CAND_FIELDS)
        assert all(x["giant_list"][k].tobytes() == y["giant_list"][k].tobytes() for k in x["giant_list"])


def test_refusals():
    kw = dict(nchan=64, fch1=FCH1, foff=-40.0 / 64, tsamp=search.TSAMP, boxcar_max=16, zap=(), dm_min=0.0, dm_max=7.0,
              dm_step=1.0, max_samples=1000)
    snr, wl = _blank()
    with search.Searcher(**kw) as s:
        with pytest.raises(libpb.PbError, match="set_giants"):
            s.giants(6.0, 0, 10)                                        # stage off
        s.set_giants()
        with pytest.raises(libpb.PbError, match="no block searched"):
            s.giants(6.0, 0, 10)                                        # no run yet
        for bad in (dict(sep_time=0), dict(sep_time=65), dict(sep_dm=-1), dict(sep_filter=-1), dict(max_giants=-1),
                    dict(max_giants=(1 << 22) + 1)):
            with pytest.raises(ValueError, match="pb_search_set_giants"):
                s.set_giants(**bad)
        assert s._gi == (3, 200, 3, 1 << 18)                            # nothing changed
        with pytest.raises(ValueError):
            s.set_planes(snr[:4], wl[:4])
        with pytest.raises(ValueError, match="tout"):
            s.set_planes(np.zeros((NDM, 1001), np.float32), np.zeros((NDM, 1001), np.uint8))
        snr[2, 10:20] = 8.0
        s.set_planes(snr, wl)
        for lo, hi in ((-1, 10), (10, 10), (20, 10), (0, TOUT + 1), (TOUT, TOUT + 1)):
            with pytest.raises(libpb.PbError, match="range"):
                s.giants(6.0, lo, hi)
        with pytest.raises(libpb.PbError, match="NaN"):
            s.giants(float("nan"))
        g = s.giants(6.0, want_list=True)                               # and the next call works
        assert g["ngiants"] == 1 and (g["i0"][0], g["i1"][0], g["npoints"][0]) == (10, 20, 10)
        s.set_giants(max_giants=0)
        with pytest.raises(libpb.PbError, match="set_giants"):
            s.giants(6.0)


def test_never_switched_on_changes_nothing():
    kw, codes, nbit, ndm, tout = _run_case(0)
    x = P.unpack(codes, kw["max_samples"], kw["nchan"], nbit)

    def go(touch):
        with search.Searcher(**kw) as s:
            if touch:                                                   # on and off again: the default path is as it was
                s.set_giants()
                s.set_giants(max_giants=0)
            pk = s.peaks(x, 5.0)
            rows = np.stack([pk["dmi"], pk["t"], pk["snr"].view(np.int32), pk["width_log2"].astype(np.int32)], axis=1)
            g = search.GulpSearch(s, threshold=5.0)
            cands = g.push(x) + g.finish()
        return rows[np.lexsort(rows.T[::-1])].tobytes(), [search.candidate_line(c) for c in cands]

    plain, touched = go(False), go(True)
    assert plain == touched and len(plain[1]) >= 1


def test_gulp_search_with_giants_on_a_small_stream():
    """push() + finish() cover every output sample once: the candidates are the restatement's on [0, nout) and
    [nout, tout) of the block's planes"""
    kw, codes, nbit, ndm, tout = _run_case(0)
    x = P.unpack(codes, kw["max_samples"], kw["nchan"], nbit)
    par = dict(sep_time=3, sep_dm=4, sep_filter=3, max_giants=4096)
    with search.Searcher(**kw) as s:
        r = s.run(x)
        g = search.GulpSearch(s, threshold=5.0, giants=par)
        got = g.push(x), g.finish()
        dms = s.dms
    nout = tout - 63
    for cands, (lo, hi) in zip(got, ((0, nout), (nout, tout))):
        ref = R.sort_strongest_first(R.giants_ref(r["snr"], r["width_log2"], 5.0, lo, hi, **par)["cands"])
        assert len(cands) == len(ref["snr"]) >= 1
        for i, c in enumerate(cands):
            assert (np.float32(c["snr"]), c["peak_idx"], c["tfilt"], c["dmi"], c["ngiant"], c["npoints"], c["i0"], c["i1"]) == (
                ref["snr"][i], ref["peak"][i], ref["tfilt"][i], ref["dmi"][i], ref["members"][i], ref["npoints"][i],
                ref["i0"][i], ref["i1"][i])
            assert c["dm"] == float(dms[c["dmi"]]) and len(search.candidate_line(c).split()) == 9
    # a gulp with more giants than max_giants is given up
    with search.Searcher(**kw) as s:
        g = search.GulpSearch(s, threshold=1.0, giants=dict(max_giants=16))
        assert g.push(x) == []


# ---- the workload's own shape, once ----

def test_production_geometry_pulse_across_a_gulp_boundary(tmp_path, capsys):
    sig = importlib.import_module("vlite-fast_amd.sigproc")
    nchan, gulp, ngulp = 4096, search.HEIMDALL_GULP, 3
    dm, t0, width = 500.0, 58000, 4                      # the sweep (~5690 samples) crosses sample 61 440
    fch1, foff, tsamp = float(np.float32(search.FCH1)), float(np.float32(search.FOFF)), float(np.float32(search.TSAMP))
    dml = search.dedisp_dm_list(2.0, 1000.0, tsamp, fch1, foff, nchan)
    rng = np.random.default_rng(53)
    stream = np.empty((ngulp * gulp, nchan), np.uint8)
    for i in range(0, stream.shape[0], 3072):
        g = rng.standard_normal((3072, nchan), dtype=np.float32)
        stream[i:i + 3072] = np.clip(np.floor(g / np.float32(0.02957) + np.float32(127.5)), 0, 255).astype(np.uint8)
    sweep = CR.delays([dm], fch1, foff, nchan, tsamp)[0]
    assert t0 + sweep[190] < 2 * gulp < t0 + sweep[3899]
    rows = t0 + sweep[None, :] + np.arange(width)[:, None]
    cols = np.broadcast_to(np.arange(nchan), rows.shape)
    stream[rows, cols] = np.clip(stream[rows, cols].astype(np.int32) + 12, 0, 255).astype(np.uint8)     # + 0.35 sigma
    hdr = b"".join([sig.send_string("HEADER_START"), sig.send_int("data_type", 1), sig.send_double("fch1", fch1),
                    sig.send_double("foff", foff), sig.send_int("nchans", nchan), sig.send_int("nbits", 8),
                    sig.send_double("tstart", 57570 + 3600 / 86400.), sig.send_double("tsamp", tsamp),
                    sig.send_int("nifs", 1), sig.send_string("HEADER_END")])
    fil = tmp_path / "gulps.fil"
    with open(fil, "wb") as f:
        f.write(hdr)
        f.write(stream.tobytes())
    maxs = gulp + int(4.148808e3 * 1000.0 * abs((fch1 + (nchan - 1) * foff) ** -2 - fch1 ** -2) / tsamp) + 64

    def go(giants):
        out = []
        with search.Searcher(max_samples=maxs, fch1=fch1, foff=foff, tsamp=tsamp, dm_list=dml) as s:
            s.set_baseline(int(2.0 / tsamp))
            g = search.GulpSearch(s, threshold=7.0, giants=giants)
            for k in range(ngulp + 1):
                out += g.push(stream[k * gulp:(k + 1) * gulp]) if k < ngulp else g.finish()
            tm = s.giant_timers() if giants is not None else None
        return out, tm

    host, _ = go(None)
    dev, tm = go({})
    key = lambda c: (-c["snr"], c["dmi"], c["peak_idx"])
    a, b = min(host, key=key), min(dev, key=key)
    print("host %d candidates, device %d; strongest %s; last call %s" % (len(host), len(dev), search.candidate_line(b), tm))
    assert (np.float32(a["snr"]), a["dmi"], a["peak_idx"], a["tfilt"]) == (np.float32(b["snr"]), b["dmi"], b["peak_idx"], b["tfilt"])
    assert abs(b["dm"] - dm) < 10 and abs(b["peak_idx"] - t0) <= 4 and b["ngiant"] > 1
    # the pulse is one candidate, not several
    near = [c for c in dev if abs(c["peak_idx"] - t0) <= 64 and abs(c["dm"] - dm) <= 100]
    assert len(near) == 1, [search.candidate_line(c) for c in near]
    # the command line: the same lines; cutouts and refinement attach to the pulse
    out = tmp_path / "cands"
    capsys.readouterr()
    n = search.main(["-f", str(fil), "-detect_thresh", "7", "-zap_chans", "0", "190", "-zap_chans", "3900", "4096", "-giants",
                     "-output_dir", str(out), "-cutouts", "-cutout_thresh", "10", "-refine", "-refine_thresh", "10"])
    printed = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert n == len(printed) == len(dev) and printed == [search.candidate_line(c) for c in dev]
    cand = [p for p in os.listdir(out) if p.endswith(".cand") and search.candidate_line(b) in open(out / p).read().splitlines()]
    assert len(cand) == 1
    stem = cand[0][:-len(".cand")]
    z = np.load(out / (stem + ".cutouts.npz"))
    assert b["peak_idx"] in list(z["peak_idx"]) and z["ft"].shape[1:] == (64, 256)
    rl = [l.split() for l in open(out / (stem + ".refined")).read().splitlines()]
    mine = [t for t in rl if " ".join(t[:9]) == " ".join(search.candidate_line(b).split())]
    assert len(mine) == 1 and len(mine[0]) == 13
