"""The search's normalisation on the GPU (k_prefix, k_series_stats, baseline_at, k_boxcar of csrc/search_run.hip) against
the restatement of its definition (include/pb_hip.h under pb_search_set_baseline; tests/search_stats_ref.py, exact
integer sums and float64 planes; held to independent answers by tests/test_search_stats_cpu.py).

Every case first checks the integer series against oracle.dedisperse_series, so a red statistic is the statistic's.
Tolerances: rms 1 binary32 ulp; level 1 ulp + the summation bound tout 2^-52 mean|v|; planes the np.spacing-derived
bound of search_stats_ref.boxcar_all (from the REFERENCE's level and rms, widened by the first-order effect of that
1-ulp freedom); widths equal except at near-ties of the float64 S/N, whose share the reference itself must keep under
1e-3.  Every case asserts that the reference finds no sample on the clip's rounding boundary (n_boundary == 0): the
seeds were chosen for that on the CPU."""
import importlib

import numpy as np
import pytest

import search_rfi_ref as R
import search_stats_ref as S

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")

F32 = np.float32
TSAMP = float(F32(search.TSAMP))
TIE_CAP = 1e-3

# (tout, W, nchan, nbit, input, boxcar_max); W: samples, or "tout" / "tout+9".  Every tout, W, input and boxcar_max of
# the list occurs at least twice; tout covers the partial strides of the 256-lane loops and of k_prefix's split.
CASES = [
    (64, 63, 64, 8, "noise", 1),
    (64, "tout", 256, 8, "drift", 16),
    (71, 1, 64, 8, "noise", 16),
    (71, "tout+9", 256, 8, "pulse", 64),
    (255, 2, 64, 8, "pulse", 16),
    (255, 63, 256, 4, "noise", 64),
    (256, 0, 256, 8, "const", 16),
    (256, 512, 64, 2, "noise", 1),
    (257, 0, 64, 8, "spike", 16),
    (257, 2, 256, 8, "drift", 64),
    (2048, 2560, 256, 8, "pulse", 64),
    (2048, 512, 64, 8, "drift", 16),
    (2056, "tout", 64, 8, "pulse", 1),
    (2056, 1, 256, 8, "drift", 64),
    (3000, 2560, 256, 8, "noise", 16),
    (3000, "tout+9", 64, 8, "const", 64),
    (3000, 0, 64, 8, "spike", 16),
    (2048, 0, 256, 8, "pulse", 64),
]
# the reference's rms is exactly 0 for these: a constant block, a block that is 0 but for one sample (the clip leaves
# a constant), W = 1 (the baseline is the sample).  Their planes are test_rms_zero's.
RMS_ZERO = [i for i, c in enumerate(CASES) if c[4] in ("const", "spike") or c[1] == 1]
RMS_POS = [i for i in range(len(CASES)) if i not in RMS_ZERO]


def _window(W, tout):
    return {"tout": tout, "tout+9": tout + 9}.get(W, W)


def _band(nchan, ascending=False):
    """(fch1, foff) rounded to binary32 as the C interface carries them (include/pb_hip.h)"""
    foff = float(F32(41.0 / nchan))
    if ascending:
        return float(F32(361.94 - 41.0)), foff
    return float(F32(361.94)), -foff


def _delays(oracle, dms, fch1, foff, nchan):
    return oracle.search_delays(dms, fch1, foff, nchan, TSAMP)


def _codes(kind, seed, T, nchan, nbit, delay20, tout):
    """[T][nchan] codes of nbit bits.  noise: Gaussian about mid-range (sigma 33.8 codes at 8 bits, as sel_and_dig_8b
    makes of unit-variance data); drift: + a 12-code sinusoid; pulse: + a strong 4-sample pulse dispersed with delay20
    and a 40-sample broadband burst; const: every code 100; spike: 0 but for one sample of one channel."""
    top = (1 << nbit) - 1
    if kind == "const":
        return np.full((T, nchan), min(100, top), np.uint8)
    if kind == "spike":
        x = np.zeros((T, nchan), np.uint8)
        x[tout // 2 + 3, nchan // 3] = top
        return x
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((T, nchan)) * (33.8 * top / 255.0) + top / 2.0
    if kind == "drift":
        g += 12.0 * np.sin(2 * np.pi * np.arange(T) / 1500.0 + 0.4)[:, None]
    if kind == "pulse":
        t0 = tout // 3
        for c in range(nchan):
            g[t0 + delay20[c]:t0 + delay20[c] + 4, c] += 40.0
        g[tout // 2:tout // 2 + 40] += 12.0
    return np.clip(np.floor(g + 0.5), 0, top).astype(np.uint8)


def _run_case(oracle, tout, W, nchan, nbit, kind, boxcar_max, seed, ascending=False, thresh=None, max_out=None):
    """one block through search.Searcher -> dict(r, series (checked exact), W, nbox, ndm, codes, peaks?)"""
    fch1, foff = _band(nchan, ascending)
    dms = 10.0 * np.arange(5)
    delays = _delays(oracle, dms, fch1, foff, nchan)
    maxd = int(delays.max())
    T = tout + maxd
    x = _codes(kind, seed, T, nchan, nbit, delays[2], tout)
    W = _window(W, tout)
    out = dict(W=W, ndm=dms.size, tout=tout)
    with search.Searcher(nchan=nchan, max_samples=T, fch1=fch1, foff=foff, tsamp=TSAMP, dm_min=0.0, dm_max=40.0,
                         dm_step=10.0, boxcar_max=boxcar_max, zap=()) as s:
        assert s.max_delay == maxd and s.ndm == dms.size
        s.set_baseline(W)
        packed = R.pack(x, nbit)
        r = s.run(packed, nbit=nbit, want_series=True)
        out["nbox"] = s.nbox
        if thresh is not None:
            out["peaks"] = [s.peaks(packed, th, nbit=nbit, **({} if max_out is None else dict(max_out=max_out)))
                            for th in thresh]
    ref, t_ref = oracle.dedisperse_series(x, delays, np.zeros(nchan, bool))
    assert t_ref == tout == r["tout"]
    assert np.array_equal(r["series"], ref), "dedispersed series differ: not a statistics finding"
    out["r"] = r
    out["series"] = ref.astype(np.int64)
    return out


def _check_stats(series, stats, W, what):
    """(a): every series' level and rms against the exact restatement -> [(level, rms, level tolerance)] per series"""
    refs, nbs = [], []
    for i, x in enumerate(series):
        lvl, rms, nb = S.series_stats(x, W)
        tol = S.level_tolerance(x, W, lvl)
        print("%s dm %d: level %.9g (ref %.9g, tol %.3g)  rms %.9g (ref %.9g, ulp %.3g)  n_boundary %d" % (
            what, i, stats[i, 0], lvl, tol, stats[i, 1], rms, np.spacing(rms), nb))
        refs.append((lvl, rms, tol))
        nbs.append(nb)
    for i, (lvl, rms, tol) in enumerate(refs):
        assert nbs[i] == 0, (what, i)                                   # a condition on the input, not a measurement
        assert abs(float(stats[i, 1]) - float(rms)) <= float(np.spacing(rms)), (what, i, stats[i, 1], rms)
        assert abs(float(stats[i, 0]) - float(lvl)) <= tol, (what, i, stats[i, 0], lvl, tol)
    return refs


def _check_planes(series, r, refs, W, nbox, what):
    """(b): S/N and width planes against float64 from the reference's own level and rms"""
    for i, x in enumerate(series):
        lvl, rms, tol = refs[i]
        assert float(rms) > 0
        sn, err = S.boxcar_all(x, lvl, rms, nbox, W, dlevel=tol, drms=float(np.spacing(rms)))
        c = S.compare_planes(r["snr"][i], r["width_log2"][i], sn, err)
        print("%s dm %d: worst |snr - ref| - bound %.3g (largest bound %.3g), near-ties %d of %d, widths off %d" % (
            what, i, c["excess"].max(), np.nanmax(err), c["tie"].sum(), x.size, (~c["width_ok"]).sum()))
        assert c["tie"].mean() <= TIE_CAP, (what, i)                    # a condition on the input
        assert c["width_ok"].all(), (what, i, np.nonzero(~c["width_ok"])[0][:8])
        assert np.array_equal(r["width_log2"][i][~c["tie"]], c["bw"][~c["tie"]]), (what, i)
        assert c["value_ok"].all(), (what, i, float(c["excess"].max()))
        # where a series ends only the widths that fit are tried
        wfit = np.floor(np.log2(np.minimum(x.size - np.arange(x.size), 1 << (nbox - 1)))).astype(int)
        assert np.all(r["width_log2"][i] <= wfit), (what, i)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_level_and_rms_of_every_trial_dm(oracle, case):
    tout, W, nchan, nbit, kind, boxcar_max = CASES[case]
    o = _run_case(oracle, tout, W, nchan, nbit, kind, boxcar_max, seed=7000 + case)
    refs = _check_stats(o["series"], o["r"]["stats"], o["W"], "case %d" % case)
    assert all((float(rms) == 0) == (case in RMS_ZERO) for _, rms, _ in refs)


@pytest.mark.parametrize("case", RMS_POS)
def test_planes_from_the_reference_statistics(oracle, case):
    tout, W, nchan, nbit, kind, boxcar_max = CASES[case]
    o = _run_case(oracle, tout, W, nchan, nbit, kind, boxcar_max, seed=7000 + case)
    refs = []
    for x in o["series"]:
        lvl, rms, nb = S.series_stats(x, o["W"])
        assert nb == 0
        refs.append((lvl, rms, S.level_tolerance(x, o["W"], lvl)))
    _check_planes(o["series"], o["r"], refs, o["W"], o["nbox"], "case %d" % case)


@pytest.mark.parametrize("case", RMS_ZERO)
def test_rms_zero(oracle, case):
    """(d) rms not positive: S/N 0 at every point, the width the definition's (the narrowest width with a positive
    numerator, else 0; the numerators here are integers below 2^24, exact in binary32, so nothing is ambiguous),
    no peak above a positive threshold and every point at threshold 0."""
    tout, W, nchan, nbit, kind, boxcar_max = CASES[case]
    o = _run_case(oracle, tout, W, nchan, nbit, kind, boxcar_max, seed=7000 + case, thresh=(1e-30, 0.0))
    r = o["r"]
    assert not r["stats"][:, 1].any()
    assert not r["snr"].any() and r["snr"].dtype == F32
    for i, x in enumerate(o["series"]):
        lvl = r["stats"][i, 0]
        if kind == "spike":
            # the exact level is 0 and the kernel's may be a rounding error of either sign, which decides the sign of
            # every numerator without the spike in it: only the points no such error can change are compared
            lvl = S.series_stats(x, o["W"])[0]
            num, e = S.boxcar_all(x, lvl, 0, o["nbox"], o["W"], dlevel=S.level_tolerance(x, o["W"], lvl))
            sure = ~np.any(np.abs(num) <= e, axis=0)
        else:
            assert int(x.max()) << (o["nbox"] - 1) < 2 ** 24
            sure = np.ones(x.size, bool)
        best, bw, _ = S.boxcar_planes(x, lvl, 0, o["nbox"], o["W"])
        assert not best.any() and sure.any() and (kind == "spike" or sure.all()), (case, i)
        assert np.array_equal(r["width_log2"][i][sure], bw[sure]), (case, i)
    above, at_zero = o["peaks"]
    assert above["total"] == 0 and above["dmi"].size == 0
    assert at_zero["total"] == o["ndm"] * tout


def test_truncated_peak_list(oracle):
    """(e) fewer rows asked for than there are points: the total is the thresholded plane's count, exactly max_out
    rows come back, each a distinct point of the thresholded plane with its S/N bits and width"""
    k, thr = 100, 1.5
    o = _run_case(oracle, 3000, 512, 256, 8, "pulse", 16, seed=7100, thresh=(thr,), max_out=k)
    r, pk = o["r"], o["peaks"][0]
    idm, it = np.nonzero(r["snr"] >= F32(thr))
    assert idm.size > 10 * k and pk["total"] == idm.size
    assert pk["dmi"].size == pk["t"].size == pk["snr"].size == pk["width_log2"].size == k
    pts = set(zip(pk["dmi"].tolist(), pk["t"].tolist()))
    assert len(pts) == k and pts <= set(zip(idm.tolist(), it.tolist()))
    assert np.array_equal(pk["snr"].view(np.int32), r["snr"][pk["dmi"], pk["t"]].view(np.int32))
    assert np.array_equal(pk["width_log2"], r["width_log2"][pk["dmi"], pk["t"]])


@pytest.mark.parametrize("W,boxcar_max", [(0, 16), (512, 64)])
def test_ascending_band(oracle, W, boxcar_max):
    """(f) foff > 0: the reference frequency is the LAST channel's.  Series exact, (a) and (b) hold."""
    fch1, foff = _band(256, ascending=True)
    d = _delays(oracle, [20.0], fch1, foff, 256)[0]
    assert foff > 0 and d[-1] == 0 and d[0] == d.max() > 100 and np.all(np.diff(d) <= 0)
    o = _run_case(oracle, 2056, W, 256, 8, "pulse", boxcar_max, seed=7200 + W, ascending=True)
    refs = _check_stats(o["series"], o["r"]["stats"], o["W"], "ascending W %d" % W)
    _check_planes(o["series"], o["r"], refs, o["W"], o["nbox"], "ascending W %d" % W)
    k = np.unravel_index(np.argmax(o["r"]["snr"][:, :900]), (o["ndm"], 900))
    assert k[0] == 2 and abs(k[1] - 2056 // 3) <= 4                       # the pulse, at DM 20 and its time


def test_production_scale(oracle):
    """(c) 4096 channels with heimdall's zapped edges, a 30 720-sample gulp, the 2-s baseline, widths to 64, noise at
    the level of the production chain's 8-bit output plus a DM-300 pulse; DM 0, 50 .. 1000.  A 64-sample sum is 3.1e7,
    above 2^24: the binary32 operands of k_boxcar are rounded before they cancel, and the bound says by how much."""
    nchan, T, W = 4096, search.HEIMDALL_GULP, 2560
    fch1, foff = float(F32(search.FCH1)), float(F32(search.FOFF))
    dms = 50.0 * np.arange(21)
    delays = _delays(oracle, dms, fch1, foff, nchan)
    zmask = np.zeros(nchan, bool)
    for lo, hi in search.HEIMDALL_ZAP:
        zmask[lo:hi] = True
    rng = np.random.default_rng(7300)
    x = rng.standard_normal((T, nchan), dtype=np.float32)
    t0 = 4000
    rows = t0 + delays[6][None, :] + np.arange(4)[:, None]
    x[rows, np.broadcast_to(np.arange(nchan), rows.shape)] += 0.35
    x = np.clip(np.floor(x / F32(0.02957) + F32(127.5)), 0, 255).astype(np.uint8)
    with search.Searcher(max_samples=T, fch1=fch1, foff=foff, tsamp=TSAMP, dm_min=0.0, dm_max=1000.0, dm_step=50.0) as s:
        assert s.ndm == 21 and s.nbox == 7 and s.max_delay == int(delays[:, ~zmask].max())
        s.set_baseline(W)
        r = s.run(x, want_series=True)
        print("stage ms:", s.timers())
    ref, tout = oracle.dedisperse_series(x, delays, zmask)
    assert tout == r["tout"] and np.array_equal(r["series"], ref)
    ref = ref.astype(np.int64)
    assert ref[0][:64].sum() > 2 ** 24
    refs = _check_stats(ref, r["stats"], W, "production")
    _check_planes(ref, r, refs, W, 7, "production")
    k = np.unravel_index(np.argmax(r["snr"]), r["snr"].shape)
    assert k[0] == 6 and abs(k[1] - t0) <= 4 and r["snr"][k] > 10
