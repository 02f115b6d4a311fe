"""The refinement of a candidate's DM, width and S/N on the GPU (pb_search_set_refine / pb_search_refine,
Searcher.refine_raw / refine, GulpSearch(refine=...), search -refine) against the NumPy restatement of its definition
(tests/search_refine_ref.py, held to the reference's own refine_dm / optimize_pulse by tests/test_search_refine_cpu.py).
The restatement is fed the block the search saw (pb_search_fetch_clean).  The fine series are compared element for
element, status / kbest / opt_loc for equality, the S/N to search_refine_ref.sn_bound (the rounding of the float64
operands).  kbest (and the width pass that hangs on it) may be left out only where the restatement's two best S/N lie
within that bound of each other: at most 1 % of the requests, which tests/test_search_refine_cpu.py asserts for these
seeded inputs from the restatement alone."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import search_refine_cases as K
import search_refine_ref as R
import search_rfi_ref as P

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")
libpb = importlib.import_module("vlite-fast_amd.libpb")
EINVAL = -22


def _compare(got, ref, what):
    """one refine_raw() result against the restatement's list -> number of near-ties left out"""
    ties = 0
    for i, r in enumerate(ref):
        w = (what, i)
        assert np.array_equal(got["series"][i].astype(np.int64), r["series"]), w
        assert got["status"][i] == r["status"], w
        assert np.array_equal(np.isnan(got["sn_dm"][i]), np.isnan(r["sn_dm"])), w
        ok = ~np.isnan(r["sn_dm"])
        d = np.abs(got["sn_dm"][i][ok] - r["sn_dm"][ok])
        print("%s request %d: worst |sn_dm - ref| %.3g (bound %.3g), kbest %d (ref %d)%s" % (
            what, i, d.max() if d.size else 0, r["err_dm"][ok].max() if d.size else 0, got["kbest"][i], r["kbest"],
            " near-tie" if r["near_tie"] else ""))
        assert np.all(d <= r["err_dm"][ok]), w
        if r["near_tie"]:
            ties += 1
            continue
        assert got["kbest"][i] == r["kbest"], w
        assert np.array_equal(got["opt_loc"][i], r["opt_loc"]), w
        if r["kbest"] < 0:
            assert np.isnan(got["opt_sn"][i]).all(), w
        else:
            assert np.all(np.abs(got["opt_sn"][i] - r["opt_sn"]) <= r["err_opt"]), w
    return ties


def _run_case(case):
    """one case on the GPU and through the restatement -> dict(got, one, ref, second: the pulse request's series from a
    second searcher that has the fine trials as its DM list)"""
    nbit, nchan, zap, use_list, _, (nstep, H, wmax), clean = K.CASES[case]
    kw, dms, zapped, maxd = K.geometry(case)
    tout, T = K.length(case)
    x = K.codes(case, T)
    reqs = K.requests(case, dms)
    with search.Searcher(max_samples=T + 100, **kw) as s:
        assert s.max_delay == maxd and T % 64 != 0
        if clean:
            s.set_rfi(True, True)
        s.set_refine(nstep=nstep, half_window=H, wmax=wmax, max_cands=len(reqs))
        assert s.run(P.pack(x, nbit), nbit=nbit)["tout"] == tout
        xt = s.fetch_clean()
        assert clean == (not np.array_equal(xt, x.T))
        got = s.refine_raw(*zip(*reqs), want_series=True)                # n = max_cands
        one = s.refine_raw(*reqs[2], want_series=True)                   # n = 1, scalars
        print("case %d device ms:" % case, s.refine_timers())
    ref = K.restate(case, xt, tout, dms)
    # the pulse's request once more through the search itself: its fine trials as a second searcher's DM list
    t, w, lo, st = reqs[2]
    fine = R.trial_dms(lo, st, nstep)
    assert np.array_equal(fine.astype(np.float32).astype(np.float64), fine) and ref[2]["valid"].all()
    kw2 = {k: v for k, v in kw.items() if k not in ("dm_list", "dm_min", "dm_max", "dm_step")}
    with search.Searcher(max_samples=T + 100, dm_list=fine.astype(np.float32), **kw2) as s2:
        if clean:
            s2.set_rfi(True, True)
        r2 = s2.run(P.pack(x, nbit), nbit=nbit, want_series=True)
    assert r2["tout"] >= tout
    second = R.series_window(r2["series"][:, :tout].astype(np.int64), t, H, wmax // 2)
    return dict(got=got, one=one, ref=ref, second=second)


@pytest.fixture(scope="module")
def runs():
    """every case once, whichever tests of this module are selected and in whatever order"""
    return [_run_case(case) for case in range(len(K.CASES))]


@pytest.mark.parametrize("case", range(len(K.CASES)))
def test_refinement_equals_the_restatement(runs, case):
    o = runs[case]
    ref = o["ref"]
    assert any(r["status"] == 1 for r in ref) == (case == 1)
    assert any(np.isnan(r["sn_dm"]).any() and r["kbest"] >= 0 for r in ref) and any(r["kbest"] < 0 and not r["status"] for r in ref)
    _compare(o["got"], ref, "case %d" % case)
    _compare(o["one"], ref[2:3], "case %d, n = 1" % case)
    assert np.array_equal(o["second"], o["got"]["series"][2])


def test_near_ties_left_out_stay_under_the_cap(runs):
    ties = sum(r["near_tie"] for o in runs for r in o["ref"])
    total = sum(len(o["ref"]) for o in runs)
    print("near-ties left out of the index comparison: %d of %d requests" % (ties, total))
    assert ties <= K.NEAR_TIE_CAP * total


def test_a_shorter_block_after_a_long_one_does_not_read_stale_samples():
    kw, dms, zapped, maxd = K.geometry(2)
    nchan, nstep, H, wmax = 200, 8, 64, 16
    rng = np.random.default_rng(51)
    x1 = rng.integers(1, 4, (4000, nchan)).astype(np.uint8)              # no zero: stale bytes would add something
    x2 = rng.integers(1, 4, (maxd + 331, nchan)).astype(np.uint8)
    tout = 331
    reqs = [(tout - 1, 3, 30.0, 0.125), (tout - 70, 2, 39.0, 0.125), (0, 1, 0.0, 0.5)]
    with search.Searcher(max_samples=4000, **kw) as s:
        s.set_refine(nstep=nstep, half_window=H, wmax=wmax, max_cands=4)
        s.run(P.pack(x1, 2), nbit=2)
        assert s.run(P.pack(x2, 2), nbit=2)["tout"] == tout
        got = s.refine_raw(*zip(*reqs), want_series=True)
    chans = np.nonzero(~zapped)[0]
    for i, (t, w, lo, st) in enumerate(reqs):
        fine = R.trial_dms(lo, st, nstep)
        valid = (fine >= 0) & (fine <= dms[-1])
        q = R.fine_series(x2.T, chans, K.delays(np.where(valid, fine, 0.0), K.FCH1, kw["foff"], nchan), tout)
        q[~valid] = 0
        r = R.refine(q, valid, t, w, H, wmax)
        r["series"] = R.series_window(q, t, H, wmax // 2)
        _compare({k: v[i:i + 1] for k, v in got.items() if k in ("series", "status", "sn_dm", "kbest", "opt_sn", "opt_loc")},
                 [r], "short block %d" % i)


def _raw_call(s, ri, rf, n=None, nstep=8, nw=8, L=160):
    """pb_search_refine with sentinel-filled outputs -> (rc, message, outputs untouched)"""
    ri, rf = np.ascontiguousarray(ri, np.int32), np.ascontiguousarray(rf, np.float32)
    m = ri.shape[0]
    outs = [np.full(m, 0x5EADBEEF, np.int32), np.full((m, nstep), -7.25), np.full(m, 0x5EADBEEF, np.int32),
            np.full((m, nw), -7.25), np.full((m, nw), 0x5EADBEEF, np.int32), np.full((m, nstep, L), 0xDEADBEEF, np.uint32)]
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rc = s._L.pb_search_refine(s._s, ri.ctypes.data_as(i32p), rf.ctypes.data_as(C.POINTER(C.c_float)), m if n is None else n,
                               outs[0].ctypes.data_as(i32p), outs[1].ctypes.data_as(f64p), outs[2].ctypes.data_as(i32p),
                               outs[3].ctypes.data_as(f64p), outs[4].ctypes.data_as(i32p),
                               outs[5].ctypes.data_as(C.POINTER(C.c_uint32)))
    clean = all(np.all(o == v) for o, v in zip(outs, (0x5EADBEEF, -7.25, 0x5EADBEEF, -7.25, 0x5EADBEEF, 0xDEADBEEF)))
    return rc, s._L.pb_search_last_error(s._s).decode(), clean


def test_refusals_leave_the_outputs_alone_and_the_next_call_works():
    kw, dms, zapped, maxd = K.geometry(0)
    T = 2048
    x = np.random.default_rng(52).integers(0, 256, (T, 64)).astype(np.uint8)
    good_i, good_f = [(500, 3)], [(8.0, 0.125)]
    with search.Searcher(max_samples=T, **kw) as s:
        rc, msg, clean = _raw_call(s, good_i, good_f)
        assert rc == EINVAL and "not switched on" in msg and clean              # before set_refine
        with pytest.raises(libpb.PbError, match="set_refine"):
            s.refine_raw(500, 3, 8.0, 0.125)
        base = dict(nstep=8, half_window=64, wmax=16, max_cands=4)
        for bad in (dict(nstep=0), dict(nstep=5000), dict(wmax=15), dict(wmax=0), dict(wmax=66), dict(half_window=31),
                    dict(half_window=1020), dict(max_cands=-1)):
            with pytest.raises(ValueError, match="pb_search_set_refine"):
                s.set_refine(**dict(base, **bad))
            assert _raw_call(s, good_i, good_f)[0] == EINVAL and s._ref is None
        s.set_refine(**base)
        rc, msg, clean = _raw_call(s, good_i, good_f)
        assert rc == EINVAL and "no block searched" in msg and clean            # before any run
        tout = s.run(x)["tout"]
        rc, msg, clean = _raw_call(s, good_i * 5, good_f * 5)
        assert rc == EINVAL and "max_cands" in msg and clean                    # n > max_cands
        for bi, bf in (((tout, 3), (8.0, 0.125)), ((-1, 3), (8.0, 0.125)), ((500, 0), (8.0, 0.125)), ((500, 17), (8.0, 0.125)),
                       ((500, 3), (np.nan, 0.125)), ((500, 3), (8.0, np.inf))):
            rc, msg, clean = _raw_call(s, good_i + [bi], good_f + [bf])
            assert rc == EINVAL and "request 1 out of range" in msg and clean, (bi, bf)
        with pytest.raises(ValueError):
            s.set_refine(**dict(base, wmax=7))                                  # refused: the geometry stays
        rc, msg, clean = _raw_call(s, good_i, good_f, n=0)
        assert rc == 0 and clean                                                # no request: nothing to do
        got = s.refine_raw(500, 3, 8.0, 0.125, want_series=True)                # the next valid call works
        xt = s.fetch_clean()
        fine = R.trial_dms(8.0, 0.125, 8)
        q = R.fine_series(xt, np.arange(64), K.delays(fine, K.FCH1, kw["foff"], 64), tout)
        r = R.refine(q, np.ones(8, bool), 500, 3, 64, 16)
        r["series"] = R.series_window(q, 500, 64, 8)
        _compare(got, [r], "after refusals")
        s.set_refine(max_cands=0)                                               # off again
        rc, msg, clean = _raw_call(s, good_i, good_f)
        assert rc == EINVAL and "not switched on" in msg and clean


def _same_refinement(r, ref, peak_offset=0):
    """a Searcher.refine entry against search_refine_cases.two_pass's"""
    assert (r["dm"], r["width"], r["peak"] - peak_offset) == (ref["dm"], ref["width"], ref["peak"])
    assert abs(r["snr"] - ref["snr"]) <= ref["snr_err"]
    assert np.array_equal(r["opt_loc"], ref["opt_loc"])
    for p in range(2):
        dms, sns, err = ref["trials"][p]
        assert np.array_equal(r["trials"][p][0], dms) and np.array_equal(np.isnan(r["trials"][p][1]), np.isnan(sns))
        ok = ~np.isnan(sns)
        assert np.all(np.abs(r["trials"][p][1][ok] - sns[ok]) <= err[ok])


def test_never_switched_on_changes_nothing():
    x, kw, dms, dm_true, t0, tout = K.offgrid_inputs()

    def go(refine_on, hook):
        direct = None
        with search.Searcher(max_samples=x.shape[0], **kw) as s:
            if refine_on:
                s.set_refine(max_cands=8)
            pk = s.peaks(x, 6.0)
            rows = np.stack([pk["dmi"], pk["t"], pk["snr"].view(np.int32), pk["width_log2"].astype(np.int32)], axis=1)
            g = search.GulpSearch(s, threshold=6.0, refine=dict(thresh=6.0) if hook else None)
            cands = g.push(x)
            if hook:
                direct = s.refine(4, t0, 1)          # the inputs tests/test_search_refine_cpu.py proves sound
            cands = cands + g.finish()
        return rows[np.lexsort(rows.T[::-1])].tobytes(), [search.candidate_line(c) for c in cands], cands, direct

    plain, on, hooked = go(False, False), go(True, False), go(True, True)
    assert plain[0] == on[0] == hooked[0] and plain[1] == on[1] == hooked[1] and len(plain[1]) >= 1
    assert all("refined" not in c for c in plain[2] + on[2]) and any("refined" in c for c in hooked[2])
    chans = np.arange(kw["nchan"])
    ref, st1 = K.two_pass(x.T, chans, tout, dms, kw["fch1"], kw["foff"], kw["nchan"], 4, t0, 1)
    _same_refinement(hooked[3], ref)
    assert abs(hooked[3]["dm"] - dm_true) <= 0.5 * st1 and abs(hooked[3]["dm"] - dm_true) < abs(dms[4] - dm_true)
    # what the hook attached to the strongest candidate is the restatement's for that candidate
    c = max(hooked[2], key=lambda c: c["snr"])
    assert c["dmi"] in (4, 5) and abs(c["peak_idx"] - t0) <= 64       # 3 DM off: smeared over ~32 samples
    ref, _ = K.two_pass(x.T, chans, tout, dms, kw["fch1"], kw["foff"], kw["nchan"], c["dmi"], c["peak_idx"], c["tfilt"])
    _same_refinement(c["refined"], ref)


def test_production_geometry_pulse_across_a_gulp_boundary_is_refined(tmp_path, capsys):
    sig = importlib.import_module("vlite-fast_amd.sigproc")
    nchan, gulp, ngulp = 4096, search.HEIMDALL_GULP, 3
    dm, t0, width = 503.0, 58000, 4                      # off the trial DMs; the sweep (~5690 samples) crosses sample 61 440
    fch1, foff, tsamp = float(np.float32(search.FCH1)), float(np.float32(search.FOFF)), float(np.float32(search.TSAMP))
    dml = search.dedisp_dm_list(2.0, 1000.0, tsamp, fch1, foff, nchan)
    zapped = np.zeros(nchan, bool)
    for lo, hi in search.HEIMDALL_ZAP:
        zapped[lo:hi] = True
    rng = np.random.default_rng(53)
    stream = np.empty((ngulp * gulp, nchan), np.uint8)
    for i in range(0, stream.shape[0], 3072):
        g = rng.standard_normal((3072, nchan), dtype=np.float32)
        stream[i:i + 3072] = np.clip(np.floor(g / np.float32(0.02957) + np.float32(127.5)), 0, 255).astype(np.uint8)
    sweep = K.delays([dm], fch1, foff, nchan, tsamp)[0]
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
    found = []
    with search.Searcher(max_samples=maxs, fch1=fch1, foff=foff, tsamp=tsamp, dm_list=dml) as s:
        s.set_baseline(int(2.0 / tsamp))
        s.set_refine(max_cands=8)
        g = search.GulpSearch(s, threshold=7.0, refine=dict(thresh=10.0, max_per_gulp=8))
        lines = []
        for k in range(ngulp + 1):
            cands = g.push(stream[k * gulp:(k + 1) * gulp]) if k < ngulp else g.finish()
            lines += [search.candidate_line(c) for c in cands]
            assert [c["peak_idx"] for c in cands if "refined" in c] == [c["peak_idx"] for c in cands if c["snr"] >= 10.0][:8]
            for c in cands:
                if "refined" in c and abs(c["dm"] - dm) < 10 and abs(c["peak_idx"] - t0) <= 4:
                    first = g.last_first
                    xt = s.fetch_clean()
                    ref, st1 = K.two_pass(xt, np.nonzero(~zapped)[0], xt.shape[1] - s.max_delay, np.asarray(s.dms, np.float64), fch1,
                                        foff, nchan, c["dmi"], c["peak_idx"] - first, c["tfilt"], tsamp=tsamp)
                    found.append((k, c, ref, st1, first))
    assert found and all(f[0] == 2 for f in found)                      # found in the third gulp only
    for _, c, ref, st1, first in found:                                 # (an off-grid pulse may leave a weaker twin)
        _same_refinement(c["refined"], ref, first)
    _, c, ref, st1, first = max(found, key=lambda f: f[1]["snr"])
    r = c["refined"]
    print("candidate DM %.3f S/N %.2f -> refined DM %.4f S/N %.2f width %d peak %d (injected DM %.1f at %d)" % (
        c["dm"], c["snr"], r["dm"], r["snr"], r["width"], r["peak"], dm, t0))
    _same_refinement(r, ref, first)
    # what pins the result is the equality above; that refinement moves a DM towards the injected one is proved on the
    # reduced geometry (test_never_switched_on_changes_nothing, tests/test_search_refine_cpu.py), not claimed here
    assert abs(r["peak"] - t0) <= 4
    # the command line: the same lines, and a .refined file per gulp that parses to the same numbers
    out = tmp_path / "cands"
    capsys.readouterr()                                                 # (what this test printed so far)
    n = search.main(["-f", str(fil), "-detect_thresh", "7", "-zap_chans", "0", "190", "-zap_chans", "3900", "4096", "-refine",
                     "-refine_thresh", "10", "-refine_max", "8", "-output_dir", str(out)])
    printed = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert n == len(printed) == len(lines) and printed == lines
    files = sorted(p for p in os.listdir(out) if p.endswith(".refined"))
    assert files and all(p[:-len(".refined")] + ".cand" in os.listdir(out) for p in files)
    rl = [l.split() for p in files for l in open(out / p).read().splitlines()]
    assert all(len(t) == 13 for t in rl)
    mine = [t for t in rl if " ".join(t[:9]) == " ".join(search.candidate_line(c).split())]
    assert len(mine) == 1
    assert (float(mine[0][9]), int(mine[0][11]), int(mine[0][12])) == (float("%.6f" % r["dm"]), r["width"], r["peak"])
    assert float(mine[0][10]) == float("%.4f" % r["snr"])
