"""The periodicity search on the GPU (csrc/search_periodic.hip; definition: include/pb_hip.h, pb_search_set_periodic) against
its restatement (tests/search_periodic_ref.py, held to hand-made answers by tests/test_search_periodic_cpu.py).

  1. the folded profiles are the restatement's on the GPU's own series, exactly, over the corners of the geometry;
  2. the window positions are the restatement's exactly and the S/N within 1 binary32 ulp of the restatement fed the GPU's
     binary32 rms (the double evaluation is correctly rounded far below a binary32 ulp: only a tie at the final rounding can
     differ);
  3. the best table is the set that the tie rules make of the GPU's own per-trial S/N: only comparisons take part, so the
     two are equal bit for bit; it does not depend on dm_chunk;
  4. a train of pulses that the single-pulse search misses at a threshold of 6 is found at its DM and period;
  5. the command line writes its .periodic line, streamed or not;
  6. a handle on which the stage is off returns what it returned before, and the refusals.
Band: fch1 384 MHz, 64 MHz wide downwards, tsamp 781.25 us, cleaning off."""
import ctypes as C
import importlib

import numpy as np
import pytest

import search_periodic_cases as CASE
import search_periodic_ref as R
import search_subband_ref as SB

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")
libpb = importlib.import_module("vlite-fast_amd.libpb")

TSAMP = 781.25e-6
EINVAL = -22


def _searcher(nchan, nsamp, dms, zap=()):
    return search.Searcher(device=0, nchan=nchan, max_samples=nsamp, fch1=384.0, foff=-64.0 / nchan, tsamp=TSAMP, boxcar_max=64,
                           zap=tuple(zap), dm_list=np.asarray(dms, np.float32))


def _nsamp(nchan, dms, tout, zap=()):
    delay = SB.delays(dms, 384.0, -64.0 / nchan, nchan, TSAMP)
    return tout + int(delay[:, ~SB.zap_mask(nchan, zap)].max()), delay


def _noise(seed, nsamp, nchan):
    return np.clip(np.rint(np.random.default_rng(seed).normal(96.0, 12.0, (nsamp, nchan))), 0, 255).astype(np.uint8)


def _ulp_apart(a, b):
    """how many binary32 values lie between two arrays of non-negative floats"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _check_fold(s, series, rms, d, k, p, B):
    """one (dm, k, p) of the device against the restatement; returns the device's fold"""
    got = s.periodic_fold(d, k, p)
    x = R.downsample(series[d], k)
    m, M, _ = R.rows_of(len(x), p)
    assert (got["m"], got["M"]) == (m, M), (d, k, p)
    if M == 0:
        assert got["prof"].shape == (0, p)
        return got
    F = R.fold_stages(x, p)
    assert np.array_equal(got["prof"], F), (d, k, p)
    snr, jb = R.evaluate(F, B, m, k, rms[d])
    assert np.array_equal(got["jbest"], jb), (d, k, p)
    apart = _ulp_apart(got["snr"], snr)
    assert apart.max() <= 1, (d, k, p, int(apart.max()))
    return got


# ---- 1, 2: profiles, window positions and S/N ----
# id: (nchan, B, tout, dms, zap, k_lo, k_hi, dm_chunk, [(k, p) checked at every DM])
GEOM = {
    # m a power of two, no padding: p 32 -> m 16 = M, p 63 -> m 8 = M
    "B32-tout512-pow2": (64, 32, 512, (0.0, 30.0), (), 0, 0, 0, [(0, 32), (0, 63), (0, 47)]),
    # m = 2^L + 1, most padding: p 32 -> m 17, M 32; p 63 -> m 8
    "B32-tout544-pad": (64, 32, 544, (0.0, 30.0), (), 0, 0, 0, [(0, 32), (0, 63), (0, 33)]),
    # the shortest block: p 32 -> m 2 (one stage, folded inside the evaluation), every other p skipped (m 1)
    "B32-tout64-m2": (64, 32, 64, (0.0, 30.0), (), 0, 0, 0, [(0, 32), (0, 33), (0, 63)]),
    # octave 2 of 2059 samples: n_k 514 = 16 x 32 + 2 = 8 x 63 + 10; octaves 0 and 1 beside it
    "B32-tout2059-k2": (64, 32, 2059, (0.0, 30.0), (), 0, 2, 0, [(2, 32), (2, 63), (2, 51), (1, 63), (0, 32)]),
    # B 64: p 64 -> m 64, p 127 -> m 32; octave 1: m 32, 16
    "B64-tout4096": (64, 64, 4096, (0.0, 30.0), (), 0, 1, 0, [(0, 64), (0, 127), (1, 64), (1, 127), (0, 100)]),
    # B 64, most padding at p 64: m 33 -> M 64; p 127: m 16
    "B64-tout2112-pad": (64, 64, 2112, (0.0, 30.0), (), 0, 0, 0, [(0, 64), (0, 127)]),
    # chunks 3 + 3 + 1 and a trial DM in each
    "ndm7-chunk3": (64, 32, 700, (0.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0), (), 0, 1, 3, [(0, 32), (1, 63), (0, 40)]),
    # a zapped band: nact 200 of 256
    "nchan256-zapped": (256, 32, 300, (0.0, 30.0), ((0, 40), (100, 116)), 0, 1, 0, [(0, 32), (0, 63), (1, 32), (1, 63)]),
    # only the higher octaves switched on: octave 3 of 4096 samples, n_k 512
    "B32-tout4096-k3": (64, 32, 4096, (0.0, 30.0), (), 3, 4, 0, [(3, 32), (3, 63), (4, 32), (4, 63)]),
}


@pytest.mark.parametrize("name", sorted(GEOM))
def test_profiles_positions_and_snr(name):
    nchan, B, tout, dms, zap, k_lo, k_hi, chunk, checks = GEOM[name]
    nsamp, _ = _nsamp(nchan, dms, tout, zap)
    x = _noise(len(name), nsamp, nchan)
    with _searcher(nchan, nsamp, dms, zap) as s:
        s.set_periodic(B, k_lo, k_hi, dm_chunk=chunk)
        r = s.run(x, want_series=True)
        assert r["tout"] == tout
        rms = r["stats"][:, 1]
        for d in range(len(dms)):
            for k, p in checks:
                _check_fold(s, r["series"], rms, d, k, p, B)
        # the table agrees with the full folds at the entries checked
        tab = s.periodic()
        for d in range(len(dms)):
            for k, p in checks:
                f = s.periodic_fold(d, k, p)
                e = tuple(tab[key][d, k - k_lo, p - B] for key in ("snr", "i", "q", "j"))
                if f["M"] == 0:
                    assert e == (0.0, -1, 0, 0) and tab["M"][d, k - k_lo, p - B] == 0 and np.isnan(tab["period_s"][d, k - k_lo, p - B])
                else:
                    assert e == R.best_of(f["snr"], f["jbest"]), (d, k, p)
                    assert (tab["m"][d, k - k_lo, p - B], tab["M"][d, k - k_lo, p - B]) == (f["m"], f["M"])


def test_pulse_across_the_profiles_end():
    """a train whose pulses fall in bins p - 1 and 0 of base period 40: the circular window of width 2 starts at bin p - 1"""
    nchan, tout, p = 64, 40 * 16 + 11, 40
    nsamp, _ = _nsamp(nchan, (0.0,), tout)
    g = np.random.default_rng(3).normal(96.0, 12.0, (nsamp, nchan))
    for t0 in range(p - 1, nsamp - 2, p):
        g[t0:t0 + 2] += 8.0
    x = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    with _searcher(nchan, nsamp, (0.0,)) as s:
        s.set_periodic(32)
        r = s.run(x, want_series=True)
        got = _check_fold(s, r["series"], r["stats"][:, 1], 0, 0, p, 32)
        assert got["jbest"][0, 1] == p - 1 and got["jbest"][0, 2] in (p - 3, p - 2, p - 1)
        assert got["snr"][0, 1] > 20 and np.argmax(got["snr"][0]) == 1
        b = s.periodic()
        assert (b["i"][0, 0, p - 32], b["q"][0, 0, p - 32], b["j"][0, 0, p - 32]) == (0, 1, p - 1)
        assert b["period_s"][0, 0, p - 32] == p * TSAMP


# ---- 3: the best table ----
def test_best_table_is_the_tie_rules_on_the_devices_own_snr():
    dms = (0.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0)
    nsamp, _ = _nsamp(64, dms, 700)
    x = _noise(11, nsamp, 64)
    tabs = {}
    with _searcher(64, nsamp, dms) as s:
        s.peaks(x, 6.0)
        for chunk in (3, 4, 0):
            s.set_periodic(32, 0, 2, dm_chunk=chunk)
            tabs[chunk] = s.periodic()
        t = tabs[0]
        for d in range(len(dms)):
            for ki in range(3):
                for p in range(32, 64):
                    f = s.periodic_fold(d, ki, p)
                    e = (t["snr"][d, ki, p - 32], t["i"][d, ki, p - 32], t["q"][d, ki, p - 32], t["j"][d, ki, p - 32])
                    want = R.best_of(f["snr"], f["jbest"]) if f["M"] else (np.float32(0), -1, 0, 0)
                    assert e == want and e[0].tobytes() == np.float32(want[0]).tobytes(), (d, ki, p)
        tm = s.periodic_timers()
        assert tm["fold"] > 0 and tm["eval"] > 0 and tm["with_copy"] >= tm["fold"] + tm["eval"] - 1e-3
    for chunk in (3, 4):
        for key in ("snr", "i", "q", "j", "m", "M"):
            assert tabs[chunk][key].tobytes() == tabs[0][key].tobytes(), (chunk, key)


# ---- 4: detection ----
def test_weak_train_is_found():
    """The case of tests/search_periodic_cases.py.  In the restatement alone (checked here before the GPU run): the largest
    single-pulse S/N over the five DMs is 3.95, the periodic S/N at DM index 2 is 15.82 at p 41, i 48 of 128 = 41.378
    samples against 41.37 (tolerance (w + 1) / (m p) = 3 / (99 x 41) = 7.4e-4), and no other DM passes 5.04."""
    ref = CASE.restated()
    b = ref["best"][2]
    k = int(np.argmax(b["snr"][0]))
    print("restatement: single %.3f, periodic %s" % (ref["single"], [float(v["snr"].max()) for v in ref["best"]]))
    assert ref["single"] < 6 and b["snr"][0, k] >= 10 and 32 + k == 41
    tol = ((1 << int(b["q"][0, k])) + 1.0) / (int(b["m"][0, k]) * 41)
    assert abs(R.period_samples(41, int(b["i"][0, k]), int(b["M"][0, k])) / CASE.PERIOD - 1) <= tol
    x, _, nsamp = CASE.block()
    with search.Searcher(device=0, nchan=CASE.NCHAN, max_samples=nsamp, fch1=CASE.FCH1, foff=CASE.FOFF, tsamp=TSAMP, zap=(),
                         dm_list=np.asarray(CASE.DMS, np.float32)) as s:
        s.set_periodic(CASE.BINS)
        pk = s.peaks(x, 6.0)
        assert pk["total"] == 0 and pk["tout"] == CASE.TOUT
        t = s.periodic()
        d, ki, pi = np.unravel_index(np.argmax(t["snr"]), t["snr"].shape)
        assert (d, ki, 32 + pi) == (2, 0, 41)
        for key in ("i", "q", "j", "m", "M"):
            assert t[key][2, 0, pi] == b[key][0, pi], key                   # the peak's entry is the restatement's
        assert _ulp_apart(t["snr"][2, 0, pi:pi + 1], b["snr"][0, pi:pi + 1]).max() <= 1
        assert abs(t["period_s"][d, ki, pi] / (CASE.PERIOD * TSAMP) - 1) <= tol
        cands = search.candidates_from_periodic(t, s.dms, TSAMP, 8.0)
        assert len(cands) == 1, cands
        c = cands[0]
        assert (c["dmi"], c["p"], c["k"], c["dm"]) == (2, 41, 0, 40.0) and c["snr"] >= 10


# ---- 5: through the tool ----
def test_command_line_writes_the_periodic_file(tmp_path, capsys):
    sig = importlib.import_module("vlite-fast_amd.sigproc")
    x, _, nsamp = CASE.block()
    hdr = b"".join([sig.send_string("HEADER_START"), sig.send_int("data_type", 1), sig.send_double("fch1", CASE.FCH1),
                    sig.send_double("foff", CASE.FOFF), sig.send_int("nchans", CASE.NCHAN), sig.send_int("nbits", 8),
                    sig.send_double("tstart", 57570.0), sig.send_double("tsamp", TSAMP), sig.send_int("nifs", 1),
                    sig.send_string("HEADER_END")])
    fil = tmp_path / "train.fil"
    fil.write_bytes(hdr + x.tobytes())
    flags = ["-f", str(fil), "-dm", "0", "80", "-dm_step", "20", "-nsamps_gulp", str(nsamp), "-detect_thresh", "6",
             "-baseline_length", "0", "-periodic", "0.025", "0.06", "-periodic_bins", "32"]
    lines = {}
    for what, more in (("gulps", []), ("pieces", ["-stream_chunk", "500"])):
        out = tmp_path / what
        capsys.readouterr()
        assert search.main(flags + more + ["-output_dir", str(out)]) == 1
        printed = capsys.readouterr().out.splitlines()
        files = sorted(p.name for p in out.iterdir())
        assert len(printed) == 1 and len(files) == 1 and files[0].endswith(".periodic"), (printed, files)   # no .cand
        assert (out / files[0]).read_text() == printed[0] + "\n"
        lines[what] = printed[0]
    col = lines["gulps"].split("\t")
    assert len(col) == 11 and float(col[0]) >= 10 and float(col[2]) == 40.0 and col[5:8] == ["2", "0", "41"]
    assert abs(float(col[1]) / (CASE.PERIOD * TSAMP) - 1) <= 7.4e-4
    assert float(col[3]) in (TSAMP, 2 * TSAMP, 4 * TSAMP) and 0 <= float(col[4]) < 1
    assert lines["pieces"] == lines["gulps"]
    # without the flag the same file gives nothing, as before
    capsys.readouterr()
    out = tmp_path / "plain"
    assert search.main(flags[:flags.index("-periodic")] + ["-output_dir", str(out)]) == 0
    assert capsys.readouterr().out == "" and list(out.iterdir()) == []


# ---- 6: off is off, and the refusals ----
def test_off_is_off_and_refusals():
    dms = (0.0, 20.0, 40.0, 60.0)
    nsamp, _ = _nsamp(256, dms, 600)
    x = _noise(2, nsamp, 256)
    L = libpb.load()

    def outputs(s):
        pk = s.peaks(x, 2.5)
        order = np.lexsort((pk["t"], pk["dmi"]))
        r = s.run(x, want_series=True)
        return b"".join(np.ascontiguousarray(pk[k][order]).tobytes() for k in ("dmi", "t", "snr", "width_log2")) + \
            r["snr"].tobytes() + r["width_log2"].tobytes() + r["stats"].tobytes() + r["series"].tobytes(), pk["total"]

    def refused(rc, what, s):
        assert rc == EINVAL and what in L.pb_search_last_error(s._s).decode(), L.pb_search_last_error(s._s).decode()

    best = (C.c_int32 * (4 * 32 * 4))(*([-7] * 512))
    m, M = C.c_int(-1), C.c_int(-1)
    with _searcher(256, nsamp, dms) as s:
        # switched on before anything was searched
        s.set_periodic(32)
        refused(L.pb_search_periodic(s._s, best), "no block searched", s)
        refused(L.pb_search_periodic_fold(s._s, 0, 0, 32, None, None, None, C.byref(m), C.byref(M)), "no block searched", s)
        s.set_periodic(0)
        before, total = outputs(s)
        assert total > 0
        # the stage is off: refused with a message, nothing written
        refused(L.pb_search_periodic(s._s, best), "not switched on", s)
        refused(L.pb_search_periodic_fold(s._s, 0, 0, 32, None, None, None, C.byref(m), C.byref(M)), "not switched on", s)
        assert set(best) == {-7} and (m.value, M.value) == (-1, -1)
        with pytest.raises(libpb.PbError, match="set_periodic"):
            s.periodic()
        with pytest.raises(ValueError):
            search.GulpSearch(s, periodic=dict(thresh=8.0))                    # the searcher's stage must be on
        s.set_periodic(32, 0, 1)
        assert outputs(s) == (before, total)
        assert s.periodic()["snr"].max() > 0
        # the refusals of a stage that is on; a refused set call changes nothing
        refused(L.pb_search_periodic(s._s, None), "pointer", s)
        for args, what in (((-1, 0, 32), "DM index"), ((4, 0, 32), "DM index"), ((0, 2, 32), "octave"), ((0, -1, 32), "octave"),
                           ((0, 0, 31), "base period"), ((0, 0, 64), "base period")):
            refused(L.pb_search_periodic_fold(s._s, args[0], args[1], args[2], None, None, None, C.byref(m), C.byref(M)), what, s)
        assert (m.value, M.value) == (-1, -1)
        for args in ((48, 0, 0, 0), (16, 0, 0, 0), (256, 0, 0, 0), (32, -1, 0, 0), (32, 2, 1, 0), (32, 0, 13, 0), (32, 0, 0, -1)):
            with pytest.raises(ValueError):
                s.set_periodic(*args)
        assert s._per == (32, 0, 1) and s.periodic()["snr"].shape == (4, 2, 32)
        s.set_periodic(0)
        assert s._per is None and outputs(s) == (before, total)
        refused(L.pb_search_periodic(s._s, best), "not switched on", s)
    # the range condition: 255 nact ceil(max_samples / bins) must stay below 2^32
    with _searcher(4096, 132000, (0.0,)) as s:
        with pytest.raises(ValueError, match="32 bits"):
            s.set_periodic(32)                                              # 255 x 4096 x 4125 = 4.31e9 >= 2^32 = 4.29e9
        s.set_periodic(64, 6, 6)                                            # 255 x 4096 x 2063 = 2.15e9
