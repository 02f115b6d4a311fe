"""RFI cleaning in the search (pb_search_set_rfi, Searcher.set_rfi, search -rfi_clean) on the GPU: the narrow pass
bit-exact against the NumPy restatement (tests/search_rfi_ref.py), the broad pass's flagged samples against the
restatement fed with the GPU's own zero-DM level and rms (themselves held to tests/search_stats_ref.py), broadband bursts gone from the candidates at the production
geometry while a dispersed pulse survives, byte-identical outputs with cleaning off, and the CLI.  The definition is
this project's own (include/pb_hip.h); parity with heimdall's cleaning is unpinned."""
import importlib

import numpy as np
import pytest

import search_rfi_ref as R
import search_stats_ref as S
import synth

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")

FCH1, FOFF = 361.94, -0.16


def _noise(seed, T, nchan, nbit=8):
    """codes [T][nchan] of nbit bits: Gaussian noise about the middle of the range"""
    g = synth.gauss(seed, T * nchan).reshape(T, nchan)
    top = (1 << nbit) - 1
    return np.clip(np.floor(g * (top / 15.0) + top / 2.0), 0, top).astype(np.uint8)


def _plant_bursts(x, bursts, amp):
    """broadband bursts: (t, width) -> +amp codes in every channel"""
    y = x.astype(np.int32)
    for t, w in bursts:
        y[t:t + w] += amp
    return np.clip(y, 0, 255).astype(np.uint8)


def _zmask(nchan, zap):
    m = np.zeros(nchan, bool)
    for lo, hi in zap:
        m[lo:hi] = True
    return m


@pytest.mark.parametrize("case", range(9))
def test_narrow_pass_bit_exact(case):
    nbit = (8, 4, 2)[case % 3]
    rng = np.random.default_rng(100 + case)
    nchan = int((64, 200, 256)[case // 3])
    zap = [(), ((0, 7), (nchan - 5, nchan)), ((nchan // 2, nchan // 2 + 9),)][case // 3]
    T = int(rng.choice([300, 1031, 2048, 4000]))
    top = (1 << nbit) - 1
    x = _noise(7 + case, T, nchan, nbit)
    # planted outliers: a few single samples, a stretch of one channel, a carrier at full scale
    n_out = T * nchan // 200
    x[rng.integers(0, T, n_out), rng.integers(0, nchan, n_out)] = rng.choice([0, top], n_out)
    x[T // 3:T // 3 + 40, nchan // 3] = top
    tol = (5.0, 3.0, 1.0)[case % 3] if nbit != 2 or case % 2 else 3.0
    kw = dict(nchan=nchan, max_samples=4096, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_min=0.0, dm_max=4.0,
              dm_step=2.0, boxcar_max=16, zap=zap)
    chans = np.nonzero(~_zmask(nchan, zap))[0]
    with search.Searcher(**kw) as s:
        s.set_rfi(narrow=True, broad=False, tol=tol)
        s.run(R.pack(x, nbit), nbit=nbit)
        got = s.fetch_clean()
        info = s.rfi_info()
    ref, n, _ = R.narrow(np.ascontiguousarray(x.T), chans, tol)
    assert np.array_equal(got, ref), (case, nbit, tol)
    assert info["n_narrow"] == n and info["n_broad_samples"] == 0 and info["ms"] > 0
    if nbit == 2 and tol >= 3:
        assert n == 0                                   # nothing can be flagged at 2 bits
    else:
        assert n > 0


def _gpu_zero_dm(xt_t, nchan, zap, W):
    """the GPU's own zero-DM series, level and rms: a DM-0 search (no delays, tout = nsamp) of the given block"""
    with search.Searcher(nchan=nchan, max_samples=xt_t.shape[0], fch1=FCH1, foff=FOFF, tsamp=search.TSAMP,
                         dm_list=[0.0], boxcar_max=1, zap=zap) as z:
        z.set_baseline(W)
        r = z.run(xt_t, want_series=True)
    assert r["tout"] == xt_t.shape[0]
    return r["series"][0], r["stats"][0]


@pytest.mark.parametrize("W,narrow,boxcar_max", [(0, True, 16), (512, True, 16), (512, False, 8), (0, True, 64)])
def test_broad_pass_flags_the_restated_samples(W, narrow, boxcar_max):
    nchan, T, tol = 256, 4096, 5.0
    zap = ((0, 10), (250, 256))
    x = _noise(31, T, nchan)
    bursts = [(300, 1), (900, 2), (1500, 3), (2100, 4), (2700, 6), (3300, 8), (4090, 5)]
    x = _plant_bursts(x, bursts, 24)
    x[1000:1100, 77] = 255                              # a carrier: the narrow pass's
    chans = np.nonzero(~_zmask(nchan, zap))[0]
    kw = dict(nchan=nchan, max_samples=T, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_min=0.0, dm_max=20.0,
              dm_step=2.0, boxcar_max=16, zap=zap)
    with search.Searcher(**kw) as s:
        s.set_baseline(W)
        if narrow:
            s.set_rfi(narrow=True, broad=False, tol=tol)
            s.run(x)
            xa = s.fetch_clean()                        # what the broad pass starts from
        else:
            xa = np.ascontiguousarray(x.T)
        s.set_rfi(narrow=narrow, broad=True, tol=tol, boxcar_max=boxcar_max)
        s.run(x)
        xb = s.fetch_clean()
        info = s.rfi_info()
    z, (level, rms) = _gpu_zero_dm(np.ascontiguousarray(xa.T), nchan, zap, W)
    assert np.array_equal(z, R.zero_dm(xa, chans))
    # that level and rms are the definition's (tests/search_stats_ref.py, under test_gpu_search_stats.py's tolerance:
    # rms 1 binary32 ulp, level 1 ulp + the summation bound), so the flag set is tied to the reference end to end
    lvl_ref, rms_ref, n_boundary = S.series_stats(z.astype(np.int64), W)
    assert n_boundary == 0
    assert abs(float(rms) - float(rms_ref)) <= float(np.spacing(rms_ref)), (rms, rms_ref)
    assert abs(float(level) - float(lvl_ref)) <= S.level_tolerance(z.astype(np.int64), W, lvl_ref), (level, lvl_ref)
    nbox = boxcar_max.bit_length()
    best, bw = R.zero_dm_snr(z, level, rms, nbox, W)
    sure = R.broad_flags(best, bw, tol * (1 + 1e-4))
    maybe = R.broad_flags(best, bw, tol * (1 - 1e-4))
    amb = maybe & ~sure                                 # samples reached only from S/N within 1e-4 of tol
    flags = R.broad_flags(best, bw, tol)
    for t, w in bursts:
        assert flags[t:min(T, t + w)].all(), (t, w)
    _, _, meds = R.narrow(xa, chans, tol, replace=False)
    ref = R.apply_broad(xa, chans, meds, flags)
    keep = ~amb
    assert np.array_equal(xb[:, keep], ref[:, keep])   # flagged samples hold med_c, the others are untouched
    assert sure.sum() <= info["n_broad_samples"] <= maybe.sum()
    assert 0 < info["n_broad_samples"] < T // 4


def _production_block(T, bursts, pulse, seed):
    """4096-channel 8-bit codes (tests/test_gpu_search.py::_plane's noise) with broadband bursts (t, width) of +1 sigma
    and a dispersed 4-sample pulse (dm, t0)"""
    nchan = 4096
    g = synth.gauss(seed, T * nchan).reshape(T, nchan)
    for t, w in bursts:
        g[t:t + w] += 1.0
    dm, t0 = pulse
    f = search.FCH1 + search.FOFF * np.arange(nchan)
    delay = np.round(4.148808e3 * dm * (f ** -2 - f[0] ** -2) / search.TSAMP).astype(int)
    rows = t0 + delay[None, :] + np.arange(4)[:, None]
    g[rows, np.broadcast_to(np.arange(nchan), rows.shape)] += 0.35
    return np.clip(np.floor(g / 0.02957 + 127.5), 0, 255).astype(np.uint8)


def _at_burst(c, bursts, fch1, foff, nchan, tsamp):
    """a candidate the burst at (t, w) explains: at its DM the burst's sweep ends at t and starts max_delay(DM) earlier"""
    span = 4.148808e3 * c["dm"] * ((fch1 + (nchan - 1) * foff) ** -2 - fch1 ** -2) / tsamp
    return any(t - span - 80 <= c["peak_idx"] <= t + w + 80 for t, w in bursts)


def test_production_geometry_bursts_gone_pulse_kept():
    T = 18432
    bursts = [(600, 1), (1800, 2), (3000, 3), (4200, 5), (5400, 8)]
    pulse = (500.0, 6600)
    x = _production_block(T, bursts, pulse, 77)
    dml = search.dedisp_dm_list(2.0, 1000.0, search.TSAMP, search.FCH1, search.FOFF, 4096)
    with search.Searcher(max_samples=T, dm_list=dml) as s:
        s.set_baseline(2560)
        pk0 = s.peaks(x, 7.0, max_out=1 << 20)
        s.set_rfi()
        pk1 = s.peaks(x, 7.0, max_out=1 << 20)
        info = s.rfi_info()
        dms = s.dms
    assert pk0["total"] <= 1 << 20 and pk1["total"] <= 1 << 20
    c0 = search.candidates_from_peaks(pk0, dms, search.TSAMP)
    c1 = search.candidates_from_peaks(pk1, dms, search.TSAMP)
    geo = (search.FCH1, search.FOFF, 4096, search.TSAMP)
    burst0 = [c for c in c0 if _at_burst(c, bursts, *geo)]
    for t, w in bursts:                                  # uncleaned: every burst shows up
        assert any(_at_burst(c, [(t, w)], *geo) for c in burst0), (t, w)
    assert not [c for c in c1 if _at_burst(c, bursts, *geo)]
    assert 0 < info["n_broad_samples"] < 2000 and info["ms"] > 0

    def pulse_cand(cs):
        near = [c for c in cs if abs(c["dm"] - pulse[0]) <= 0.05 * pulse[0] and abs(c["peak_idx"] - pulse[1]) <= 4]
        assert near, "pulse not found"
        return max(near, key=lambda c: c["snr"])

    p0, p1 = pulse_cand(c0), pulse_cand(c1)
    assert p1["snr"] >= 0.95 * p0["snr"], (p0, p1)


def test_off_means_off():
    nchan, T = 256, 4096
    x = _plant_bursts(_noise(41, T, nchan), [(1000, 2), (2500, 6)], 30)
    kw = dict(nchan=nchan, max_samples=T, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_min=0.0, dm_max=40.0,
              dm_step=2.0, boxcar_max=16, zap=((0, 10),))

    def outputs(s):
        r = s.run(x, want_series=True)
        pk = s.peaks(x, 6.0)
        order = np.lexsort((pk["width_log2"], pk["t"], pk["dmi"]))
        return [r["snr"].tobytes(), r["width_log2"].tobytes(), r["series"].tobytes(), r["stats"].tobytes(),
                np.stack([pk["dmi"][order], pk["t"][order], pk["snr"][order].view(np.int32),
                          pk["width_log2"][order].astype(np.int32)]).tobytes(), s.fetch_clean().tobytes()]

    with search.Searcher(**kw) as a:
        never = outputs(a)
        assert a.rfi_info() == dict(n_narrow=0, n_broad_samples=0, ms=0.0)
    with search.Searcher(**kw) as b:
        b.set_rfi(False, False)
        off = outputs(b)
    with search.Searcher(**kw) as c:
        c.set_rfi()
        cleaned = outputs(c)
        assert c.rfi_info()["n_broad_samples"] > 0
        c.set_rfi(False, False)
        after = outputs(c)
        assert c.rfi_info() == dict(n_narrow=0, n_broad_samples=0, ms=0.0)
    assert off == never and after == never
    assert cleaned[0] != never[0]                        # (and cleaning did change something)


def _fil(tmp_path, codes):
    sigproc = importlib.import_module("vlite-fast_amd.sigproc")
    fil = tmp_path / "obs_kur.fil"
    fil.write_bytes(sigproc.sigproc_header(7, 0.87, -0.72, "B0833-45", 57570 + 3600 / 86400., 1, 8) + codes.tobytes())
    return str(fil)


def test_gulps_and_cli_with_and_without_cleaning(tmp_path, capsys):
    T, gulp = 16384, 8192
    bursts = [(3000, 2), (5000, 4), (9000, 8), (11000, 1)]
    pulse = (150.0, 7000)                               # its sweep (~1700 samples) crosses sample 8192
    x = _production_block(T, bursts, pulse, 78)
    fil = _fil(tmp_path, x)
    args = ["-f", fil, "-dm", "2", "400", "-nsamps_gulp", str(gulp), "-zap_chans", "0", "190", "-zap_chans", "3900",
            "4096", "-detect_thresh", "7"]
    n_plain = search.main(args)
    plain = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    # what the CLI printed before cleaning existed: the same Searcher and GulpSearch, never configured for cleaning
    sigproc = importlib.import_module("vlite-fast_amd.sigproc")
    with open(fil, "rb") as f:
        hdr, off = sigproc.read_header(f.read(4096))
    tsamp = hdr["tsamp"]
    dml = search.dedisp_dm_list(2.0, 400.0, tsamp, hdr["fch1"], hdr["foff"], 4096, 1.25)
    maxs = gulp + int(4.148808e3 * 400.0 * abs((hdr["fch1"] + 4095 * hdr["foff"]) ** -2 - hdr["fch1"] ** -2) / tsamp) + 64
    with search.Searcher(max_samples=maxs, dm_list=dml, fch1=hdr["fch1"], foff=hdr["foff"], tsamp=tsamp,
                         zap=((0, 190), (3900, 4096))) as s:
        s.set_baseline(int(2.0 / tsamp))
        g = search.GulpSearch(s, threshold=7.0)
        ref = []
        for i in range(0, T, gulp):
            ref += g.push(x[i:i + gulp])
        ref += g.finish()
    assert plain == [search.candidate_line(c) for c in ref] and n_plain == len(plain)
    cols = [l.split() for l in plain]
    def span(dm):
        return 4.148808e3 * dm * ((hdr["fch1"] + 4095 * hdr["foff"]) ** -2 - hdr["fch1"] ** -2) / tsamp

    def at_burst(c):
        return any(t - span(float(c[5])) - 80 <= int(c[1]) <= t + w + 80 for t, w in bursts)

    def has_pulse(cs):
        return any(abs(float(c[5]) - pulse[0]) < 15 and abs(int(c[1]) - pulse[1]) <= 4 for c in cs)

    assert any(at_burst(c) for c in cols) and has_pulse(cols)
    search.main(args + ["-rfi_clean"])
    clean = [l.split() for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert not [c for c in clean if at_burst(c)]
    assert has_pulse(clean)
