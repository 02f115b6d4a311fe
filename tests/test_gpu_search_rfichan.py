"""The cleaning's channel stage (pb_search_set_rfi_chan, Searcher.set_rfi_chan, search -rfi_chan) on the GPU: every output
equal to the NumPy restatement (tests/search_rfichan_ref.py) at the geometries where the kernels can go wrong, the order
with the narrow and broad passes, the effect on a pulse under noisy channels, off means off, the refusals, streaming,
polarisation and the CLI.  The definition is this project's own (include/pb_hip.h)."""
import importlib
import os

import numpy as np
import pytest

import search_pol_ref as P
import search_rfi_ref as RFI
import search_rfichan_ref as R
import synth
from test_gpu_search_rfi import _gpu_zero_dm, _noise, _plant_bursts
from test_gpu_search_stream import LEN4, N, NCH4, fil_header, run_main, same, searcher, stream4, to_device

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")
libpb = importlib.import_module("vlite-fast_amd.libpb")

FCH1, FOFF = 361.94, -0.16
KEYS = ("sum", "stat", "fill", "recv", "cast", "mask")
# (nchan, zap) by the number of unzapped channels they leave: on both sides of the sort's padding to a power of two
GEO = {1: (3, ((0, 1), (2, 3))), 2: (4, ((1, 3),)), 3: (3, ()), 100: (112, ((0, 4), (50, 58))), 257: (264, ((100, 107),)),
       1024: (1030, ((0, 6),)), 3710: (4096, search.HEIMDALL_ZAP)}


def handle(nact, max_samples, **kw):
    """a searcher of GEO[nact] at DM 0 only: no delays, so blocks down to 64 samples are searched"""
    nchan, zap = GEO[nact]
    s = search.Searcher(nchan=nchan, max_samples=max_samples, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_list=[0.0],
                        boxcar_max=4, zap=zap, **kw)
    assert s.nact == nact and s.max_delay == 0
    return s


def block(seed, nsamp, nchan, nbit=8):
    """codes [nsamp][nchan] below 2^nbit: noise whose spread differs a little from channel to channel and a lot in a few"""
    rng = np.random.default_rng(seed)
    top = (1 << nbit) - 1
    sig = top / 16.0 * (1.0 + 0.05 * rng.standard_normal(nchan))
    loud = rng.random(nchan) < 0.06
    sig[loud] *= rng.uniform(1.5, 4.0, int(loud.sum()))
    x = rng.standard_normal((nsamp, nchan)) * sig[None, :] + top / 2.0 + rng.uniform(-1, 1, nchan)[None, :]
    return np.clip(np.floor(x + 0.5), 0, top).astype(np.uint8)


def check(s, x, radius, tol, tag=None):
    """the stage's outputs after s searched the block x [nsamp][nchan] == the restatement's, which is returned"""
    nsamp = x.shape[0]
    ref = R.stage(np.ascontiguousarray(x.T), s.chans, nsamp, radius, tol)
    got = s.rfi_chan_info()
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (tag, k)
    assert got["nflag"] == ref["nflag"] and got["ms"] > 0, tag
    assert np.array_equal(s.fetch_clean(), ref["xt"]), tag
    return ref


@pytest.mark.parametrize("nact", [1, 2, 3, 100, 257, 1024])
def test_equal_to_the_restatement_at_every_block_length(nact):
    """4096 + 5 first: the shorter blocks after it leave its bytes beyond their own nsamp in the rows, and their moments
    must be those of their own samples (what a fill does beyond nsamp no entry point can read back: every path
    overwrites a sample before it reads it; k_rfichan_fill stores through stream_store16 with the range [0, nsamp))"""
    nchan = GEO[nact][0]
    flagged = 0
    with handle(nact, 4101) as s:
        s.set_rfi_chan(0, 3.0)
        x0 = block(10 + nact, 4101, nchan)
        for i, nsamp in enumerate((4101, 64, 1037, 1000)):
            x = x0 if i == 0 else block(20 * nact + i, nsamp, nchan)
            s.run(x)
            flagged += check(s, x, 0, 3.0, tag=(nact, nsamp))["nflag"]
    if nact >= 100:
        assert flagged > 0                                          # (the comparison was not of empty masks)


@pytest.mark.parametrize("nbit", [8, 4, 2])
def test_bit_depths(nbit):
    """at 2 bits S takes few values: many ties in the sort"""
    nchan = GEO[100][0]
    x = block(40 + nbit, 1037, nchan, nbit)
    with handle(100, 1037) as s:
        s.set_rfi_chan(0, 3.0)
        s.run(RFI.pack(x, nbit), nbit=nbit)
        check(s, x, 0, 3.0, tag=nbit)


def test_production_channels_and_edge_zaps():
    x = block(50, 256, 4096)
    with handle(3710, 256) as s:
        s.set_rfi_chan()
        s.run(x)
        ref = check(s, x, 0, 4.0)
    assert 0 < ref["nflag"] < 3710 and not ref["mask"][:190].any() and not ref["mask"][3900:].any()


@pytest.mark.parametrize("kind", ["all 255", "all 0", "alternating"])
def test_extreme_blocks(kind):
    """all 255: the widest sums, S = 0 everywhere; alternating 0 / 255 along every row: the largest S"""
    nchan, nsamp = GEO[100][0], 4101
    x = np.zeros((nsamp, nchan), np.uint8)
    if kind == "all 255":
        x[:] = 255
    elif kind == "alternating":
        x[::2] = 255
        x[:, 40] = 128                                              # one quiet channel among them
    with handle(100, nsamp) as s:
        s.set_rfi_chan(0, 3.0)
        s.run(x)
        ref = check(s, x, 0, 3.0, tag=kind)
    assert ref["nflag"] == 0
    if kind == "alternating":
        assert ref["stat"][10] == 4101 * 2051 * 65025 - (2051 * 255) ** 2 and ref["cast"][40] > 0


def test_the_longest_block_the_stage_accepts():
    """2^23 samples of 255 in one channel: a lane's 32-bit sum of squares ends at 8192 x 260100 < 2^32; an alternating
    channel beside it: S = nsamp^2 255^2 / 4, the largest value the 64-bit statistic takes"""
    nsamp = 1 << 23
    x = np.empty((nsamp, 2), np.uint8)
    x[:, 0] = 255
    x[0::2, 1], x[1::2, 1] = 0, 255
    with search.Searcher(nchan=2, max_samples=nsamp, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_list=[0.0], boxcar_max=1,
                         zap=()) as s:
        s.set_rfi_chan(1, 4.0)
        s.peaks(x, float("inf"), max_out=1)
        got = s.rfi_chan_info()
    assert got["sum"].tolist() == [255 * nsamp, 255 * nsamp // 2]
    assert got["stat"].tolist() == [0, nsamp * (nsamp // 2) * 65025 - (255 * nsamp // 2) ** 2]
    assert got["fill"].tolist() == [255, 128]
    ref = R.votes(got["stat"], 1, 4.0)
    assert got["recv"].tolist() == ref[0].tolist() and got["cast"].tolist() == ref[1].tolist()
    assert got["mask"].tolist() == ref[2].astype(int).tolist()


@pytest.mark.parametrize("radius", [0, 1, 257])
@pytest.mark.parametrize("tol", [3.0, 4.0, 50.0])
def test_radius_and_tolerance(radius, tol):
    nchan = GEO[257][0]
    x = block(60, 1000, nchan)
    with handle(257, 1000) as s:
        s.set_rfi_chan(radius, tol)
        s.run(x)
        check(s, x, radius, tol, tag=(radius, tol))


def test_host_and_device_input_agree():
    nchan = GEO[257][0]
    x = block(61, 1037, nchan)
    keep, ptr = to_device(x.ravel(), True)
    with handle(257, 1037) as s:
        s.set_rfi_chan(0, 3.0)
        a = s.run(x)
        ref = check(s, x, 0, 3.0)
        b = s.run(None, device_ptr=ptr, nsamp=1037)
        check(s, x, 0, 3.0)
    assert ref["nflag"] > 0 and a["snr"].tobytes() == b["snr"].tobytes()


def test_the_stage_comes_before_narrow_and_broad():
    """with all three on the block is the restatement's fill, then tests/search_rfi_ref.py's narrow pass, then its broad
    pass fed the GPU's own zero-DM level and rms (as tests/test_gpu_search_rfi.py feeds it)"""
    nchan, T, tol = 256, 4096, 5.0
    zap = ((0, 10), (250, 256))
    x = _plant_bursts(_noise(31, T, nchan), [(300, 1), (1500, 3), (2700, 6)], 24)
    rng = np.random.default_rng(8)
    x[rng.integers(0, T, 60), rng.integers(50, 120, 60)] = 255      # single samples: the narrow pass's
    for c in (40, 41, 130, 200):                                    # channels that are loud throughout: this stage's
        x[:, c] = np.clip(rng.normal(127, 60, T), 0, 255).astype(np.uint8)
    kw = dict(nchan=nchan, max_samples=T, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_min=0.0, dm_max=20.0, dm_step=2.0,
              boxcar_max=16, zap=zap)
    with search.Searcher(**kw) as s:
        chans = s.chans
        s.set_rfi_chan(0, 4.0)
        s.set_rfi(narrow=True, broad=False, tol=tol)
        s.run(x)
        xa = s.fetch_clean()
        n_narrow = s.rfi_info()["n_narrow"]
        ci = s.rfi_chan_info()
        s.set_rfi(narrow=True, broad=True, tol=tol)
        s.run(x)
        xb = s.fetch_clean()
        info = s.rfi_info()
        assert info["ms"] > 0 and s.rfi_chan_info()["ms"] > 0
    ref = R.stage(np.ascontiguousarray(x.T), chans, T, 0, 4.0)
    assert {40, 41, 130, 200} <= set(np.nonzero(ref["mask"])[0].tolist()) and np.array_equal(ci["mask"], ref["mask"])
    xn, n, meds = RFI.narrow(ref["xt"], chans, tol)
    assert np.array_equal(xa, xn) and n_narrow == n and n > 0
    z, (level, rms) = _gpu_zero_dm(np.ascontiguousarray(xa.T), nchan, zap, 0)
    assert np.array_equal(z, RFI.zero_dm(xa, chans))
    best, bw = RFI.zero_dm_snr(z, level, rms, 5, 0)
    sure, maybe = RFI.broad_flags(best, bw, tol * (1 + 1e-4)), RFI.broad_flags(best, bw, tol * (1 - 1e-4))
    flags = RFI.broad_flags(best, bw, tol)
    keep = ~(maybe & ~sure)                                         # but for samples reached only from S/N within 1e-4 of tol
    _, _, meds = RFI.narrow(xa, chans, tol, replace=False)
    xr = RFI.apply_broad(xa, chans, meds, flags)
    assert flags[300] and flags[1500:1503].all() and flags[2700:2706].all()
    assert np.array_equal(xb[:, keep], xr[:, keep])
    assert sure.sum() <= info["n_broad_samples"] <= maybe.sum()


def _effect_block():
    """256 channels x 4096 samples of Gaussian codes, sigma 8 about 127, every sixteenth channel (8, 24, ..) sigma 32; a
    pulse of 4 samples x 14 codes at DM 20 from sample 2000 on"""
    nchan, T = 256, 4096
    g = synth.gauss(91, T * nchan).reshape(T, nchan)
    sig = np.full(nchan, 8.0)
    loud = np.arange(8, nchan, 16)
    sig[loud] = 32.0
    v = g * sig[None, :] + 127.0
    f = np.float64(np.float32(FCH1)) + np.float64(np.float32(FOFF)) * np.arange(nchan)
    delay = np.floor(4.148808e3 * 20.0 * (f ** -2 - f[0] ** -2) / np.float64(np.float32(search.TSAMP)) + 0.5).astype(int)
    rows = 2000 + delay[None, :] + np.arange(4)[:, None]
    v[rows, np.broadcast_to(np.arange(nchan), rows.shape)] += 14.0
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8), loud


def test_noisy_channels_flagged_and_the_pulse_gains():
    """One sixteenth of the channels at 4 x sigma: the series' variance is 15/16 + 16/16 = 1.94 times the clean one, the
    rms 1.39 times; flagging them removes 1/16 of the signal, so the expected gain is 1.39 x 15/16 = 1.30.  The bound of
    1.2 leaves room for the clipped-rms estimator and the noise under the pulse.  FAILS WITHOUT THE FEATURE."""
    x, loud = _effect_block()
    kw = dict(nchan=256, max_samples=4096, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_min=0.0, dm_max=40.0, dm_step=2.0,
              boxcar_max=16, zap=())

    def pulse(r):
        w = r["snr"][10, 1996:2005]                                 # DM 20 is trial 10
        return float(w.max())

    with search.Searcher(**kw) as s:
        off = pulse(s.run(x))
        s.set_rfi_chan()                                            # the defaults: radius 0, tol 4
        on = pulse(s.run(x))
        info = s.rfi_chan_info()
    print("S/N off %.2f on %.2f ratio %.3f flagged %s" % (off, on, on / off, np.nonzero(info["mask"])[0].tolist()))
    assert 30 < off < 50
    assert np.nonzero(info["mask"])[0].tolist() == loud.tolist() and info["nflag"] == 16
    assert on >= 1.2 * off, (on, off)


def test_off_means_off():
    x, _ = _effect_block()
    kw = dict(nchan=256, max_samples=4096, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_min=0.0, dm_max=40.0, dm_step=2.0,
              boxcar_max=16, zap=((0, 10),))
    zero = dict(nflag=0, ms=0.0)

    def outputs(s):
        r = s.run(x, want_series=True)
        i = s.rfi_chan_info()
        assert {k: i[k] for k in zero} == zero and not any(i[k].any() for k in KEYS)
        return [r[k].tobytes() for k in ("snr", "width_log2", "series", "stats")] + [s.fetch_clean().tobytes()]

    with search.Searcher(**kw) as a:
        never = outputs(a)
    with search.Searcher(**kw) as b:
        b.set_rfi_chan()
        r = b.run(x)
        assert b.rfi_chan_info()["nflag"] > 0 and r["snr"].tobytes() != never[0]
        b.set_rfi_chan(tol=0)
        again = outputs(b)
    with search.Searcher(**kw) as c:
        c.set_rfi_chan(tol=0)                                       # off on a handle where it was never on
        fresh = outputs(c)
    assert again == never and fresh == never


def test_refusals_change_nothing():
    x = block(70, 1000, GEO[100][0])
    with handle(100, 1000) as s:
        s.set_rfi_chan(7, 3.0)
        s.run(x)
        before = check(s, x, 7, 3.0)
        for radius, tol, word in ((-1, 4.0, "radius"), (101, 4.0, "radius"), (0, float("nan"), "tol"), (0, float("inf"), "tol"),
                                  (0, -1.0, "tol")):
            with pytest.raises(ValueError, match=word):
                s.set_rfi_chan(radius, tol)
            assert s._L.pb_search_set_rfi_chan(s._s, radius, tol) == -22
        s.run(x)
        after = check(s, x, 7, 3.0)                                 # still radius 7, tol 3
        s.set_rfi_chan(100, 3.0)                                    # radius == nact is accepted
        s.run(x)
        check(s, x, 100, 3.0)
    assert before["nflag"] == after["nflag"] > 0


def _stream():
    """test_gpu_search_stream's 8-bit stream with channel 30 loud in its second half only and channel 50 in its first"""
    x = np.array(stream4(8)[0])
    rng = np.random.default_rng(9)
    x[LEN4 // 2:, 30] = rng.integers(0, 256, LEN4 - LEN4 // 2)
    x[:LEN4 // 2, 50] = rng.integers(0, 256, LEN4 // 2)
    return x


def _masks(log):
    return [(first, {k: v for k, v in info.items() if k != "ms"}) for first, info in log]


def test_streaming_equals_whole_gulps_and_masks_are_per_gulp():
    x = _stream()
    with searcher(NCH4) as s:
        s.set_rfi_chan()
        g = search.GulpSearch(s, threshold=7.0)
        ref, ref_log = [], []
        for i in range(0, LEN4, N):
            ref += g.push(x[i:i + N])
            ref_log += _masks(g.chan_log)
        ref += g.finish()
        assert g.chan_log == []                                     # finish() searches no block
    assert len(ref_log) == 4 and len(ref) >= 2
    m = np.array([info["mask"] for _, info in ref_log])
    assert m[0, 50] == 1 and m[0, 30] == 0 and m[3, 30] == 1 and m[3, 50] == 0     # each gulp's own mask
    pieces, off = [], 0
    rng = np.random.default_rng(42)
    while off < LEN4:
        pieces.append(min(int(rng.integers(1, 701)), LEN4 - off))
        off += pieces[-1]
    with searcher(NCH4) as s:
        s.set_rfi_chan()
        g = search.GulpSearch(s, threshold=7.0, gulp=N)
        got, log, off = [], [], 0
        for n in pieces:
            got += g.feed(x[off:off + n])
            log += _masks(g.chan_log)
            off += n
        got += g.finish()                                           # (searches the remainder first)
        log += _masks(g.chan_log)
    same(got, ref)
    same(log, ref_log)


def test_the_tail_handed_on_is_raw():
    x = _stream()[:900]
    with searcher(NCH4) as s:
        keep = s.max_delay + 7
        s.set_rfi_chan()
        s.set_gulp(keep)
        s.push(x)
        p1 = s.gulp_peaks(7.0)
        i1 = s.rfi_chan_info()
        clean = s.fetch_clean()
        assert i1["mask"][50] == 1 and (clean[50] == i1["fill"][50]).all()
        check(s, x, 0, 4.0)
        p2 = s.gulp_peaks(7.0)                                      # the same block again: the first call's mask and bytes
        i2 = s.rfi_chan_info()
        assert all(np.array_equal(i1[k], i2[k]) for k in KEYS) and i2["nflag"] == i1["nflag"] and i2["ms"] == i1["ms"]
        assert np.array_equal(s.fetch_clean(), clean) and p1["total"] == p2["total"]
        with pytest.raises(libpb.PbError, match="cleaned in place"):
            s.push(x[:1])
        s.gulp_advance(keep)
        assert np.array_equal(s.gulp_fetch(), x.T[:, 900 - keep:])  # channel 50's tail is the file's, not the fill


def test_polarisation_planes_stay_what_the_file_held():
    nchan, nsamp = 96, 2500
    rng = np.random.default_rng(12)
    x = P.quantise8(rng.standard_normal((nsamp, 4, nchan)))
    x[:, :, 40] = rng.integers(0, 256, (nsamp, 4))
    kw = dict(nchan=nchan, fch1=384.0, foff=-0.5, tsamp=781.25e-6, dm_min=0.0, dm_max=60.0, dm_step=2.0, boxcar_max=64,
              zap=((0, 3), (90, 96)))
    p4, xt = P.planes(x)
    with search.Searcher(max_samples=nsamp, **kw) as s:
        s.set_pol(max_cands=4)
        s.set_rfi_chan()
        s.run(x)
        ref = R.stage(xt, s.chans, nsamp, 0, 4.0)
        assert ref["mask"][40] == 1 and np.array_equal(s.fetch_clean(), ref["xt"])
        assert np.array_equal(s.rfi_chan_info()["mask"], ref["mask"])
        for k in range(4):
            assert np.array_equal(s.pol_fetch(k), p4[k]), k


def test_cli_writes_the_chans_file(tmp_path, capsys):
    x = _stream()
    fil = tmp_path / "s8.fil"
    fil.write_bytes(fil_header(NCH4, 8) + x.tobytes())
    out = tmp_path / "cands"
    common = ["-f", str(fil), "-dm", "0", "1000", "-dm_step", "100", "-boxcar_max", "8", "-nsamps_gulp", str(N),
              "-detect_thresh", "7", "-zap_chans", "5", "9", "-baseline_length", "0", "-output_dir", str(out)]
    run_main(capsys, common)
    assert not [f for f in os.listdir(out) if f.endswith(".chans")]
    run_main(capsys, common + ["-rfi_chan", "-rfi_chan_tol", "4.5"])
    def when(f):                                                    # <UTC>_<beam> or, later in the same second, <UTC>.<first sample>_<beam>
        stem = f[:-len("_01.chans")]
        return (stem[:19], int(stem[20:]) if len(stem) > 19 else -1)

    files = sorted((f for f in os.listdir(out) if f.endswith(".chans")), key=when)
    assert len(files) == 4                                          # one per gulp searched, the remainder among them
    seen = []
    for f in files:
        lines = open(out / f).read().splitlines()
        head = lines[0].split()
        assert head[0] == "#" and int(head[1]) == len(lines) - 1 and head[2:] == ["60", "0", "4.5"]
        rows = [[int(v) for v in l.split()] for l in lines[1:]]
        assert all(len(r) == 4 and r[1] > 0 and 0 <= r[2] <= 255 and r[3] > 0 for r in rows)
        seen.append([r[0] for r in rows])
    assert 50 in seen[0] and 30 not in seen[0] and 30 in seen[-1] and 50 not in seen[-1]
