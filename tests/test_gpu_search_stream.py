"""The streaming stage of the search on the GPU (pb_search_set_gulp / push / gulp_peaks / gulp_advance,
GulpSearch(gulp=N).feed, search -stream_chunk): every criterion is equality.

  * the accumulated block equals the unpacked concatenation of the pieces (tests/search_rfi_ref.unpack), whatever their
    lengths, bit widths, memory and address;
  * the advance hands on the RAW tail, also where it overlaps its destination and where the gulp was cleaned in place;
  * a stream fed in pieces gives the candidates -- dicts, lines, cutouts, refinements, what goes to the coincidencer --
    of the same stream pushed in whole host gulps of unpacked values (GulpSearch(gulp=None).push, the path that existed
    before), however it is cut.

Geometries: the smallest that reach each branch of the append -- 64 channels (one tile), 72 (a 2-bit row of 18 bytes:
the byte path), 192 (rows of 48 / 96 / 192 bytes: a ragged last tile of the 16-byte path), 4096 (many tiles); a band and
a DM range that give a largest delay of 100 to 300 samples; gulps of 512 new samples."""
import functools
import importlib

import numpy as np
import pytest

from helpers import libpb, make_input
from search_rfi_ref import pack, unpack

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")

N = 512


def _f32(v):
    return float(np.float32(v))


FCH1, FOFF, TSAMP = _f32(search.FCH1), _f32(search.FOFF), _f32(search.TSAMP)
GRID = {64: (1000, 100), 72: (1000, 100), 192: (400, 50), 4096: (20, 2)}
ZAP = {64: ((5, 9),), 72: ((5, 9),), 192: ((40, 47),), 4096: search.HEIMDALL_ZAP}


def searcher(nchan, max_samples=2048, boxcar_max=8):
    s = search.Searcher(nchan=nchan, max_samples=max_samples, fch1=FCH1, foff=FOFF, tsamp=TSAMP, dm_min=0,
                        dm_max=GRID[nchan][0], dm_step=GRID[nchan][1], boxcar_max=boxcar_max, zap=ZAP[nchan])
    assert 100 <= s.max_delay <= 300, s.max_delay
    return s


def values(seed, nsamp, nchan, nbit):
    return np.random.default_rng(seed).integers(0, 1 << nbit, (nsamp, nchan)).astype(np.uint8)


def to_device(codes, odd):
    """packed bytes -> (tensor that owns them, device address): 256-byte aligned, or one byte past that"""
    import torch
    dev = torch.zeros(codes.size + 1, dtype=torch.uint8, device="cuda")
    dev[int(odd):int(odd) + codes.size] = torch.from_numpy(np.ascontiguousarray(codes)).cuda()
    torch.cuda.synchronize()                               # the search's stream waits for no other
    ptr = dev.data_ptr() + int(odd)
    assert ptr % 16 == (1 if odd else 0)
    return dev, ptr


def point_set(pk):
    assert pk["total"] == pk["dmi"].size
    return (pk["tout"], sorted(zip(pk["dmi"].tolist(), pk["t"].tolist(), pk["snr"].view(np.uint32).tolist(),
                                   pk["width_log2"].tolist())))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the append

PIECES = (3, 63, 127, 1280, 3, 3, 3, 64, 3, 1, 1, 65, 65, 1)        # every length of {1, 3, 63, 64, 65, 127, 1280}
FILLS = np.cumsum((0,) + PIECES[:-1])


def test_the_piece_order_meets_every_alignment():
    assert set(PIECES) == {1, 3, 63, 64, 65, 127, 1280}
    assert {0, 1, 3, 4, 15, 16, 17} <= set(int(f) % 64 for f in FILLS)
    assert {0, 1, 3, 4, 15} <= set(int(f) % 16 for f in FILLS)


@pytest.mark.parametrize("nbit", [8, 4, 2])
@pytest.mark.parametrize("nchan", [64, 72, 192, 4096])
def test_append_equals_the_unpacked_concatenation(nchan, nbit):
    total = sum(PIECES)
    x = values(1000 + nchan + nbit, total, nchan, nbit)
    codes = pack(x, nbit)
    rowb = nchan * nbit // 8
    assert np.array_equal(unpack(codes, total, nchan, nbit), x)
    with searcher(nchan) as s:
        s.set_gulp(s.max_delay + 7)
        for where in ("host", "device", "device, odd address"):
            if where != "host":
                keep, ptr = to_device(codes, where != "device")
            fill = 0
            for n in PIECES:
                if where == "host":
                    got = s.push(codes[fill * rowb:(fill + n) * rowb], nbit=nbit)
                else:
                    got = s.push(nbit=nbit, device_ptr=ptr + fill * rowb, nsamp=n)
                fill += n
                assert got == fill
                if n == 1280 or fill == total or fill < 200:
                    assert np.array_equal(s.gulp_fetch(), x[:fill].T), (where, fill)
            assert s.gulp_timers()["append"] > 0
            s.gulp_advance(0)
            assert s.gulp_fill() == 0


@pytest.mark.parametrize("nchan", [64, 192])
def test_append_of_mixed_bit_widths(nchan):
    rng = np.random.default_rng(77)
    parts, fill = [], 0
    with searcher(nchan) as s:
        s.set_gulp(16)
        for i, n in enumerate((65, 1, 127, 3, 64, 63, 200, 5, 17)):
            nbit = (8, 4, 2)[i % 3]
            x = values(2000 + i, n, nchan, nbit)
            if rng.integers(2):
                keep, ptr = to_device(pack(x, nbit), i % 2)
                fill = s.push(nbit=nbit, device_ptr=ptr, nsamp=n)
            else:
                fill = s.push(pack(x, nbit), nbit=nbit)
            parts.append(x)
            assert np.array_equal(s.gulp_fetch(), np.concatenate(parts).T), i
        assert fill == sum(p.shape[0] for p in parts)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the advance

@pytest.mark.parametrize("nchan,nbit", [(64, 8), (192, 2), (4096, 4)])
def test_advance_hands_on_the_raw_tail(nchan, nbit):
    fill = 301
    x = values(3000 + nchan, fill, nchan, nbit)
    more = values(3001 + nchan, 130, nchan, nbit)
    with searcher(nchan) as s:
        s.set_gulp(fill)
        for keep in (0, 1, 77, 200, fill):                  # 200 > fill - 200: source and destination overlap
            assert s.push(pack(x, nbit), nbit=nbit) == fill
            assert np.array_equal(s.gulp_fetch(), x.T)
            s.gulp_advance(keep)
            assert s.gulp_fill() == keep
            assert np.array_equal(s.gulp_fetch(), x[fill - keep:].T), keep
            assert s.push(pack(more, nbit), nbit=nbit) == keep + 130
            assert np.array_equal(s.gulp_fetch(), np.concatenate([x[fill - keep:], more]).T), keep
            s.gulp_advance(0)


def test_a_short_stream_after_a_long_one_equals_a_fresh_handle():
    nchan = 192
    long_, short = np.full((2000, nchan), 255, np.uint8), values(3100, 400, nchan, 2)
    with searcher(nchan) as s:
        s.set_gulp(64)
        s.push(long_)
        s.gulp_run()
        s.gulp_advance(0)
        s.push(pack(short, 2), nbit=2)
        a = s.gulp_run(want_series=True)
        pa = s.gulp_peaks(3.0)
    with searcher(nchan) as fresh:
        fresh.set_gulp(64)
        fresh.push(pack(short, 2), nbit=2)
        b = fresh.gulp_run(want_series=True)
        pb = fresh.gulp_peaks(3.0)
    assert a["tout"] == b["tout"] == 400 - s.max_delay
    for k in ("snr", "stats", "series", "width_log2"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert pa["total"] > 0 and point_set(pa) == point_set(pb)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the raw tail under cleaning

def test_cleaning_leaves_the_raw_tail_to_the_advance():
    nchan, fill = 192, 900
    rng = np.random.default_rng(3200)
    x = np.clip(rng.normal(128, 12, (fill, nchan)), 0, 255).astype(np.uint8)
    with searcher(nchan) as s:
        keep = s.max_delay + 7
        x[fill - keep + 5:fill - 3:11, 60] = 255             # channel outliers inside the tail
        x[fill - 40:fill - 38, :] = np.minimum(x[fill - 40:fill - 38, :].astype(np.int32) + 60, 255).astype(np.uint8)  # an impulse
        s.set_rfi(True, True, 5.0)
        s.set_gulp(keep)
        s.push(x)
        assert np.array_equal(s.gulp_fetch(), x.T)
        p1 = s.gulp_peaks(3.0)
        clean = s.fetch_clean()
        info = s.rfi_info()
        assert info["n_narrow"] > 0 and info["n_broad_samples"] > 0
        tail = slice(fill - keep, fill)
        assert clean.shape == (nchan, fill) and not np.array_equal(clean[:, tail], x.T[:, tail])
        assert (clean[60, tail] != x.T[60, tail]).any() and (clean[:, fill - 40] != x[fill - 40]).any()
        p2 = s.gulp_peaks(3.0)                                 # the same block again: the same bytes
        assert p1["total"] > 0 and point_set(p1) == point_set(p2)
        assert np.array_equal(s.fetch_clean(), clean) and s.rfi_info()["n_narrow"] == info["n_narrow"]
        # the block path on the same samples: the gulp was searched as a block is
        with searcher(nchan) as b:
            b.set_rfi(True, True, 5.0)
            assert point_set(b.peaks(x, 3.0)) == point_set(p1) and np.array_equal(b.fetch_clean(), clean)
        with pytest.raises(libpb().PbError, match="cleaned in place"):
            s.push(x[:1])
        s.gulp_advance(keep)
        assert np.array_equal(s.gulp_fetch(), x.T[:, tail])
        s.push(x[:100])
        assert np.array_equal(s.gulp_fetch(), np.concatenate([x[tail], x[:100]]).T)


# ---------------------------------------------------------------------------------------------------------------------
# 4. equal however the stream is cut

NCH4, LEN4 = 64, 3 * N + 177
PULSES = ((300, 8), (1000, 5), (1400, 8), (None, 10))    # (first sample, trial DM): 1000 sweeps across sample 2 N; None: the
                                                         # stream's last output samples, which only finish() reports


@functools.lru_cache(maxsize=None)
def stream4(nbit):
    """a seeded stream of three gulps and a remainder, values below 2^nbit: noise, four dispersed pulses (one whose sweep
    straddles sample 1024, one in the stream's last samples), outliers in one channel and a broadband impulse"""
    rng = np.random.default_rng(4000 + nbit)
    top = (1 << nbit) - 1
    mid, sig, amp = {8: (128, 20.0, 40), 4: (7.5, 2.0, 4), 2: (1.5, 1.0, 2)}[nbit]
    x = np.clip(np.floor(rng.normal(mid, sig, (LEN4, NCH4)) + 0.5), 0, top).astype(np.int32)
    with searcher(NCH4) as s:
        dms, md = np.asarray(s.dms), s.max_delay
    import search_cutout_ref as CR
    for t0, which in PULSES:
        dm = dms[which]
        t0 = LEN4 - md - 4 if t0 is None else t0
        sweep = CR.delays([dm], FCH1, FOFF, NCH4, TSAMP)[0]
        rows = np.minimum(t0 + sweep[None, :] + np.arange(2)[:, None], LEN4 - 1)
        x[rows, np.broadcast_to(np.arange(NCH4), rows.shape)] += amp
    assert 1000 < 2 * N < 1000 + CR.delays([dms[5]], FCH1, FOFF, NCH4, TSAMP)[0].max()
    x[700:1500:37, 20] = top
    x[1200:1202] += amp
    x = np.clip(x, 0, top).astype(np.uint8)
    x.setflags(write=False)
    return x, md


MODES = ("points", "giants", "all on")


def gulper(s, mode, gulp):
    kw = {}
    if mode == "giants":
        kw["giants"] = {}
    if mode == "all on":
        s.set_rfi(True, True, 5.0)
        s.set_cutouts(nsub=8, nt=32, ndmrow=8, max_cands=8)
        s.set_refine(nstep=8, half_window=64, wmax=8, max_cands=8)
        kw.update(cutouts=dict(thresh=7.0, max_per_gulp=8), refine=dict(thresh=7.0, max_per_gulp=8))
    g = search.GulpSearch(s, threshold=7.0, gulp=gulp, **kw)
    g.sent = []
    g._send = lambda cands, first, nsamps: g.sent.append((first, nsamps, g.last_first, [search.candidate_line(c) for c in cands]))
    return g


def same(a, b):
    """candidates, or anything they hold, equal value by value (NaN equal to NaN)"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b)
        for k in a:
            same(a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b)
        for u, v in zip(a, b):
            same(u, v)
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    elif isinstance(a, float) and a != a:
        assert b != b
    else:
        assert type(a) is type(b) and a == b, (a, b)


@functools.lru_cache(maxsize=None)
def reference4(nbit, mode):
    """GulpSearch(gulp=None).push of whole gulps of the unpacked values, the remainder last, then finish()"""
    x, _ = stream4(nbit)
    with searcher(NCH4) as s:
        g = gulper(s, mode, None)
        per_call = [g.push(x[i:i + N]) for i in range(0, LEN4, N)] + [g.finish()]
        done = g.done
    assert sum(1 for c in per_call[:-1] if c) >= 2           # candidates in at least two gulps
    return [c for call in per_call for c in call], g.sent, done


@pytest.mark.parametrize("nbit", [8, 4, 2])
@pytest.mark.parametrize("mode", MODES)
def test_equal_however_the_stream_is_cut(mode, nbit):
    x, md = stream4(nbit)
    ref, sent, done = reference4(nbit, mode)
    if mode == "all on":
        assert any("cutout" in c for c in ref) and any(c.get("refined") for c in ref)
    codes = pack(x, nbit)
    rowb = NCH4 * nbit // 8
    rng = np.random.default_rng(41)
    cut_random = []
    while sum(cut_random) < LEN4:
        cut_random.append(min(int(rng.integers(1, 701)), LEN4 - sum(cut_random)))
    exact = [N] * (LEN4 // N) + [LEN4 % N]
    keep, ptr = to_device(codes, nbit == 4)
    for name, pieces, dev in (("random", cut_random, False), ("gulps", exact, False), ("one piece", [LEN4], False),
                              ("device", cut_random[::-1], True), ("empty pieces", [0, 700, 0, 700, LEN4 - 1400, 0], False)):
        with searcher(NCH4) as s:
            g = gulper(s, mode, N)
            got, off = [], 0
            for n in pieces:
                if dev:
                    got += g.feed(nbit=nbit, device_ptr=ptr + off * rowb, nsamp=n)
                else:
                    got += g.feed(codes[off * rowb:(off + n) * rowb], nbit=nbit)
                off += n
            got += g.finish()
            assert g.done == done, name
        assert len(got) == len(ref), name
        same(got, ref)
        assert [search.candidate_line(c) for c in got] == [search.candidate_line(c) for c in ref], name
        assert g.sent == sent, name


def test_feed_refuses_what_it_cannot_cut():
    with searcher(64) as s:
        g = search.GulpSearch(s, gulp=N)
        with pytest.raises(ValueError):
            g.feed(np.zeros(64, np.uint8), nbit=3)
        with pytest.raises(ValueError):
            g.feed(nbit=8, device_ptr=1024)
        with pytest.raises(ValueError):
            search.GulpSearch(s).feed(np.zeros(64, np.uint8))
    s = search.Searcher(nchan=3, max_samples=256, fch1=FCH1, foff=FOFF, tsamp=TSAMP, dm_min=0, dm_max=10, dm_step=5, zap=())
    with s:
        with pytest.raises(ValueError, match="whole bytes"):
            search.GulpSearch(s, gulp=N).feed(np.zeros(3, np.uint8), nbit=2)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the chain: pb_process batches fed from device memory

R5, S5 = 64, 16
T5 = R5 * S5 // 8                   # 128 samples of 4096 channels per batch


@pytest.mark.parametrize("nbit", [2, 8])
def test_batches_of_pb_process_fed_where_they_lie(nbit):
    lp = libpb()
    nco, gulp, nbatch = 4096, 100, 3
    kw = dict(nchan=nco, max_samples=512, fch1=FCH1, foff=FOFF, tsamp=TSAMP, dm_min=0, dm_max=6, dm_step=2, boxcar_max=4,
              zap=search.HEIMDALL_ZAP)
    host, fed = [], []
    with lp.PbHandle(nbit=nbit, rfi_mode=2, rows_per_seg=R5, max_seg=S5) as h, search.Searcher(**kw) as s:
        g = search.GulpSearch(s, threshold=1.0, gulp=gulp)
        for b in range(nbatch):
            data = make_input(500 + nbit + b, R5, S5)
            for sg in range(S5):
                h.submit_planar(0, sg, data[sg, 0], data[sg, 1])
            h.process(S5)
            h.sync()
            dev, _ = h.output_dev(0, 1)
            fed += g.feed(nbit=nbit, device_ptr=dev, nsamp=T5)
            host.append(unpack(h.fetch(0, 0, S5, raw=False)["kur"], T5, nco, nbit).copy())
        fed += g.finish()
        done = g.done
    x = np.concatenate(host)
    with search.Searcher(**kw) as s:
        g = search.GulpSearch(s, threshold=1.0)
        ref = [c for i in range(0, x.shape[0], gulp) for c in g.push(x[i:i + gulp])] + g.finish()
        assert g.done == done == x.shape[0] - s.max_delay
    assert len(ref) > 0
    same(fed, ref)


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals and neutrality

def test_refusals_change_nothing():
    lp = libpb()
    nchan = 64
    x = values(6000, 500, nchan, 8)
    with searcher(nchan, max_samples=600) as s:
        for call in (lambda: s.push(x[:1]), lambda: s.gulp_peaks(5.0), lambda: s.gulp_run(), lambda: s.gulp_advance(0),
                     lambda: s.gulp_fetch(), lambda: s.gulp_fill()):
            with pytest.raises(lp.PbError, match="not switched on"):
                call()
        with pytest.raises(ValueError, match="keep_max"):
            s.set_gulp(601)
        s.set_gulp(300)
        s.push(x)
        before = s.gulp_fetch()
        for call, msg in ((lambda: s.push(x[:101]), "max_samples"),
                          (lambda: s.push(x[:1], nbit=3), "nbit"),
                          (lambda: s.push(x[:1], nbit=16), "nbit"),
                          (lambda: s.gulp_advance(501), "0..fill"),
                          (lambda: s.gulp_advance(-1), "0..fill"),
                          (lambda: s.gulp_advance(301), "keep_max")):
            with pytest.raises(lp.PbError, match=msg):
                call()
            assert s.gulp_fill() == 500 and np.array_equal(s.gulp_fetch(), before)
        s.gulp_advance(s.max_delay + 63)                      # too few samples for a run
        short = s.gulp_fetch()
        for call in (lambda: s.gulp_peaks(5.0), lambda: s.gulp_run()):
            with pytest.raises(lp.PbError, match="shorter than the largest dispersion delay"):
                call()
            assert np.array_equal(s.gulp_fetch(), short)
        # the block entry on a handle with the stage on: its usual result, and the stage left empty
        pk = s.peaks(x, 3.0)
        assert s.gulp_fill() == 0 and s.gulp_fetch().shape == (nchan, 0)
        s.push(x)
        assert point_set(s.gulp_peaks(3.0)) == point_set(pk)
        s.set_gulp(0)
        with pytest.raises(lp.PbError, match="not switched on"):
            s.gulp_fill()
    with searcher(nchan, max_samples=600) as never:
        assert pk["total"] > 0 and point_set(never.peaks(x, 3.0)) == point_set(pk)


def fil_header(nchan, nbits):
    sig = importlib.import_module("vlite-fast_amd.sigproc")
    return b"".join([sig.send_string("HEADER_START"), sig.send_int("data_type", 1), sig.send_double("fch1", FCH1),
                     sig.send_double("foff", FOFF), sig.send_int("nchans", nchan), sig.send_int("nbits", nbits),
                     sig.send_double("tstart", 57570 + 3600 / 86400.), sig.send_double("tsamp", TSAMP),
                     sig.send_int("nifs", 1), sig.send_string("HEADER_END")])


def run_main(capsys, argv):
    capsys.readouterr()
    n = search.main(argv)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert n == len(lines)
    return lines


def test_command_line_with_and_without_stream_chunk(tmp_path, capsys):
    x, _ = stream4(2)
    for nbits in (8, 2):
        with open(tmp_path / ("s%d.fil" % nbits), "wb") as f:
            f.write(fil_header(NCH4, nbits))
            f.write(pack(x, nbits).tobytes())
    common = ["-dm", "0", "1000", "-dm_step", "100", "-boxcar_max", "8", "-nsamps_gulp", str(N), "-detect_thresh", "7",
              "-zap_chans", "5", "9", "-baseline_length", "0"]
    plain = run_main(capsys, ["-f", str(tmp_path / "s8.fil")] + common)
    assert len(plain) >= 3
    assert run_main(capsys, ["-f", str(tmp_path / "s8.fil"), "-stream_chunk", "1280"] + common) == plain
    assert run_main(capsys, ["-f", str(tmp_path / "s8.fil"), "-stream_chunk", "77"] + common) == plain
    assert run_main(capsys, ["-f", str(tmp_path / "s2.fil"), "-stream_chunk", "1280"] + common) == plain
    with pytest.raises(SystemExit, match="8-bit single-IF"):
        search.main(["-f", str(tmp_path / "s2.fil")] + common)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the workload's own shape, once

def test_production_geometry_fed_by_the_second(tmp_path, capsys):
    import search_cutout_ref as CR
    nchan, gulp = 4096, search.HEIMDALL_GULP
    length = gulp + 12 * 1280                                # a gulp and a partial one
    dm, t0 = 500.0, gulp - 2000                              # the sweep (~5690 samples) crosses sample 30 720
    dml = search.dedisp_dm_list(2.0, 1000.0, TSAMP, FCH1, FOFF, nchan)
    rng = np.random.default_rng(71)
    x = rng.integers(0, 4, (length, nchan), dtype=np.uint8)
    x[x == 3] = rng.integers(0, 3, int((x == 3).sum()), dtype=np.uint8)         # keep headroom below the top code
    sweep = CR.delays([dm], FCH1, FOFF, nchan, TSAMP)[0]
    assert t0 + sweep[190] < gulp < t0 + sweep[3899]
    rows = t0 + sweep[None, :] + np.arange(4)[:, None]
    x[rows, np.broadcast_to(np.arange(nchan), rows.shape)] += 1
    codes = pack(x, 2)
    with open(tmp_path / "p2.fil", "wb") as f:
        f.write(fil_header(nchan, 2))
        f.write(codes.tobytes())
    maxs = gulp + int(4.148808e3 * 1000.0 * abs((FCH1 + (nchan - 1) * FOFF) ** -2 - FCH1 ** -2) / TSAMP) + 64

    def make(gulp_arg):
        s = search.Searcher(max_samples=maxs, fch1=FCH1, foff=FOFF, tsamp=TSAMP, dm_list=dml)
        s.set_baseline(int(2.0 / TSAMP))
        s.set_rfi(True, True, 5.0)
        s.set_cutouts(nsub=64, nt=min(256, (maxs // 64) & ~1), max_cands=32)
        s.set_refine(half_window=max(64, min(128, (maxs // 4) & ~1)), max_cands=32)
        return s, search.GulpSearch(s, threshold=7.0, giants=dict(sep_time=3, sep_dm=200, sep_filter=3, max_giants=1 << 18),
                                    cutouts=dict(thresh=7.0, max_per_gulp=32), refine=dict(thresh=7.0, max_per_gulp=32),
                                    gulp=gulp_arg)

    s, g = make(None)
    with s:
        ref = g.push(x[:gulp]) + g.push(x[gulp:]) + g.finish()
    del g
    strongest = min(ref, key=lambda c: (-c["snr"], c["dmi"], c["peak_idx"]))
    assert abs(strongest["dm"] - dm) < 10 and abs(strongest["peak_idx"] - t0) <= 4 and "cutout" in strongest
    rowb = nchan // 4
    s, g = make(gulp)
    with s:
        fed = []
        for i in range(0, length, 1280):
            fed += g.feed(codes[i * rowb:(i + 1280) * rowb], nbit=2)
        fed += g.finish()
        tm = s.gulp_timers()
    print("production geometry: %d candidates, strongest %s; last push and advance %s" % (len(fed), search.candidate_line(strongest), tm))
    same(fed, ref)
    lines = run_main(capsys, ["-f", str(tmp_path / "p2.fil"), "-stream_chunk", "1280", "-detect_thresh", "7", "-zap_chans", "0", "190",
                              "-zap_chans", "3900", "4096", "-giants", "-rfi_clean", "-cutouts", "-refine", "-output_dir",
                              str(tmp_path / "cands")])
    assert lines == [search.candidate_line(c) for c in ref]
