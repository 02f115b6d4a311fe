"""The fp32 entry of the streaming search on the GPU (pb_search_push_f32, Searcher.push_plane, GulpSearch.feed_plane,
process_baseband --search): every criterion is equality.

  (a) the accumulated block equals the NumPy restatement (tests/search_plane_ref.py, pinned to the oracle's sel_and_dig_8b
      by tests/test_search_plane_cpu.py) of the concatenated pieces, for every alignment of the block's fill, host and
      device planes, both load paths and two scales;
  (b) planes and codes of 8, 4 and 2 bits pushed in turn make one block;
  (c) every refusal leaves the block as it was, and a handle that has used the entry searches like one that never did;
  (d) pb_process's fp32 plane of an nbit = 2 handle fed through feed_plane gives the blocks and candidates of an nbit = 8
      handle's codes fed through feed;
  (e) a coadder's sum pushed with scale 1/sqrt(N) gives the block of pb_coadd_digitise's 8-bit codes;
  (f) the reference's self-test pulse has, from the plane of a 2-bit handle, exactly the S/N of an 8-bit handle's codes
      and more than from the 2-bit codes;
  (g) process_baseband -b 2 --search writes the candidate files of -b 8 followed by search -f, and the .fil files of a
      run without --search.

Geometries of (a): 64 channels (one tile), 66 (rows of 264 bytes: scalar loads), 72, 192 (three tiles of the float4
path), 4096; max_samples 2048."""
import importlib
import os

import numpy as np
import pytest

import search_plane_ref as PR
from helpers import libpb, make_input
from search_rfi_ref import pack
from test_gpu_search_stream import FCH1, FOFF, TSAMP, point_set, same

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")

GRID = {64: (1000, 100), 66: (1000, 100), 72: (1000, 100), 192: (400, 50), 4096: (20, 2)}
ZAP = {64: ((5, 9),), 66: ((5, 9),), 72: ((5, 9),), 192: ((40, 47),), 4096: search.HEIMDALL_ZAP}
SCALES = (np.float32(1.0), np.float32(1.0 / np.sqrt(2.0)))


def searcher(nchan, max_samples=2048, boxcar_max=8):
    return search.Searcher(nchan=nchan, max_samples=max_samples, fch1=FCH1, foff=FOFF, tsamp=TSAMP, dm_min=0,
                           dm_max=GRID[nchan][0], dm_step=GRID[nchan][1], boxcar_max=boxcar_max, zap=ZAP[nchan])


def plane_to_device(plane, odd):
    """float32 values -> (tensor that owns them, device address): 256-byte aligned, or 4 bytes past that"""
    import torch
    flat = np.ascontiguousarray(plane, np.float32).ravel()
    dev = torch.zeros(flat.size + 1, dtype=torch.float32, device="cuda")
    dev[int(odd):int(odd) + flat.size] = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()                               # the search's stream waits for no other
    ptr = dev.data_ptr() + 4 * int(odd)
    assert ptr % 16 == (4 if odd else 0)
    return dev, ptr


def codes_to_device(codes):
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(codes)).cuda()
    torch.cuda.synchronize()
    return dev, dev.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# (a) the block

# 63 pieces of 1, 65 or 129 samples, each one more than a multiple of 64: the fill goes through every value mod 64
STEPS = tuple(p for _, p in sorted(zip([i * 37 % 63 for i in range(63)], (129,) * 8 + (65,) * 15 + (1,) * 40)))
LONG = (130, 127, 64, 65, 129, 128, 1, 100, 63, 130, 2, 66, 130, 126, 130, 130, 130, 130, 8, 130, 129)
PASSES = (STEPS, LONG)


def test_the_piece_order_meets_every_alignment():
    fills = np.cumsum((0,) + STEPS)
    assert set(int(f) % 64 for f in fills) == set(range(64)) and STEPS[:4] != tuple(sorted(STEPS[:4], reverse=True))
    assert all(1 <= n <= 130 for p in PASSES for n in p) and {1, 2, 8, 63, 64, 65, 66, 127, 128, 129, 130} <= set(STEPS + LONG)
    assert all(sum(p) <= 2048 for p in PASSES) and sum(LONG) > 1900
    fl = np.cumsum((0,) + LONG[:-1])
    assert len(set(int(f) % 16 for f in fl)) >= 8 and any(f % 64 + n > 128 for f, n in zip(fl, LONG))   # three tiles


@pytest.mark.parametrize("nchan", [64, 66, 72, 192, 4096])
def test_block_equals_the_restatement(nchan):
    with searcher(nchan) as s:
        s.set_gulp(16)
        for ip, pieces in enumerate(PASSES):
            total = sum(pieces)
            x = PR.test_values(7000 + nchan + ip, total * nchan).reshape(total, nchan)
            assert np.isnan(x).any() and np.isinf(x).any()
            for where in ("host", "device", "device + 4 bytes"):
                if where != "host":
                    keep, ptr = plane_to_device(x, where != "device")
                for scale in SCALES:
                    want = PR.quantise8(x, scale)
                    fill = 0
                    for n in pieces:
                        if where == "host":
                            got = s.push_plane(x[fill:fill + n], scale=scale)
                        else:
                            got = s.push_plane(device_ptr=ptr + 4 * fill * nchan, nsamp=n, scale=scale)
                        fill += n
                        assert got == fill
                        if fill < 70 or fill == total or n == 130:
                            assert np.array_equal(s.gulp_fetch(), want[:fill].T), (where, float(scale), fill)
                    tm = s.gulp_timers()
                    assert tm["append"] > 0 and (tm["copy"] > 0 or where != "host")
                    s.gulp_advance(0)
                    assert s.gulp_fill() == 0


def test_a_host_plane_longer_than_a_staging_slice():
    """max_samples = 256: a host plane goes through the staging buffer in slices of 64 samples"""
    nchan = 72
    x = PR.test_values(7100, 250 * nchan).reshape(250, nchan)
    with searcher(nchan, max_samples=256) as s:
        s.set_gulp(16)
        assert s.push_plane(x[:3]) == 3 and s.push_plane(x[3:]) == 250
        assert np.array_equal(s.gulp_fetch(), PR.quantise8(x).T)


# ---------------------------------------------------------------------------------------------------------------------
# (b) planes and codes in turn

@pytest.mark.parametrize("nchan", [64, 192])
def test_planes_and_codes_in_turn(nchan):
    rng = np.random.default_rng(7200)
    parts = []
    with searcher(nchan) as s:
        s.set_gulp(16)
        for i, n in enumerate((65, 1, 127, 3, 64, 63, 130, 5, 17, 100, 33, 2)):
            kind = ("plane", 8, "plane", 4, "plane", 2)[i % 6]
            on_dev = bool(rng.integers(2))
            if kind == "plane":
                x = PR.test_values(7300 + i, n * nchan).reshape(n, nchan)
                scale = SCALES[(i // 2) % 2]
                if on_dev:
                    keep, ptr = plane_to_device(x, i % 4 == 0)
                    fill = s.push_plane(device_ptr=ptr, nsamp=n, scale=scale)
                else:
                    fill = s.push_plane(x, scale=scale)
                parts.append(PR.quantise8(x, scale))
            else:
                v = rng.integers(0, 1 << kind, (n, nchan)).astype(np.uint8)
                if on_dev:
                    keep, ptr = codes_to_device(pack(v, kind))
                    fill = s.push(nbit=kind, device_ptr=ptr, nsamp=n)
                else:
                    fill = s.push(pack(v, kind), nbit=kind)
                parts.append(v)
            assert np.array_equal(s.gulp_fetch(), np.concatenate(parts).T), i
        assert fill == sum(p.shape[0] for p in parts)


# ---------------------------------------------------------------------------------------------------------------------
# (c) refusals and neutrality

def test_refusals_change_nothing():
    lp = libpb()
    nchan = 64
    x = PR.test_values(7400, 500 * nchan).reshape(500, nchan)
    codes = np.random.default_rng(7401).integers(0, 256, (500, nchan)).astype(np.uint8)
    keep, ptr = plane_to_device(x, False)
    with searcher(nchan, max_samples=600) as s:
        with pytest.raises(lp.PbError, match="not switched on"):
            s.push_plane(x[:1])
        s.set_gulp(300)
        assert s.push_plane(x) == 500
        before = s.gulp_fetch()
        assert np.array_equal(before, PR.quantise8(x).T)
        for call, msg in ((lambda: s.push_plane(x[:101]), "max_samples"),
                          (lambda: s.push_plane(device_ptr=ptr, nsamp=101), "max_samples"),
                          (lambda: s.push_plane(device_ptr=ptr, nsamp=-1), "negative"),
                          (lambda: s.push_plane(x[:1], scale=0.0), "scale"),
                          (lambda: s.push_plane(x[:1], scale=-1.0), "scale"),
                          (lambda: s.push_plane(x[:1], scale=float("inf")), "scale"),
                          (lambda: s.push_plane(device_ptr=ptr, nsamp=1, scale=float("nan")), "scale"),
                          (lambda: s.push_plane(device_ptr=ptr + 1, nsamp=1), "multiple of 4"),
                          (lambda: s.push_plane(device_ptr=ptr + 2, nsamp=1), "multiple of 4")):
            with pytest.raises(lp.PbError, match=msg):
                call()
            assert s.gulp_fill() == 500 and np.array_equal(s.gulp_fetch(), before)
        # a block cleaned in place takes no plane either
        s.set_rfi(True, True, 5.0)
        p1 = s.gulp_peaks(3.0)
        clean = s.fetch_clean()
        with pytest.raises(lp.PbError, match="cleaned in place"):
            s.push_plane(x[:1])
        assert np.array_equal(s.fetch_clean(), clean) and point_set(s.gulp_peaks(3.0)) == point_set(p1)
        s.gulp_advance(300)
        assert np.array_equal(s.gulp_fetch(), before[:, 200:])
        s.set_rfi(False, False)
        # after all that the handle searches codes as one that never saw a plane does
        s.gulp_advance(0)
        s.push(codes)
        used = s.gulp_peaks(3.0)
        block = s.peaks(codes, 3.0)
    with searcher(nchan, max_samples=600) as never:
        never.set_gulp(300)
        never.push(codes)
        fresh = never.gulp_peaks(3.0)
        assert fresh["total"] > 0 and point_set(fresh) == point_set(used)
        assert point_set(never.peaks(codes, 3.0)) == point_set(block)


# ---------------------------------------------------------------------------------------------------------------------
# (d) through pb_process

R5, S5 = 64, 16
T5 = R5 * S5 // 8                   # 128 samples of 4096 channels per batch


@pytest.mark.parametrize("rfi_mode,stream", [(2, 1), (0, 0)])
def test_plane_of_a_2_bit_handle_equals_codes_of_an_8_bit_handle(rfi_mode, stream):
    lp = libpb()
    nco, gulp, nbatch = 4096, 100, 3
    kw = dict(nchan=nco, max_samples=512, fch1=FCH1, foff=FOFF, tsamp=TSAMP, dm_min=0, dm_max=6, dm_step=2, boxcar_max=4,
              zap=search.HEIMDALL_ZAP)
    hkw = dict(rfi_mode=rfi_mode, rows_per_seg=R5, max_seg=S5)
    fed = {"plane": [], "codes": []}
    blocks = {"plane": [], "codes": []}
    with lp.PbHandle(nbit=2, keep_ave=True, **hkw) as h2, lp.PbHandle(nbit=8, **hkw) as h8, \
            search.Searcher(**kw) as sp, search.Searcher(**kw) as sc:
        gp, gc = search.GulpSearch(sp, threshold=1.0, gulp=gulp), search.GulpSearch(sc, threshold=1.0, gulp=gulp)
        for b in range(nbatch):
            data = make_input(520 + b, R5, S5, dropped=False)
            for h in (h2, h8):
                for sg in range(S5):
                    h.submit_planar(0, sg, data[sg, 0], data[sg, 1])
                h.process(S5)
                h.sync()
            _, ave = h2.output_dev(0, stream)
            codes, _ = h8.output_dev(0, stream)
            fed["plane"] += gp.feed_plane(device_ptr=ave, nsamp=T5)
            fed["codes"] += gc.feed(nbit=8, device_ptr=codes, nsamp=T5)
            blocks["plane"].append(sp.gulp_fetch())
            blocks["codes"].append(sc.gulp_fetch())
            # and the plane is the one the restatement turns into the 8-bit handle's bytes
            out2 = h2.fetch(0, 0, S5, raw=stream == 0, kur=stream == 1, ave=True)
            out8 = h8.fetch(0, 0, S5, raw=stream == 0, kur=stream == 1)
            plane = out2["ave_kur" if stream else "ave_raw"]
            assert np.array_equal(PR.quantise8(plane), out8["kur" if stream else "raw"])
        fed["plane"] += gp.finish()
        fed["codes"] += gc.finish()
        assert gp.done == gc.done == nbatch * T5 - sp.max_delay
    for a, b in zip(blocks["plane"], blocks["codes"]):
        assert a.shape == b.shape and a.shape[1] > 0 and np.array_equal(a, b)
    assert len(fed["codes"]) > 0
    same(fed["plane"], fed["codes"])


def test_feed_and_feed_plane_alternate_on_one_stream():
    nchan, gulp = 64, 512
    n = 3 * gulp + 177
    x = PR.test_values(7500, n * nchan).reshape(n, nchan)
    q = PR.quantise8(x)
    with searcher(nchan) as s:
        g = search.GulpSearch(s, threshold=3.0, gulp=gulp)
        ref = g.feed(q) + g.finish()
        done = g.done
    with searcher(nchan) as s:
        g = search.GulpSearch(s, threshold=3.0, gulp=gulp)
        got, off = [], 0
        for i, k in enumerate((700, 1, 300, 0, 512, n - 1513)):
            got += g.feed_plane(x[off:off + k]) if i % 2 == 0 else g.feed(q[off:off + k])
            off += k
        got += g.finish()
        assert off == n and g.done == done
    assert len(ref) > 0
    same(got, ref)
    with searcher(nchan) as s:
        with pytest.raises(ValueError):
            search.GulpSearch(s).feed_plane(x[:1])
        with pytest.raises(ValueError):
            search.GulpSearch(s, gulp=gulp).feed_plane(device_ptr=1024)


# ---------------------------------------------------------------------------------------------------------------------
# (e) the coadder's use

def test_a_coadded_sum_pushed_with_its_scale():
    import torch
    lp = libpb()
    nco, T, N = 4096, 128, 3
    rng = np.random.default_rng(7600)
    total = (rng.normal(0, 1, (T, nco)).astype(np.float32) + rng.normal(0, 1, (T, nco)).astype(np.float32)
             + rng.normal(0, 1, (T, nco)).astype(np.float32))
    d_sum = torch.from_numpy(total).cuda()
    d_codes = torch.zeros(T * nco, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    scale = np.float32(1.0 / np.sqrt(3.0))
    with lp.PbHandle(nbit=8, rfi_mode=2, rows_per_seg=16, max_seg=2) as h:
        h.coadd_digitise(d_sum.data_ptr(), T * nco, N, d_codes.data_ptr())
        h.sync()
    kw = dict(nchan=nco, max_samples=256, fch1=FCH1, foff=FOFF, tsamp=TSAMP, dm_min=0, dm_max=6, dm_step=2, boxcar_max=4,
              zap=search.HEIMDALL_ZAP)
    with search.Searcher(**kw) as s:
        s.set_gulp(8)
        assert s.push_plane(device_ptr=d_sum.data_ptr(), nsamp=T, scale=scale) == T
        from_plane = s.gulp_fetch()
        s.gulp_advance(0)
        assert s.push(nbit=8, device_ptr=d_codes.data_ptr(), nsamp=T) == T
        from_codes = s.gulp_fetch()
    assert np.array_equal(from_plane, from_codes)
    assert np.array_equal(from_plane, PR.quantise8(total, scale).T) and len(np.unique(from_plane)) > 150


# ---------------------------------------------------------------------------------------------------------------------
# (f) the gain

def test_the_pulse_is_stronger_at_8_bit_depth_than_in_the_2_bit_codes(capsys):
    """The reference's self-test pulse as tests/test_gpu_chain.py sets it up (DM 14, 2 ms, x1.05, 512 samples).  The
    oracle's chain alone on the same bytes, quantised by the restatement and searched by NumPy at trial DM 14, gives
    S/N 32.82 from the plane at 8-bit depth and 30.48 from the 2-bit codes (sample 64 both)."""
    import test_gpu_chain as CH
    lp = libpb()
    data = CH._noise(0)
    best = {}
    with search.Searcher(nchan=CH.NCO, max_samples=CH.T2, boxcar_max=16, zap=search.HEIMDALL_ZAP, **CH.DMS2) as s:
        s.set_gulp(1)
        dmi = int(np.nonzero(np.asarray(s.dms) == CH.PULSE_DM)[0][0])
        for nbit in (2, 8):
            with lp.PbHandle(nbit=nbit, rfi_mode=1, rows_per_seg=CH.R2, max_seg=CH.S2, inject_frb=True, keep_ave=nbit == 2) as h:
                h.set_frb_params(dm=CH.PULSE_DM, width_rows=-1, amp=CH.PULSE_AMP)
                CH._process(h, data, CH.S2, inject_now=1)
                codes, ave = h.output_dev(0, 1)
                feeds = [("codes%d" % nbit, lambda: s.push(nbit=nbit, device_ptr=codes, nsamp=CH.T2))]
                if nbit == 2:
                    feeds.append(("plane", lambda: s.push_plane(device_ptr=ave, nsamp=CH.T2)))
                for name, feed in feeds:
                    assert feed() == CH.T2
                    best[name] = s.gulp_run()["snr"][dmi].max()
                    s.gulp_advance(0)
    with capsys.disabled():
        print("\npulse at trial DM %g: S/N %.4f from the fp32 plane of a 2-bit handle, %.4f from an 8-bit handle's codes, "
              "%.4f from the 2-bit codes" % (CH.PULSE_DM, best["plane"], best["codes8"], best["codes2"]))
    assert np.float32(best["plane"]).view(np.uint32) == np.float32(best["codes8"]).view(np.uint32)
    assert best["plane"] > best["codes2"]


# ---------------------------------------------------------------------------------------------------------------------
# (g) the host

RG, SEG = 64, 10
SEARCH_FLAGS = "-dm 0 6 -dm_step 2 -boxcar_max 4 -nsamps_gulp 128 -detect_thresh 1 -zap_chans 0 190 -zap_chans 3900 4096"
EXTRA = "-giants -cutouts -refine"


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """one observation of 5 shortened seconds (80 samples each; the last is dropped), about 80 MB.  (Seed 32: the first
    gulp's strongest cluster peaks where the 256-sample block leaves the refinement its window, so the run with -refine
    writes a .refined file; seeds 31 and 33 .. 36 give none.)"""
    from test_gpu_pipeline import _dump
    path = str(tmp_path_factory.mktemp("plane_dump") / "obs.uw")
    _dump(path, make_input(32, RG, 5 * SEG))
    return path


def host_run(dump, datadir, nbit, *more):
    pbmod = importlib.import_module("vlite-fast_amd.process_baseband")
    os.makedirs(str(datadir), exist_ok=True)
    argv = ["-w", "2", "-r", "2", "-b", str(nbit), "--no-control", "--replay", dump, "--datadir", str(datadir), "--logdir",
            str(datadir / "logs"), "--rows-per-seg", str(RG)] + list(more)
    assert pbmod.run(pbmod.build_parser().parse_args(argv)) == 0
    fils = sorted(p for p in os.listdir(str(datadir)) if p.endswith(".fil"))
    assert len(fils) == 2 and fils[1].endswith("_kur.fil")
    return [str(datadir / f) for f in fils]


def search_file(fil, out, flags):
    import shlex
    search.main(["-f", fil, "-stream_chunk", "80"] + shlex.split(flags) + ["-output_dir", str(out)])


def files(d):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in sorted(os.listdir(str(d)))}


@pytest.fixture(scope="module")
def plain(dump, tmp_path_factory):
    """the .fil files of -b 2 and -b 8 runs without --search"""
    root = tmp_path_factory.mktemp("plane_plain")
    return {nbit: host_run(dump, root / ("b%d" % nbit), nbit) for nbit in (2, 8)}


def test_host_search_of_the_plane_equals_b8_then_search_f(dump, plain, tmp_path, capsys):
    A, B = tmp_path / "A", tmp_path / "B"
    fils = host_run(dump, tmp_path / "run1", 2, "--search", "%s -output_dir %s" % (SEARCH_FLAGS, A))
    search_file(plain[8][1], B, SEARCH_FLAGS)
    capsys.readouterr()
    a, b = files(A), files(B)
    assert len(a) > 0 and all(f.endswith(".cand") for f in a)
    assert list(a) == list(b) and a == b
    # and what is written is what a run without --search writes
    for mine, theirs in zip(fils, plain[2]):
        assert os.path.basename(mine) == os.path.basename(theirs)
        assert open(mine, "rb").read() == open(theirs, "rb").read()
    hdr = importlib.import_module("vlite-fast_amd.sigproc").read_header(open(fils[1], "rb").read(4096))[0]
    assert hdr["nbits"] == 2


def test_host_search_of_the_codes_equals_search_f_on_its_own_file(dump, plain, tmp_path, capsys):
    Cd, D = tmp_path / "C", tmp_path / "D"
    host_run(dump, tmp_path / "run3", 2, "--search", "%s -output_dir %s" % (SEARCH_FLAGS, Cd), "--search-input", "codes")
    search_file(plain[2][1], D, SEARCH_FLAGS)
    capsys.readouterr()
    c, d = files(Cd), files(D)
    assert len(c) > 0 and list(c) == list(d) and c == d


def test_host_search_with_giants_cutouts_and_refinement(dump, plain, tmp_path, capsys):
    A, B = tmp_path / "A", tmp_path / "B"
    flags = SEARCH_FLAGS + " " + EXTRA
    host_run(dump, tmp_path / "run5", 2, "--search", "%s -output_dir %s" % (flags, A))
    search_file(plain[8][1], B, flags)
    capsys.readouterr()
    a, b = files(A), files(B)
    assert list(a) == list(b)
    kinds = set(f.rsplit(".", 1)[1] for f in a)
    assert {"cand", "npz", "refined"} <= kinds, kinds
    for f in a:
        if f.endswith(".npz"):
            za, zb = np.load(os.path.join(str(A), f)), np.load(os.path.join(str(B), f))
            assert sorted(za.files) == sorted(zb.files)
            for k in za.files:
                assert za[k].dtype == zb[k].dtype and np.array_equal(za[k], zb[k], equal_nan=za[k].dtype.kind == "f"), (f, k)
        else:
            assert a[f] == b[f], f
