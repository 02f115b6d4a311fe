"""The imager on the GPU (pb_imager_*, libpb.PbImager) against the CPU restatement of its definition
(tests/image_ref.py): image and per-baseline sums bit for bit in both modes, with and without phases, over pixel counts
around the kernel's pixel tile and baseline counts 1 .. 153; reuse of one imager; refusals; timers; and the chain from
voltages through the handle and the correlator to fine delays."""
import ctypes as C
import importlib

import numpy as np
import pytest

import correlate_ref as XR
import image_ref as IR
from helpers import libpb

pytestmark = pytest.mark.gpu

NFFT, NCO = 12500, 4096
PX = libpb().IMAGE_PX
CASES = [(1, 1), (2, 3), (PX - 1, 3), (PX, 3), (PX + 1, 28), (67, 28), (257, 3), (5, 153)]


def _inputs(seed, npix, nbl):
    """visibilities with zero channels and a zero baseline slot; delays that are whole samples, half samples (the ties of
    rint), negative, and fractional; phases of several turns"""
    rng = np.random.default_rng(seed)
    u = (rng.standard_normal((nbl, 2, NCO)) + 1j * rng.standard_normal((nbl, 2, NCO))).astype(np.complex64)
    u[:, :, 700:900] = 0
    u[rng.integers(nbl), 1] = 0
    u[:, 0, ::97] = 0
    dd = rng.uniform(-20000, 20000, (npix, nbl))
    kind = rng.integers(0, 4, (npix, nbl))
    dd = np.where(kind == 0, np.rint(dd), np.where(kind == 1, np.rint(dd) + 0.5, dd))
    dd.flat[0] = -6250.0                               # k / 2 turns: every odd bin a tie
    dd.flat[-1] = 0.0
    dpsi = rng.uniform(-4, 4, (npix, nbl))
    dpsi.flat[0] = 0.5
    return u, dd, dpsi


def _same(got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), int((got.view(np.uint32) != ref.view(np.uint32)).sum())


@pytest.mark.parametrize("npix,nbl", CASES)
def test_image_and_per_baseline_sums_equal_the_restatement(npix, nbl):
    lp = libpb()
    u, dd, dpsi = _inputs(1000 * npix + nbl, npix, nbl)
    with lp.PbImager(nbl, npix) as im:
        im.set_vis(u)
        for psi in (None, dpsi):
            _, ref_z = IR.image(u, dd, psi)
            for mode, m in (("delay", IR.DELAY), ("phase", IR.PHASE)):
                img, z = im.run(dd, psi, mode=mode, per_baseline=True)
                _same(z.view(np.float32), ref_z.view(np.float32))
                _same(img, IR.combine(ref_z, m))
                _same(im.run(dd, psi, mode=mode), img)             # the image alone, without the per-baseline copy


def test_an_imager_is_reused_across_grids_and_visibilities():
    lp = libpb()
    u, dd, dpsi = _inputs(77, 40, 6)
    u2 = _inputs(78, 1, 6)[0]
    with lp.PbImager(6, 64) as im:
        im.set_vis(u)
        for n in (40, PX + 3, 1, 33):
            img, z = im.run(dd[:n], dpsi[:n], per_baseline=True)
            ref_img, ref_z = IR.image(u, dd[:n], dpsi[:n])
            _same(z.view(np.float32), ref_z.view(np.float32))
            _same(img, ref_img)
        im.set_vis(u2)
        img, z = im.run(dd[:19], per_baseline=True)
        ref_img, ref_z = IR.image(u2, dd[:19])
        _same(z.view(np.float32), ref_z.view(np.float32))
        _same(img, ref_img)


def test_refusals_and_their_messages():
    lp = libpb()
    L = lp.load()
    for kw, msg in ((dict(nbl=0, max_pix=4), "nbl must be 1..256"), (dict(nbl=257, max_pix=4), "nbl must be 1..256"),
                    (dict(nbl=3, max_pix=0), "max_pix must be positive")):
        with pytest.raises(ValueError, match=msg):
            lp.PbImager(**kw)
    u, dd, dpsi = _inputs(5, 4, 3)
    with lp.PbImager(3, 4) as im:
        with pytest.raises(lp.PbError, match="no pb_imager_set_vis yet"):
            im.run(dd)
        im.set_vis(u)
        ref = im.run(dd, dpsi)
        with pytest.raises(ValueError, match="npix must be 1..max_pix"):
            im.run(np.concatenate([dd, dd]))
        with pytest.raises(ValueError, match="npix must be 1..max_pix"):
            im.run(dd[:0])
        for bad in (np.nan, np.inf, -np.inf, 2.0 ** 24 + 2, -2.0 ** 24 - 2):
            d = dd.copy()
            d[3, 2] = bad
            with pytest.raises(ValueError, match="a dd is not finite or beyond 2\\^24 samples"):
                im.run(d)
        d = dd.copy()
        d[0, 0] = 2.0 ** 24                                # the largest delay is accepted
        im.run(d)
        for bad in (np.nan, np.inf):
            p = dpsi.copy()
            p[1, 1] = bad
            with pytest.raises(ValueError, match="a dpsi is not finite"):
                im.run(dd, p)
        f64p, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        img = np.zeros(4, np.float32)
        for mode in (-1, 2):
            assert L.pb_imager_run(im._m, mode, 4, dd.ctypes.data_as(f64p), None, img.ctypes.data_as(fp), None) == -22
            assert b"mode must be 0 (delay) or 1 (phase)" in L.pb_imager_last_error(im._m)
        assert L.pb_imager_run(im._m, 0, 4, None, None, img.ctypes.data_as(fp), None) == -22
        assert b"dd is null" in L.pb_imager_last_error(im._m)
        assert L.pb_imager_set_vis(im._m, None) == -22
        with pytest.raises(ValueError):
            im.set_vis(u[:2])
        with pytest.raises(ValueError):
            im.run(dd[:, :2])
        with pytest.raises(ValueError):
            im.run(dd, mode="both")
        _same(im.run(dd, dpsi), ref)                       # a refused call leaves the imager as it was


def test_timers_are_positive():
    lp = libpb()
    u, dd, dpsi = _inputs(6, 64, 3)
    with lp.PbImager(3, 64) as im:
        assert im.timers() == (0.0, 0.0, 0.0)
        im.set_vis(u)
        im.run(dd, dpsi, per_baseline=True)
        t = im.timers()
        print("upload %.4f ms, kernels %.4f ms, copy back %.4f ms" % t)
        assert len(t) == 3 and all(v > 0 for v in t)


def test_fine_delays_through_the_handle_and_the_correlator():
    """voltages -> coherence handle -> pb_correlate -> weighted_vis (one gate, no off-gate) -> the scan on the GPU:
    the three delays within 0.1 sample (5 sigma of the expected 0.019), and the scan itself equal to the restatement"""
    lp = libpb()
    loc = importlib.import_module("vlite-fast_amd.localise")
    R = 8
    u8 = XR.delayed_antennas(5, R * NFFT, (0, 58, 131))
    with lp.PbHandle(nant=3, nbit=8, npol=2, rfi_mode=0, rows_per_seg=R, max_seg=1, coherence=True) as h:
        for a in range(3):
            h.submit_planar(a, 0, u8[a, 0], u8[a, 1])
        h.process(1)
        vis, used = h.correlate(0, 1, R)
    assert vis.shape == (1, 6, 4, NCO)
    u, bls = loc.weighted_vis(vis, 0, used)
    assert bls == [(0, 1), (0, 2), (1, 2)]
    coarse = loc.coarse_delays(u)
    with lp.PbImager(3, 101) as im:
        im.set_vis(u)
        fd = loc.fine_delays(im, coarse)
    ref = IR.RefImager(3)
    ref.set_vis(u)
    _, ref_scan = ref.run(fd["dd"], per_baseline=True)
    _same(fd["scan"].view(np.float32), ref_scan.view(np.float32))
    dev = fd["samples"] - np.array([58, 131, 73])
    print("deviations of the baselines' delays (samples), per pol:", np.round(dev, 4).tolist())
    print("fitted antenna delays:", np.round(fd["fit_samples"], 4).tolist())
    assert np.abs(dev).max() <= 0.1
    assert np.abs(fd["fit_samples"] - [0, 58, 131]).max() <= 0.1
