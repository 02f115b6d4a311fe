"""The imager's definition on the CPU (include/pb_hip.h: pb_imager_run; tests/image_ref.py): its rotation polynomial
against binary64, its binary32 sums against a binary64 evaluation within the first-order bound of DESIGN.md section 11,
and a noiseless point source imaged on a grid."""
import numpy as np
import pytest

import image_ref as IR


def test_rotation_polynomial_is_within_2_to_minus_22():
    r = np.arange(-(1 << 19), (1 << 19) + 1) / float(1 << 20)              # every multiple of 2^-20 in [-0.5, 0.5]
    r = np.concatenate([r, np.random.default_rng(3).uniform(-0.5, 0.5, 1000000)]).astype(np.float32)
    cr, sr = IR.rotation(r)
    r64 = r.astype(np.float64)
    err = max(np.abs(cr - np.cos(2 * np.pi * r64)).max(), np.abs(sr - np.sin(2 * np.pi * r64)).max())
    print("largest rotation error: %.3f x 2^-22" % (err * 2 ** 22))
    assert err <= 2.0 ** -22
    # the quarter turns and the ties of the reduction are exact
    cr, sr = IR.rotation(np.array([0.0, 0.25, 0.5, -0.25, -0.5], np.float32))
    assert np.array_equal(cr, [1, 0, -1, 0, -1]) and np.array_equal(sr, [0, 1, 0, -1, 0])


def test_phase_reduces_in_double_with_ties_to_even():
    dd = np.array([[0.0, 12500.0, 6250.0, -6250.0, 0.5]])
    r = IR.phase(dd)
    assert not r[0, 0].any() and not r[0, 1].any()
    k = IR.BINS
    assert np.array_equal(np.abs(r[0, 2]), np.where(k % 2 == 1, 0.5, 0.0))          # k / 2 turns: ties
    assert np.array_equal(r[0, 2], np.where(k % 4 == 1, 0.5, np.where(k % 4 == 3, -0.5, 0.0)))   # rint: ties to even
    assert np.array_equal(r[0, 3], -r[0, 2])
    assert np.abs(r).max() <= 0.5


@pytest.mark.parametrize("nbl,mode", [(3, IR.DELAY), (3, IR.PHASE), (28, IR.DELAY)])
def test_float32_restatement_within_the_first_order_bound(nbl, mode):
    rng = np.random.default_rng(100 + nbl + mode)
    npix = 6
    u = (rng.standard_normal((nbl, 2, IR.NCHANOUT)) + 1j * rng.standard_normal((nbl, 2, IR.NCHANOUT))).astype(np.complex64)
    dd = rng.uniform(-20000, 20000, (npix, nbl))
    dpsi = rng.uniform(-4, 4, (npix, nbl))
    img, z = IR.image(u, dd, dpsi, mode)
    img64, z64 = IR.image64(u, dd, dpsi, mode)
    Bz = np.array([[IR.error_bound(u[b, s], 0) for s in range(2)] for b in range(nbl)])
    rz = (np.abs(z.astype(np.complex128) - z64) / Bz[None]).max()
    ri = (np.abs(img.astype(np.float64) - img64) / IR.error_bound(u, nbl)).max()
    print("nbl %d mode %d: largest error / bound: z %.4f, image %.4f" % (nbl, mode, rz, ri))
    assert rz <= 1.0 and ri <= 1.0


def test_point_source_peaks_at_its_pixel_in_both_modes():
    import importlib
    loc = importlib.import_module("vlite-fast_amd.localise")
    ps = IR.point_source()
    img, _ = IR.image64(ps["u"], ps["dd"])
    others = np.delete(img, ps["ipix"])
    print("delay mode: source %.1f, largest other %.1f" % (img[ps["ipix"]], others.max()))
    assert int(np.argmax(img)) == ps["ipix"]
    assert img[ps["ipix"]] > 0.999 * 2 * len(ps["bls"]) * IR.NCHANOUT
    assert others.max() < 0.9 * img[ps["ipix"]]
    # phase mode: the source's visibilities carry the antennas' phases, the image takes them off again
    psi = loc.baseline_phase(ps["d_ant"], ps["bls"])
    u = (ps["u"].astype(np.complex128) * np.exp(2j * np.pi * psi[ps["ipix"]])[:, None, None]).astype(np.complex64)
    img, _ = IR.image64(u, ps["dd"], psi, IR.PHASE)
    others = np.delete(img, ps["ipix"])
    print("phase mode: source %.1f, largest other %.1f" % (img[ps["ipix"]], others.max()))
    assert int(np.argmax(img)) == ps["ipix"]
    assert others.max() < 0.9 * img[ps["ipix"]]
