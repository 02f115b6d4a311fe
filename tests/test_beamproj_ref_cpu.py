"""The projecting beamformer's definition and the host side of the spatial nulls, without a GPU: the restatement
(tests/beamproj_ref.py) against beam_ref with the unit matrix, against binary64 and against the quadratic form of the
correlator's restated visibilities within the derived bound; nulling.projectors' algebra; and the
physical test, an interferer of ten times the antennas' own noise taken out of a beam of four antennas
(tests/null_synth.py), per pol, which one projector for both pols cannot do."""
import importlib

import numpy as np
import pytest

import beam_ref as BR
import beamproj_ref as PR
import correlate_ref as XR
import null_synth as NS
from helpers import make_input

nulling = importlib.import_module("vlite-fast_amd.nulling")

NCO = 4096
F = np.float32
R = 8

_noise = {}


def noise_case(oracle, A):
    """A antennas of helpers.make_input (RFI bursts, a flagged row, a dropped frame), one segment of 8 rows, both
    streams"""
    if A not in _noise:
        data = np.stack([make_input(500 + 3 * a, R, 1) for a in range(A)])
        _noise[A] = XR.batch_spectra(oracle, data, R, 2)
    return _noise[A]


@pytest.mark.parametrize("A", [1, 3, 8])
def test_unit_matrix_gives_beam_refs_beams(oracle, A):
    """as numbers: only signs of zero may differ (0 - (+-0) and the like in w' = s^T I)"""
    delay, psi, gain = BR.five_beams(A, 60 + A)
    shift = (np.arange(NCO) % 3).astype(np.int32)
    for st, (X, w) in noise_case(oracle, A).items():
        ref, used = BR.beamform(X, w if st else None, delay, psi, gain, shift, 2)
        got, pused = PR.beamform_proj(X, w if st else None, delay, PR.identity(A), psi, gain, shift, 2)
        assert got.shape == ref.shape and got.dtype == ref.dtype and np.abs(ref).max() > 0
        assert np.array_equal(got, ref)
        ur, ui = PR.weights(PR.identity(A), delay, psi, gain)
        sr, si = BR.weights(delay, psi, gain)
        for p in range(2):
            assert np.array_equal(ur[:, p], sr) and np.array_equal(ui[:, p], si)
        # rows_used: every antenna counts here, beam_ref drops those of gain 0
        if st == 0:
            assert np.array_equal(pused, used)
        else:
            all_ant = BR.rows_used(w, R, np.ones((5, A), F), shift, 2, got.shape[1])
            assert np.array_equal(pused, all_ant) and np.all(pused <= used)


@pytest.mark.parametrize("A", [1, 2, 5, 8])
def test_restatement_against_binary64_and_the_visibilities(oracle, A):
    """within B_beam of beamform64, and the quadratic form w' V w'^H of the correlator's restated visibilities of the
    same gates within B_beam + B_vis of the restated beams (non-Hermitian random matrices with exact zeros)"""
    tscr = 4
    delay, psi, gain = BR.five_beams(A, 70 + A)
    proj = PR.random_proj(A, 80 + A)
    W = PR.weights64(proj, delay, psi, gain)
    for st, (X, w) in noise_case(oracle, A).items():
        beams, _ = PR.beamform_proj(X, w if st else None, delay, proj, psi, gain, None, tscr)
        exact = PR.beamform64(X, W, None, tscr)
        bound = PR.error_bound(X, proj, gain, None, tscr)
        live = bound > 0
        assert live.any() and np.all(beams[~live] == 0) and np.all(exact[~live] == 0)
        worst = (np.abs(beams - exact)[live] / bound[live]).max()
        print("A = %d stream %d: restatement against binary64, largest error / bound = %.4f" % (A, st, worst))
        assert worst <= 1.0
        vis, _ = XR.correlate(X, w if st else None, XR.uniform_row0(R, tscr), tscr)
        form = PR.from_visibilities64(vis, W)
        both = bound + PR.error_bound(X, proj, gain, None, tscr, through="vis")
        worst = (np.abs(form - beams)[live] / both[live]).max()
        print("A = %d stream %d: form of the visibilities against the beams, largest error / bound = %.4f "
              "(%.2e of the largest value)" % (A, st, worst, np.abs(form - beams).max() / np.abs(beams).max()))
        assert worst <= 1.0 and np.all(form[~live] == 0)
        # the all-zero channel of pol 0 gives AA = CR = CI = 0 there, the unit-matrix channel of pol 1 beam_ref's BB
        assert not beams[:, :, (0, 2, 3), 17].any()
        plain, _ = BR.beamform(X, w if st else None, delay, psi, gain, None, tscr)
        assert np.array_equal(beams[:, :, 1, 4000], plain[:, :, 1, 4000])


def _random_cov(A, seed, rows=12):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, NCO, A, rows)) + 1j * rng.standard_normal((2, NCO, A, rows))
    return np.einsum("pcir,pcjr->pcij", x, np.conj(x))


@pytest.mark.parametrize("A,K", [(2, 1), (4, 1), (4, 2), (8, 3)])
def test_projectors_are_idempotent_and_hermitian(A, K):
    proj, count = nulling.projectors(_random_cov(A, A + K), K)
    assert proj.shape == (2, NCO, A, A) and proj.dtype == np.complex64 and count.shape == (2, NCO)
    assert count.dtype == np.int32 and np.all(count == K)
    P = proj.astype(np.complex128)
    assert np.abs(P @ P - P).max() <= 1e-6
    assert np.abs(P - np.conj(np.swapaxes(P, 2, 3))).max() <= 1e-6
    assert np.abs(np.trace(P, axis1=2, axis2=3).real - (A - K)).max() <= 1e-5
    proj0, count0 = nulling.projectors(_random_cov(A, 1), 0)
    assert np.array_equal(proj0, PR.identity(A)) and not count0.any()
    for bad in (-1, A):
        with pytest.raises(ValueError):
            nulling.projectors(_random_cov(A, 1), bad)


def test_projectors_annihilate_a_planted_steering_vector():
    """C = r v v^H + n I exactly: P v = 0 to the eigensolver's accuracy, and P C P^H = n P"""
    A = 5
    rng = np.random.default_rng(3)
    v = rng.standard_normal((2, NCO, A)) + 1j * rng.standard_normal((2, NCO, A))
    cov = 10.0 * np.einsum("pci,pcj->pcij", v, np.conj(v)) + 0.5 * np.eye(A)
    proj, count = nulling.projectors(cov, 1)
    assert np.all(count == 1)
    left = np.einsum("pcij,pcj->pci", proj.astype(np.complex128), v)
    worst = (np.abs(left).max(axis=-1) / np.linalg.norm(v, axis=-1)).max()
    print("largest |P v| / |v| = %.2e" % worst)
    assert worst <= 1e-6                                     # complex64's rounding of P
    f = nulling.filtered_vis(cov, proj)
    assert np.abs(f - 0.5 * proj.astype(np.complex128)).max() <= 1e-5 * np.abs(cov).max()


def test_min_ratio_and_zero_channels_keep_the_identity():
    A = 4
    rng = np.random.default_rng(4)
    v = rng.standard_normal((2, NCO, A)) + 1j * rng.standard_normal((2, NCO, A))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    strength = np.where(np.arange(NCO) % 2 == 0, 20.0, 0.5)          # even channels: largest eigenvalue 21, odd 1.5
    cov = strength[None, :, None, None] * np.einsum("pci,pcj->pcij", v, np.conj(v)) + np.eye(A)
    cov[1, 100] = 0                                                  # a zapped channel
    cov[0, 101] = 0
    proj, count = nulling.projectors(cov, 1, min_ratio=5.0)
    want = np.broadcast_to((np.arange(NCO) % 2 == 0).astype(np.int32), (2, NCO)).copy()
    want[1, 100] = 0
    assert np.array_equal(count, want)
    eye = PR.identity(A)
    assert np.array_equal(proj[count == 0], eye[count == 0])
    assert np.abs(proj[count == 1] - eye[count == 1]).max() > 0.1
    # without min_ratio every channel with data is nulled, the zero ones still are not
    proj, count = nulling.projectors(cov, 1)
    assert count.sum() == 2 * NCO - 2 and count[1, 100] == 0 and count[0, 101] == 0
    assert np.array_equal(proj[1, 100], eye[0, 0]) and np.array_equal(proj[0, 101], eye[0, 0])
    with pytest.raises(ValueError):
        nulling.projectors(cov, 1, min_ratio=0.0)


def test_covariances_follow_the_baseline_order():
    A = 3
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((A, 2, 6, NCO)) + 1j * rng.standard_normal((A, 2, 6, NCO))).astype(np.complex64)
    vis, _ = XR.correlate(x, None, XR.uniform_row0(6, 3), 3)               # two gates
    cov = nulling.covariances(vis, A)
    assert cov.shape == (2, NCO, A, A) and cov.dtype == np.complex128
    x64 = x.astype(np.complex128)
    want = np.einsum("iptc,jptc->pcij", x64, np.conj(x64))
    assert np.abs(cov - want).max() <= 1e-5 * np.abs(want).max()
    assert np.array_equal(cov, np.conj(np.swapaxes(cov, 2, 3)))
    assert np.array_equal(nulling.covariances(vis.sum(axis=0), A), nulling.covariances(vis.sum(axis=0)[None], A))
    with pytest.raises(ValueError):
        nulling.covariances(vis, 4)
    assert nulling.gate_rows(0, 48, 16) == [([0, 16, 32], 16)]
    assert nulling.gate_rows(3, 40, 16) == [([3, 19], 16), ([35], 5)] and nulling.gate_rows(2, 7, 16) == [([2], 5)]
    with pytest.raises(ValueError):
        nulling.gate_rows(5, 5, 16)


def test_nulls_take_the_interferer_out_of_the_beam():
    """numpy.fft.rfft rows of null_synth's digitised voltages through the restatements"""
    X = NS.rfft_spectra(NS.case_antennas(), NS.CASE["nrows"])
    delay = np.array([NS.CASE["sky_delays"]])

    def gates(first, nrows):
        return XR.correlate(X, None, np.repeat(np.asarray(first)[:, None], NCO, axis=1), nrows)[0]

    NS.physical_checks(X.shape[0], lambda: BR.beamform(X, None, delay)[0],
                    lambda proj: PR.beamform_proj(X, None, delay, proj)[0], gates)
