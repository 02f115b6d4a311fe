"""The conventions that the correlator, the imager, the beamformer and the host code between them share, without a GPU:
the sign of a delay, the side of a baseline that is conjugated, the antenna a phase belongs to.  Each kernel's own test
holds it to a restatement of its own definition; here the three restatements (correlate_ref, image_ref, beam_ref) are
held to one another and to binary64 through the oracle's spectra of a source with FRACTIONAL delays
(tests/array_synth.py), where localise.phase_turns(d) = -3 d is no whole or half turn and its sign matters."""
import importlib

import numpy as np
import pytest

import array_synth as AS
import beam_ref as BR
import correlate_ref as XR
import image_ref as IR
from helpers import make_input

loc = importlib.import_module("vlite-fast_amd.localise")
beamform = importlib.import_module("vlite-fast_amd.beamform")

NFFT, NCO = 12500, 4096
F = np.float32
R = 8
DELAYS = np.array([0.0, 58.25, 131.4])
BLS = [(0, 1), (0, 2), (1, 2)]


def table(delays, *extra):
    """the (delay, psi) that the beamform tool passes to pb_beamform for --delays d0 d1 d2 [--phase-turns]"""
    argv = ["--replay", "a", "b", "c", "--delays"] + ["%r" % float(d) for d in delays] + list(extra) + ["-o", "x"]
    return beamform.beam_table(beamform.parse_args(argv))


def ratios(form, delays=DELAYS):
    """form(delay, psi, gain) -> beams [7][1][4][4096] over all 8 rows.  The band-summed AA of the tool's beam at the
    true delays with --phase-turns, at the negated delays with --phase-turns, at the true delays without, and at the
    true delays with the sign of --phase-turns' psi flipped, each over the summed AA of the three one-hot beams"""
    d0, p0 = table(delays, "--phase-turns")
    d1, p1 = table(-delays, "--phase-turns")
    d2, p2 = table(delays)
    assert p2 is None and np.array_equal(d0, [delays]) and np.array_equal(d1, [-delays])
    d1h, g1h = beamform.one_hot(3)
    delay = np.concatenate([d0, d1, d2, d0, d1h])
    psi = np.concatenate([p0, p1, np.zeros((1, 3)), -p0, np.zeros((3, 3))])
    gain = np.concatenate([np.ones((4, 3), F), g1h])
    beams = form(delay, psi, gain)
    assert beams.shape == (7, 1, 4, NCO)
    aa = beams[:, 0, 0].astype(np.float64).sum(axis=-1)
    return aa[:4] / aa[4:].sum()


def check_ratios(r):
    """A s + (1 - s) = 2.0 for three antennas that share half their variance; the thresholds are those of
    test_beam_ref_cpu for this kind of source.  Without the phases the antennas are 3 d = 0.75 and 0.2 turns apart, with
    the phases' sign flipped twice that: the beam without --phase-turns lies strictly between the two signs."""
    print("coherent / incoherent AA: true delays with --phase-turns %.4f  negated delays %.4f  without the phases %.4f"
          "  psi of the other sign %.4f" % tuple(r))
    assert r[0] >= 1.9
    assert r[1] <= 1.1
    assert r[3] < r[2] < r[0]


def image_ratios(phase_image, delay_image, u, d=DELAYS):
    """PHASE image at baseline_phase(d) and at its negative, each over the DELAY image, all at dd = d_j - d_i"""
    dd = loc.antenna_to_baseline(d, BLS)[None]
    dpsi = loc.baseline_phase(d, BLS)[None]
    ref = float(delay_image(u, dd))
    r = float(phase_image(u, dd, dpsi)) / ref, float(phase_image(u, dd, -dpsi)) / ref
    print("PHASE image / DELAY image: baseline_phase %.5f  negated %.5f" % r)
    return r


def check_image_ratios(r):
    """these two conditions tell the signs apart; they claim no accuracy"""
    assert r[0] >= 0.99
    assert r[1] < 0.5


def check_fine_delays(fd):
    dev = np.abs(fd["samples"] - loc.antenna_to_baseline(DELAYS, BLS))
    print("largest deviation of a baseline's delay: %.4f samples; fitted antenna delays %s"
          % (dev.max(), np.round(fd["fit_samples"], 4).tolist()))
    assert dev.max() <= 0.1
    assert np.abs(fd["fit_samples"] - DELAYS).max() <= 0.1


def closure_sides(vis, beam, gain):
    """vis complex [1][6][4][4096], beam [1][4][4096] of the gains `gain` at the true delays and phases -> (u of the
    imager, complex128 [3][2][4096]: g_i g_j V_ij of products 0 and 3, unnormalised; the beam's side of the identity:
    sum over the channels of AA + BB minus the autos' share)"""
    index = dict((b, k) for k, b in enumerate(XR.baselines(3)))
    g = np.asarray(gain, np.float64)
    vis = np.asarray(vis, np.complex128)
    u = np.stack([g[i] * g[j] * vis[0, index[(i, j)]][[0, 3]] for i, j in BLS])
    autos = sum(g[i] ** 2 * vis[0, index[(i, i)]][[0, 3]].real.sum() for i in range(3))
    return u, beam[0, :2].astype(np.float64).sum() - autos


@pytest.fixture(scope="module")
def source(oracle):
    """three antennas that share half their variance at delays 0, 58.25, 131.4 samples, each carrying phase_turns of
    its delay, through the oracle's channeliser: X complex64 [3][2][8][4096]; its visibilities over the 8 rows"""
    u8 = AS.phased_antennas(5, R, DELAYS, loc.phase_turns(DELAYS))
    assert u8.shape == (3, 2, R * NFFT) and u8.dtype == np.uint8
    X = XR.batch_spectra(oracle, u8[:, None], R, 0)[0][0]
    vis, used = XR.correlate(X, None, XR.uniform_row0(R, R), R)
    return X, vis, used


def test_the_source_carries_what_it_says():
    """spectra64 of antenna a over those of antenna 0, at full sharing: exp(-2 pi i k d / 12500 + 2 pi i p)"""
    p = loc.phase_turns(DELAYS)
    X = AS.spectra64(3, 2, DELAYS, p, shared=1.0)
    assert X.shape == (3, 2, 2, NCO) and X.dtype == np.complex128
    for a in (1, 2):
        want = np.exp(2j * np.pi * (p[a] - IR.BINS * DELAYS[a] / 12500.0))
        got = X[a] / X[0]
        # the rescaling to unit variance is real and positive; channel 4095 is bin 6250, which is real and left alone
        assert np.abs(got / np.abs(got) - want)[..., :-1].max() < 1e-9
        assert np.abs(got.imag[..., -1]).max() < 1e-9 and got.real[..., -1].min() > 0
    # and the digitised rows are the voltages: mean 128.5 - 0.5 (floor), sigma 16.9
    u8 = AS.phased_antennas(3, 2, DELAYS, p)
    assert abs(u8.mean() - 128.0) < 0.1 and abs(u8.std() - 16.9) < 0.1
    assert np.array_equal(u8, AS.phased_antennas(3, 2, DELAYS, p))


def test_beam_sign_and_phase(source):
    """the beam that the tool forms for --delays 0 58.25 131.4 --phase-turns adds the common half coherently: psi must
    take the antennas' phase_turns off.  With psi = +phase_turns(delay) the phase goes on a second time: 0.665."""
    X = source[0]
    check_ratios(ratios(lambda delay, psi, gain: BR.beamform(X, None, delay, psi, gain, tscr=R)[0]))


def test_beam_sign_and_phase_in_binary64():
    """the same without the oracle and without digitising: fully shared antennas, 3.0 expected"""
    X = AS.spectra64(5, R, DELAYS, loc.phase_turns(DELAYS), shared=1.0)
    r = ratios(lambda delay, psi, gain: BR.beamform64(X, delay, psi, gain, tscr=R))
    print("fully shared, binary64: %.5f  negated delays %.5f  without the phases %.5f  psi of the other sign %.5f" % tuple(r))
    assert abs(r[0] - 3.0) < 1e-3 and r[1] <= 1.1 and r[3] < r[2] < r[0]


def test_imager_sign_and_phase(source):
    _, vis, used = source
    u, bls = loc.weighted_vis(vis, 0, used)
    assert bls == BLS
    check_image_ratios(image_ratios(lambda u, dd, dpsi: IR.image64(u, dd, dpsi, IR.PHASE)[0][0],
                                    lambda u, dd: IR.image64(u, dd, None, IR.DELAY)[0][0], u))


def test_fractional_delays_come_back(source):
    _, vis, used = source
    u, bls = loc.weighted_vis(vis, 0, used)
    coarse = loc.coarse_delays(u)
    assert np.abs(coarse - loc.antenna_to_baseline(DELAYS, BLS)).max() <= 12500 / 4096.0
    im = IR.RefImager(3)
    im.set_vis(u)
    check_fine_delays(loc.fine_delays(im, coarse))


def test_imager_and_beamformer_close(source):
    """|sum_i w_i x_i|^2 = sum_i |w_i x_i|^2 + 2 Re sum_(i<j) w_i conj(w_j) x_i conj(x_j): twice the PHASE image of
    u = g_i g_j V_ij at (dd, baseline_phase) is the beam's AA + BB at (d, -phase_turns(d)) less the autos' share.
    Both sides in binary64 on the same binary32 spectra: 1e-9 of the beam's side."""
    X, _, _ = source
    Xd = X.astype(np.complex128)
    vis = np.zeros((1, 6, 4, NCO), np.complex128)
    for b, (i, j) in enumerate(XR.baselines(3)):
        for p in range(2):
            for q in range(2):
                vis[0, b, 2 * p + q] = (Xd[i, p] * np.conj(Xd[j, q])).sum(axis=0)
    gain = np.array([1.0, 0.75, 1.5], F)
    delay, psi = table(DELAYS, "--phase-turns")
    beam = BR.beamform64(X, delay, psi, gain[None], tscr=R)[0]
    u, rhs = closure_sides(vis, beam, gain)
    lhs = 2.0 * IR.image64(u, loc.antenna_to_baseline(DELAYS, BLS)[None], loc.baseline_phase(DELAYS, BLS)[None], IR.PHASE)[0][0]
    print("2 x PHASE image %.9e  beam less autos %.9e  relative difference %.2e" % (lhs, rhs, abs(lhs - rhs) / abs(rhs)))
    assert rhs > 0 and abs(lhs - rhs) <= 1e-9 * abs(rhs)


_noise = {}


def noise_case(oracle, A):
    """A antennas of helpers.make_input (RFI bursts, a flagged row, a dropped frame), one segment of 8 rows, both
    streams"""
    if A not in _noise:
        data = np.stack([make_input(400 + 3 * a, R, 1) for a in range(A)])
        _noise[A] = XR.batch_spectra(oracle, data, R, 2)
    return _noise[A]


@pytest.mark.parametrize("A", [1, 2, 3, 4, 5, 6, 7, 8])
def test_restatements_against_binary64(oracle, A):
    """the beamformer's restatement within error_bound of beamform64, and the quadratic form of the correlator's
    restated visibilities within the two bounds added of the restated beams: conjugation side, baseline order and all
    four products in one identity"""
    tscr = 4
    delay, psi, gain = BR.five_beams(A, 50 + A)
    shift = (np.arange(NCO) % 3).astype(np.int32)
    for st, (X, w) in noise_case(oracle, A).items():
        # a shifted window of the beam alone, then the gates that the correlator shares
        for sh, nout in ((shift, 1), (None, R // tscr)):
            beams, _ = BR.beamform(X, w if st else None, delay, psi, gain, sh, tscr, nout)
            exact = BR.beamform64(X, delay, psi, gain, sh, tscr, nout)
            bound = BR.error_bound(X, gain, sh, tscr, nout)
            live = bound > 0
            assert live.any() and np.all(beams[~live] == 0) and np.all(exact[~live] == 0)
            worst = (np.abs(beams - exact)[live] / bound[live]).max()
            print("A = %d stream %d: restatement against binary64, largest error / bound = %.4f" % (A, st, worst))
            assert worst <= 1.0
        vis, _ = XR.correlate(X, w if st else None, XR.uniform_row0(R, tscr), tscr)
        form = BR.from_visibilities64(vis, delay, psi, gain)
        both = bound + BR.error_bound(X, gain, None, tscr, through="vis")
        worst = (np.abs(form - beams)[live] / both[live]).max()
        rel = np.abs(form - beams).max() / np.abs(beams).max()
        print("A = %d stream %d: form of the visibilities against the beams, largest error / bound = %.4f "
              "(%.2e of the largest value)" % (A, st, worst, rel))
        assert worst <= 1.0 and np.all(form[~live] == 0)
