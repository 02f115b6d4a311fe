"""The beamformer's definition on the CPU (tests/beam_ref.py; no GPU): the sign of the delays -- passing the true delays
of correlate_ref.delayed_antennas lines the antennas up, the negated ones do not --, the weight of an undelayed antenna,
and the bookkeeping of windows and rows_used."""
import numpy as np
import pytest

import beam_ref as BR
import correlate_ref as XR

NFFT, CHANMIN, NCO = 12500, 2155, 4096
DELAYS = (0, 58, 131)


@pytest.fixture(scope="module")
def spectra():
    """delayed_antennas through numpy.fft.rfft rows, as image_ref.delayed_gate: complex64 [3][2][8][4096]"""
    nrows = 8
    v = XR.delayed_antennas(5, nrows * NFFT, DELAYS).astype(np.float64) - 128.0
    X = np.fft.rfft(v.reshape(len(DELAYS), 2, nrows, NFFT), axis=-1)[..., CHANMIN:CHANMIN + NCO]
    return X.astype(np.complex64)


def _aa(X, delay, gain=None):
    """band- and row-summed AA per beam, in double"""
    beams, _ = BR.beamform(X, None, delay, gain=gain, tscr=X.shape[2])
    assert beams.shape == (np.atleast_2d(delay).shape[0], 1, 4, NCO)
    return beams[:, 0, 0].astype(np.float64).sum(axis=-1)


def test_true_delays_add_coherently_and_negated_ones_do_not(spectra):
    d = np.array(DELAYS, np.float64)
    incoherent = _aa(spectra, np.zeros((3, 3)), gain=np.eye(3, dtype=np.float32)).sum()
    ratios = _aa(spectra, np.stack([d, -d, d + np.array([0, 0.5, 0]), d + np.array([0, 0.37, -0.41])])) / incoherent
    print("coherent / incoherent AA: true %.4f  negated %.4f  antenna 1 off by 0.5 %.4f  wrong fractions %.4f" % tuple(ratios))
    # A s + (1 - s) = 2.0 for three antennas that share half of their variance
    assert ratios[0] >= 1.9
    assert ratios[1] <= 1.1
    assert ratios[1] < ratios[2] < ratios[0]


def test_weight_of_an_undelayed_antenna_is_one():
    wr, wi = BR.weights(np.zeros((1, 1)))
    assert wr.dtype == np.float32 and wr.shape == (1, 1, NCO)
    assert np.array_equal(wr.view(np.uint32), np.ones((1, 1, NCO), np.float32).view(np.uint32))
    assert np.array_equal(wi.view(np.uint32), np.zeros((1, 1, NCO), np.float32).view(np.uint32))
    # and a gain scales it, a gain of 0 leaves +-0
    wr, wi = BR.weights(np.array([[0.0, 17.25]]), gain=np.array([[0.5, 0.0]], np.float32))
    assert np.all(wr[0, 0] == 0.5) and np.all(wi[0, 0] == 0) and np.all(wr[0, 1] == 0) and np.all(wi[0, 1] == 0)


def test_one_hot_beam_is_the_antennas_own_power(spectra):
    beams, used = BR.beamform(spectra, None, np.zeros((1, 3)), gain=np.array([[0, 1, 0]], np.float32), tscr=1)
    x = spectra[1]
    aa = x[0].real * x[0].real + x[0].imag * x[0].imag
    assert beams.shape == (1, 8, 4, NCO) and np.array_equal(beams[0, :, 0], aa) and np.all(used == 1)


def test_windows_and_rows_used(spectra):
    T = spectra.shape[2]
    P = BR.detect(spectra, np.array(DELAYS, np.float64))
    shift = (np.arange(NCO) % 3).astype(np.int32)
    out = BR.integrate(P, shift, 3, 2)
    for c in (0, 1, 2, 4095):
        for s in range(2):
            acc = np.zeros(4, np.float32)
            for k in range(3):
                acc = acc + P[0, shift[c] + 3 * s + k, :, c]
            assert np.array_equal(out[0, s, :, c].view(np.uint32), acc.view(np.uint32))
    w = np.ones((3, T), np.float32)
    w[0, 4] = 0
    w[2, 1] = 0
    gain = np.array([[1, 1, 1], [0, 1, 1], [0, 1, 0], [0, 0, 0]], np.float32)
    used = BR.rows_used(w, T, gain, shift, 3, 2)
    assert used.shape == (4, 2, NCO) and used.dtype == np.int32
    assert used[:, :, 0].tolist() == [[2, 2], [2, 3], [3, 3], [3, 3]]          # channel 0: rows 0..2 and 3..5
    assert used[:, :, 2].tolist() == [[2, 3], [3, 3], [3, 3], [3, 3]]          # channel 2: rows 2..4 and 5..7
    assert np.all(BR.rows_used(None, T, gain, shift, 3, 2) == 3)
    with pytest.raises(AssertionError):
        BR.integrate(P, shift, 3, 3)                                             # 2 + 9 > 8: the window leaves the batch
