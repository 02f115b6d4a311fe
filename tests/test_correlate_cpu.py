"""The correlator's definition and its host-side numpy, without a GPU: the float32 restatement (correlate_ref.py)
against a double sum and against the properties the definition promises, delay recovery on seeded voltages, the golden
outputs of the reference's correlate / get_delays / fit_delays, and dm_row0."""
import importlib
import os

import numpy as np
import pytest

import correlate_ref as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NFFT, NCO = 12500, 4096


def corr():
    return importlib.import_module("vlite-fast_amd.correlate")


@pytest.fixture(scope="module")
def noise_spectra(oracle):
    """three antennas, two 16-row segments, raw stream: X [3][2][32][4096]"""
    from helpers import make_input
    R, nseg = 16, 2
    data = np.stack([make_input(60 + a, R, nseg, rfi=False, dropped=False) for a in range(3)])
    return XR.batch_spectra(oracle, data, R, 0)[0][0]


def test_restatement_against_a_double_sum(noise_spectra):
    """every value within the rounding of its binary32 operations: two products and one sum per term (3 roundings of
    at most |ax bx| + |ay by| each) and nrows additions of partial sums that the same total bounds"""
    X = noise_spectra
    nrows = 16
    row0 = XR.uniform_row0(32, nrows)
    vis, used = XR.correlate(X, None, row0, nrows)
    assert np.all(used == nrows)
    Xd = X.astype(np.complex128)
    for g in range(2):
        rows = slice(g * nrows, (g + 1) * nrows)
        for b, (i, j) in enumerate(XR.baselines(3)):
            for p in range(2):
                for q in range(2):
                    a, c = Xd[i, p, rows], Xd[j, q, rows]
                    exact = (a * np.conj(c)).sum(axis=0)
                    mag_re = (np.abs(a.real * c.real) + np.abs(a.imag * c.imag)).sum(axis=0)
                    mag_im = (np.abs(a.imag * c.real) + np.abs(a.real * c.imag)).sum(axis=0)
                    got = vis[g, b, 2 * p + q].astype(np.complex128)
                    assert np.all(np.abs(got.real - exact.real) <= (nrows + 3) * 2.0 ** -24 * mag_re)
                    assert np.all(np.abs(got.imag - exact.imag) <= (nrows + 3) * 2.0 ** -24 * mag_im)


def test_autos_are_hermitian_exactly(noise_spectra):
    vis, _ = XR.correlate(noise_spectra, None, XR.uniform_row0(32, 32), 32)
    for b, (i, j) in enumerate(XR.baselines(3)):
        if i != j:
            continue
        for pr in (0, 3):
            assert np.array_equal(vis[0, b, pr].imag.view(np.uint32), np.zeros(NCO, np.uint32))     # +0, not -0
            assert np.all(vis[0, b, pr].real > 0)
        assert np.array_equal(vis[0, b, 2], np.conj(vis[0, b, 1]))


def test_swapping_two_antennas_conjugates_their_baseline(noise_spectra):
    X = noise_spectra[:2]
    row0 = XR.uniform_row0(32, 8)
    a, _ = XR.correlate(X, None, row0, 8)
    b, _ = XR.correlate(np.ascontiguousarray(X[::-1]), None, row0, 8)
    for p in range(2):
        for q in range(2):
            assert np.array_equal(b[:, 1, 2 * p + q], np.conj(a[:, 1, 2 * q + p]))
    assert np.array_equal(b[:, 0], a[:, 2]) and np.array_equal(b[:, 2], a[:, 0])


def _lag_case(oracle, delays, shared):
    R = 8
    u8 = XR.delayed_antennas(5, R * NFFT, delays, shared)
    X = XR.batch_spectra(oracle, u8[:, None], R, 0)[0][0]
    vis, used = XR.correlate(X, None, XR.uniform_row0(R, R), R)
    return corr().lag_delays(vis[0], used[0])


@pytest.mark.parametrize("delay,shared,lagbin", [(58, 0.5, 19), (-119, 0.25, 4057)])
def test_two_antenna_delay_is_recovered(oracle, delay, shared, lagbin):
    """58 samples are 58 * 4096 / 12500 = 19.005 lag bins; -119 samples -38.99, i.e. bin 4096 - 39"""
    lag = _lag_case(oracle, (0, delay), shared)
    want = np.fft.fftfreq(NCO)[lagbin]
    for k in range(2):
        assert lag.cycles[k, 0, 1] == want and lag.cycles[k, 1, 0] == -want
        assert abs(lag.samples[k, 0, 1] - delay) < 0.5 * NFFT / NCO
        print("pol product %d: peak %.1f, third-largest %.1f" % (3 * k, lag.peak[k, 0, 1], lag.third[k, 0, 1]))
        assert lag.peak[k, 0, 1] >= 10 * lag.third[k, 0, 1]
    if delay == 58:
        assert abs(lag.samples[0, 0, 1] - 57.98) < 0.005


def test_three_antennas_through_fit_delays(oracle):
    delays = (0, 58, -61)
    lag = _lag_case(oracle, delays, 0.5)
    for k in range(2):
        m, model = corr().fit_delays(lag.samples[k])
        assert m[0] == 0
        # delays[i][j] = m_i - m_j is positive when antenna j is the later one: m_k = -(lateness of antenna k)
        assert np.all(np.abs(-m - np.array(delays)) < 0.5 * NFFT / NCO + 1e-9), m
        assert np.all(np.abs(model - lag.samples[k]) < NFFT / NCO)


def test_fit_delays_is_exact_on_consistent_delays():
    m0 = np.array([0.0, 3.5, -7.25, 11.0])
    m, model = corr().fit_delays(m0[:, None] - m0[None, :])
    assert np.allclose(m, m0, rtol=0, atol=1e-12) and np.allclose(model, m0[:, None] - m0[None, :], atol=1e-12)


# ---- the golden: what the reference's own functions return (tests/golden/make_correlate_golden.py)

# The restatement runs on the oracle's fixed-order binary32 FFT, the golden on numpy's double FFT rounded to complex64 and
# added in complex64.  Largest deviation measured, relative to the largest in-band |cmatrix|: 2.345e-07 (two beams) and
# 3.220e-07 (three); the bound is four times the larger one.
GOLDEN_TOL = 4 * 3.22e-7


@pytest.fixture(scope="module")
def corr_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_correlate.npz"))


def _golden_vis(oracle, G, name):
    delays = [int(d) for d in G[name + "_delays"]]
    nchunk = int(G["nchunk"])
    u8 = XR.delayed_antennas(int(G[name + "_seed"]), nchunk * NFFT, delays)
    X = XR.batch_spectra(oracle, u8[:, None], nchunk, 0)[0][0]
    vis, _ = XR.correlate(X, None, XR.uniform_row0(nchunk, nchunk), nchunk)
    return vis[0], nchunk


@pytest.mark.parametrize("name", ["b2", "b3"])
def test_golden_cmatrix(oracle, corr_golden, name):
    """The restatement over 8 rows, scaled by 1 / (12500 * nchunk), against the reference's cmatrix in band.  Measured:
    2.345e-07 (b2) and 3.220e-07 (b3) of the largest |cmatrix|; asserted: 4 * 3.22e-7 = 1.288e-6."""
    vis, nchunk = _golden_vis(oracle, corr_golden, name)
    got = vis[:, 0].astype(np.complex128) / (NFFT * nchunk)
    ref = corr_golden[name + "_cmatrix"].astype(np.complex128)
    dev = np.abs(got - ref).max() / float(corr_golden[name + "_cmax"])
    print("%s: largest deviation / largest |cmatrix| = %.3e" % (name, dev))
    assert dev <= GOLDEN_TOL


@pytest.mark.parametrize("name", ["b2", "b3"])
def test_golden_delays(oracle, corr_golden, name):
    vis, _ = _golden_vis(oracle, corr_golden, name)
    lag = corr().lag_delays(vis)
    assert np.array_equal(lag.cycles[0], corr_golden[name + "_get_delays"])
    m, model = corr().fit_delays(lag.cycles[0])
    assert np.allclose(m, corr_golden[name + "_fit"], rtol=1e-6, atol=0)
    assert np.allclose(model, corr_golden[name + "_fit_model"], rtol=1e-6, atol=0)


def test_golden_lag_delays_on_the_reference_matrix(corr_golden):
    """lag_delays on the reference's own matrix (autos and crosses as stored) gives the reference's delays"""
    for name, nant in (("b2", 2), ("b3", 3)):
        cm = corr_golden[name + "_cmatrix"]
        vis = np.repeat(cm[:, None, :], 4, axis=1)
        assert np.array_equal(corr().lag_delays(vis).cycles[0], corr_golden[name + "_get_delays"])


# ---- dm_row0

@pytest.mark.parametrize("dm", [0.0, 56.7, 500.0])
def test_dm_row0(dm):
    total = 1 << 20
    r = corr().dm_row0(dm, 7, total)
    assert r.dtype == np.int32 and r.shape == (NCO,) and r[0] == 7
    assert np.all(np.diff(r) >= 0)
    for c in (0, 1, 1000, 4095):
        f = (384.0 - (2155 + c) * 64.0 / 6251) * 1e-3
        f0 = (384.0 - 2155 * 64.0 / 6251) * 1e-3
        d = dm * 4.15e-3 * (f ** -2 - f0 ** -2)
        assert r[c] == 7 + int(np.floor(d / (12500 / 128e6) + 0.5)), c
    if dm == 0:
        assert np.all(r == 7)
    with pytest.raises(ValueError):
        corr().dm_row0(dm, -1, total)
    with pytest.raises(ValueError):
        corr().dm_row0(dm, total, total)
