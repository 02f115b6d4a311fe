"""The fringe-stopping correlator's definition on the CPU (include/pb_hip.h: pb_correlate_tracked; no GPU): its binary32
restatement against a binary64 evaluation, its sign convention and its effect on a source whose delay and phase drift,
its identity with the imager, and the geometry that makes its model."""
import importlib

import numpy as np
import pytest

import correlate_ref as XR
import correlate_track_ref as TR
import fringe_synth as FS
import image_ref as IR

BLS = XR.baselines(3)
ROW0 = XR.uniform_row0(FS.ROWS, FS.ROWS)
FULL = FS.model_of(FS.D0, FS.D1, FS.P0, FS.P1)
STATIC = FULL * np.array([1.0, 0.0, 1.0, 0.0])


@pytest.fixture(scope="module")
def spectra():
    """numpy.fft.rfft spectra of the digitised drifting source, complex128 [3][2][24][4096]"""
    return FS.spectra_of_codes(FS.drifting_antennas(FS.SEED, FS.ROWS, FS.D0, FS.D1, FS.P0, FS.P1, FS.SHARED), FS.ROWS)


def test_synth_without_drift_is_array_synth():
    import array_synth
    assert np.array_equal(FS.voltages(3, 2, (0, 5.5), (0, 0), (0.1, 0.2), (0, 0)), array_synth.voltages(3, 2, (0, 5.5), (0.1, 0.2)))


def test_restatement_against_binary64(spectra):
    """the binary32 restatement against the binary64 evaluation of the same sums on the same complex64 spectra: the
    largest deviation relative to the largest modulus, measured 2.02e-7 (one 24-row gate; the rotation's 2^-22 and 24
    binary32 additions), held to four times that as DESIGN.md section 10 holds its reference pin"""
    X = spectra.astype(np.complex64)
    v32, used = TR.correlate_tracked(X, None, ROW0, FS.ROWS, FULL)
    v64 = TR.correlate64(X, ROW0, FS.ROWS, FULL)
    dev = np.abs(v32 - v64).max() / np.abs(v64).max()
    print("restatement against binary64: %.3g of the largest modulus" % dev)
    assert dev <= 4 * 2.02e-7
    assert np.all(used == FS.ROWS)


def test_convention_and_effect(spectra):
    """|sum_c V(c)| / sum_c sqrt(auto_i auto_j), pol 0 x pol 0, one 24-row gate, in binary64.  Measured: 0.507, 0.503,
    0.505 (baselines 0-1, 0-2, 1-2) with the full model; 0.094, 0.068, 0.055 with its rates set to zero; 0.503, 0.504,
    0.501 for a source that does not drift under its static model.  The two conditions tell tracking from not tracking
    and the signs apart; they claim no accuracy."""
    tracked = FS.band_coherence(TR.correlate64(spectra, ROW0, FS.ROWS, FULL)[0], BLS)
    untracked = FS.band_coherence(TR.correlate64(spectra, ROW0, FS.ROWS, STATIC)[0], BLS)
    print("tracked", tracked, "static model", untracked)
    for b in ((0, 1), (0, 2), (1, 2)):
        assert tracked[b] >= 0.45, (b, tracked[b])
        assert untracked[b] <= 0.2, (b, untracked[b])
    # a wrong sign of either pair of columns does not stop the fringes
    for flip in (np.array([-1.0, -1.0, 1.0, 1.0]), np.array([1.0, 1.0, -1.0, -1.0])):
        wrong = FS.band_coherence(TR.correlate64(spectra, ROW0, FS.ROWS, FULL * flip)[0], BLS)
        assert max(wrong.values()) <= 0.2, wrong


def test_identity_with_the_imager(spectra):
    """with rates 0, in binary64: sum_c V'_ij(c) is the imager's z at dd = d_j - d_i, dpsi = psi_j - psi_i"""
    cross = [(i, j) for i, j in BLS if i != j]
    plain = TR.correlate64(spectra, ROW0, FS.ROWS)[0]
    tracked = TR.correlate64(spectra, ROW0, FS.ROWS, STATIC)[0]
    u = np.stack([plain[BLS.index(b)][[0, 3]] for b in cross])                 # [3][2][4096]
    dd = np.array([[STATIC[j, 0] - STATIC[i, 0] for i, j in cross]])
    dpsi = np.array([[STATIC[j, 2] - STATIC[i, 2] for i, j in cross]])
    _, z = IR.image64(u, dd, dpsi, IR.PHASE)
    for k, b in enumerate(cross):
        for s, prod in enumerate((0, 3)):
            got = tracked[BLS.index(b), prod].sum()
            assert abs(got - z[0, k, s]) <= 1e-9 * np.abs(u[k, s]).sum(), (b, prod)


def _source_vector_near(loc, ra, dec, unix, dt):
    """localise.source_vector at unix + dt with the sidereal angle taken as gmst_rad(unix) plus its rate times dt -- the
    formula of gmst_rad is linear in time, so this is the same angle without the rounding of its Julian date, which in
    binary64 resolves 40 us: 2 10^-5 of the two seconds a central difference spans"""
    g = loc.gmst_rad(unix) + 24.06570982441908 / 86400.0 * (np.pi / 12.0) * dt
    T = (float(unix + dt) / 86400.0 + 2440587.5 - 2451545.0) / 36525.0
    v = np.array([np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)])
    return v @ (loc._r3(g) @ loc.precession_matrix(T)).T


@pytest.mark.parametrize("dec_deg", [-30.0, 22.0, 70.0])
def test_delay_rates_against_the_central_difference(dec_deg):
    """antenna_delay_rates against (antenna_delays(source_vector(unix + 1)) - antenna_delays(source_vector(unix - 1))) / 2,
    8 antennas of 10 km extent: the difference's truncation is Omega^2 (1 s)^2 / 6 = 9 10^-10 relative; held to 10^-7.
    The difference's source vectors take their sidereal angle from the epoch's (see _source_vector_near; with
    localise.source_vector itself the two sides agree to 5.5 10^-6, the Julian date's rounding), and are
    localise.source_vector's at the epoch.  The rate carries the precession's term (unix given): the sidereal term alone
    is 0.7, 1.0, 1.6 10^-7 off at these declinations, which is the precession's 50" a year over the Earth's turn."""
    loc = importlib.import_module("vlite-fast_amd.localise")
    rng = np.random.default_rng(3)
    xyz = np.array([-1601185.4, -5041977.5, 3554875.9]) + rng.uniform(-5e3, 5e3, (8, 3))
    unix, ra, dec = 1700000000.0, np.radians(83.6), np.radians(dec_deg)
    s = loc.source_vector(ra, dec, unix)
    assert np.array_equal(_source_vector_near(loc, ra, dec, unix, 0.0), s)
    diff = (loc.antenna_delays(xyz, _source_vector_near(loc, ra, dec, unix, 1.0))
            - loc.antenna_delays(xyz, _source_vector_near(loc, ra, dec, unix, -1.0))) / 2      # samples per second
    rate = loc.antenna_delay_rates(xyz, s, unix) / loc.ROW_S
    rel = np.abs(rate - diff).max() / np.abs(diff).max()
    print("dec %g: %.3g relative" % (dec_deg, rel))
    assert rel <= 1e-7
    sidereal = loc.antenna_delay_rates(xyz, s) / loc.ROW_S
    assert np.abs(sidereal - diff).max() / np.abs(diff).max() <= 1e-6


def test_track_model_columns():
    loc = importlib.import_module("vlite-fast_amd.localise")
    rng = np.random.default_rng(4)
    xyz = np.array([-1601185.4, -5041977.5, 3554875.9]) + rng.uniform(-5e3, 5e3, (4, 3))
    unix, ra, dec = 1700000000.0, np.radians(83.6), np.radians(22.0)
    clock = np.array([0.0, 12.5, -3.0, 40.0])
    m = loc.track_model(xyz, ra, dec, unix, clock)
    s = loc.source_vector(ra, dec, unix)
    assert m.shape == (4, 4) and m.dtype == np.float64
    assert np.array_equal(m[:, 0], loc.antenna_delays(xyz, s, clock))
    assert np.array_equal(m[:, 1], loc.antenna_delay_rates(xyz, s, unix))
    assert np.array_equal(m[:, 2], 3.0 * m[:, 0]) and np.array_equal(m[:, 3], 3.0 * m[:, 1])
    # a kilometre of east-west baseline drifts by a few nanoseconds a second: 10^-5 samples per row at most here
    assert 0 < np.abs(m[:, 1] - m[0, 1]).max() < 1e-4
