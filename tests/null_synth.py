"""A seeded array source with an interferer, for the tests of the spatial nulls (vlite-fast_amd/nulling.py,
pb_beamform_proj): array_synth's generator -- per pol and FFT row of 12500 samples a common
Gaussian row that antenna a sees circularly delayed and turned -- with a second common row.

  the sky row         delays sky_delays[a], no phase, power `sky` times an antenna's own noise, present only in the rows
                      pulse = (first, last + 1): the pulse a beam at sky_delays adds coherently
  the interferer      delays rfi_delays[a], a seeded phase per (antenna, pol), power `rfi` times the own noise, in every
                      row: one direction per (pol, channel), different in the two pols
  own noise           power 1 per antenna and pol

The sum is scaled so that the off-pulse rows have unit variance and digitised as array_synth digitises.  Nothing here
has to match the reference: the generator is numpy's."""
import importlib

import numpy as np

from array_synth import CHANMIN, MEAN, NCHANOUT, NFFT, SIGMA


def _seen(common, delays, phases):
    """common float64 [2][nrows][12500], delays [A], phases [A][2] turns -> [A][2][nrows][12500]: array_synth's factor
    exp(-2 pi i k d_a / 12500) exp(+2 pi i p_a) on every bin but the real ones, each row back at unit variance"""
    k = np.arange(NFFT // 2 + 1, dtype=np.float64)
    spec = np.fft.rfft(common, axis=-1)
    out = np.empty((len(delays),) + common.shape)
    for a in range(len(delays)):
        for p in range(2):
            t = phases[a, p] - k * (delays[a] / NFFT)
            factor = np.exp(2j * np.pi * (t - np.rint(t)))
            factor[0] = factor[-1] = 1.0
            v = np.fft.irfft(spec[p] * factor, n=NFFT, axis=-1)
            out[a, p] = v / v.std(axis=-1, keepdims=True)
    return out


def rfi_phases(seed, A):
    """the interferer's phase per (antenna, pol), turns in [-0.5, 0.5)"""
    return np.random.default_rng([seed, 1]).uniform(-0.5, 0.5, (A, 2))


def voltages(seed, nrows, sky_delays, rfi_delays, rfi=10.0, sky=1.0, pulse=None):
    """float64 [A][2][nrows][12500]; off-pulse rows have unit variance"""
    sky_delays = np.asarray(sky_delays, np.float64)
    rfi_delays = np.asarray(rfi_delays, np.float64)
    assert sky_delays.ndim == 1 and rfi_delays.shape == sky_delays.shape and rfi >= 0 and sky >= 0
    A = sky_delays.shape[0]
    rng = np.random.default_rng([seed, 0])
    common = rng.standard_normal((2, 2, nrows, NFFT))           # (sky, interferer)
    own = rng.standard_normal((A, 2, nrows, NFFT))
    on = np.zeros(nrows)
    if pulse is not None:
        assert 0 <= pulse[0] < pulse[1] <= nrows
        on[pulse[0]:pulse[1]] = 1.0
    v = own + np.sqrt(rfi) * _seen(common[1], rfi_delays, rfi_phases(seed, A))
    v = v + np.sqrt(sky) * on[None, None, :, None] * _seen(common[0], sky_delays, np.zeros((A, 2)))
    return v / np.sqrt(1.0 + rfi)


def antennas(seed, nrows, sky_delays, rfi_delays, rfi=10.0, sky=1.0, pulse=None):
    """u8 [A][2][nrows * 12500]: voltages() digitised (mean 128.5, sigma 16.9 codes, floor, clipped to 0..255)"""
    g = voltages(seed, nrows, sky_delays, rfi_delays, rfi, sky, pulse) * SIGMA + MEAN
    g = np.where(g <= 0, 0, np.where(g >= 255, 255, np.floor(g)))
    return g.astype(np.uint8).reshape(len(sky_delays), 2, nrows * NFFT)


def rfft_spectra(u8, nrows):
    """u8 [A][2][nrows * 12500] -> complex64 [A][2][nrows][4096]: the in-band numpy.fft.rfft rows of the codes"""
    x = u8.reshape(u8.shape[0], 2, nrows, NFFT).astype(np.float64)
    return np.fft.rfft(x, axis=-1)[..., CHANMIN:CHANMIN + NCHANOUT].astype(np.complex64)


# the case of DESIGN.md section 13: four antennas, an interferer of ten times the own noise, a pulse of the own noise's
# power in rows 52 .. 59 of 64, projectors trained on rows 0 .. 47
CASE = dict(seed=11, nrows=64, sky_delays=(0.0, 58.25, 131.4, -77.7), rfi_delays=(0.0, -312.6, 95.3, 401.9), rfi=10.0,
            sky=1.0, pulse=(52, 60))
TRAIN = (0, 48)
OFF_ROWS = (48, 49, 50, 51, 60, 61, 62, 63)
ON_ROWS = tuple(range(52, 60))


def case_antennas():
    return antennas(**CASE)


def levels(beams):
    """beams [1][64][4][4096] at tscr = 1 -> per pol (AA, BB) the band-summed off-pulse level (rows outside both the
    training stretch and the pulse) and the pulse's contrast (on - off) / off: float64 [2], [2]"""
    s = np.asarray(beams, np.float64)[0, :, :2].sum(axis=-1)              # [64][2]
    off = s[list(OFF_ROWS)].mean(axis=0)
    on = s[list(ON_ROWS)].mean(axis=0)
    return off, (on - off) / off


# asked for (the issue's figures; theory for A = 4, r = 10 n, s = n, K = 1: off level (A - 1) n / (A (n + r)) = 0.068,
# contrast ((A - 1) s / n) / (A s / (n + r)) = 8.25)
OFF_RATIO_MAX = 0.09
CONTRAST_RATIO_MIN = 6.5


def report(name, plain, nulled):
    """prints the figures of one projector and returns (off level nulled / un-nulled, contrast nulled / un-nulled),
    each float64 [2 pols]"""
    off0, con0 = levels(plain)
    off1, con1 = levels(nulled)
    for p in range(2):
        print("%s pol %d: off-pulse level %.4g -> %.4g (ratio %.4f, asked <= %.2f, theory 0.068); contrast %.4f -> %.4f "
              "(ratio %.3f, asked >= %.1f, theory 8.25)" % (name, p, off0[p], off1[p], off1[p] / off0[p], OFF_RATIO_MAX,
                                                            con0[p], con1[p], con1[p] / con0[p], CONTRAST_RATIO_MIN))
    return off1 / off0, con1 / con0


def physical_checks(A, beam_plain, beam_proj, correlate_gates):
    """What the CPU and the GPU test of the physical case share.  A antennas; beam_plain()
    -> beams [1][64][4][4096] at the sky's delays, beam_proj(proj) likewise through the matrices; correlate_gates(first
    rows, nrows) -> vis [ngate][nbl][4][4096].  Asserts the issue's two thresholds per pol for the per-pol projectors
    and that the projector of the pol-summed matrix reaches neither."""
    nulling = importlib.import_module("vlite-fast_amd.nulling")
    vis = None
    for first, nrows in nulling.gate_rows(TRAIN[0], TRAIN[1], 16):
        v = correlate_gates(first, nrows).astype(np.complex128).sum(axis=0)
        vis = v if vis is None else vis + v
    cov = nulling.covariances(vis, A)
    proj, count = nulling.projectors(cov, 1)
    assert np.all(count == 1)
    plain = beam_plain()
    off, con = report("per-pol projectors", plain, beam_proj(proj))
    assert np.all(off <= OFF_RATIO_MAX)
    assert np.all(con >= CONTRAST_RATIO_MIN)
    both = cov.sum(axis=0)
    shared, _ = nulling.projectors(np.stack([both, both]), 1)
    off, con = report("one projector from the pol-summed matrix", plain, beam_proj(shared))
    assert np.all(off > OFF_RATIO_MAX)
    assert np.all(con < CONTRAST_RATIO_MIN)
