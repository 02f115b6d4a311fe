"""A seeded array source with fractional delays and per-antenna phases, for the tests that hold the correlator, the
imager and the beamformer to one another (tests/test_array_conventions_cpu.py, tests/test_gpu_array_seam.py).

Per pol and FFT row of 12500 samples a common Gaussian row; antenna a sees it circularly delayed by delays[a] samples
and turned by phases[a] turns -- bin k of its numpy.fft.rfft times exp(-2 pi i k d_a / 12500) exp(+2 pi i p_a), the real
bins 0 and 6250 left alone --, rescaled to unit variance, mixed with noise of its own and digitised as
correlate_ref.delayed_antennas digitises.  A row is exactly one FFT block of a taps = 1 channeliser, so the spectra
that come back are the common row's times that factor, plus the antenna's own noise and the quantisation's.
Nothing here has to match the reference: the generator is numpy's."""
import numpy as np

NFFT, CHANMIN, NCHANOUT = 12500, 2155, 4096
SIGMA, MEAN = 16.9, 128.5


def voltages(seed, nrows, delays, phases, shared=0.5):
    """float64 [A][2][nrows][12500], unit variance: sqrt(shared) of the delayed and turned common row plus
    sqrt(1 - shared) of the antenna's own noise"""
    delays = np.asarray(delays, np.float64)
    phases = np.asarray(phases, np.float64)
    assert delays.ndim == 1 and phases.shape == delays.shape and 0.0 <= shared <= 1.0
    A = delays.shape[0]
    rng = np.random.default_rng(seed)
    common = rng.standard_normal((2, nrows, NFFT))
    own = rng.standard_normal((A, 2, nrows, NFFT))
    k = np.arange(NFFT // 2 + 1, dtype=np.float64)
    spec = np.fft.rfft(common, axis=-1)
    out = np.empty((A, 2, nrows, NFFT))
    for a in range(A):
        t = phases[a] - k * (delays[a] / NFFT)
        factor = np.exp(2j * np.pi * (t - np.rint(t)))
        factor[0] = factor[-1] = 1.0
        v = np.fft.irfft(spec * factor, n=NFFT, axis=-1)
        v = v / v.std(axis=-1, keepdims=True)
        out[a] = np.sqrt(shared) * v + np.sqrt(1.0 - shared) * own[a]
    return out


def phased_antennas(seed, nrows, delays, phases, shared=0.5):
    """u8 [A][2][nrows * 12500]: voltages() digitised (mean 128.5, sigma 16.9 codes, floor, clipped to 0..255)"""
    g = voltages(seed, nrows, delays, phases, shared) * SIGMA + MEAN
    g = np.where(g <= 0, 0, np.where(g >= 255, 255, np.floor(g)))
    return g.astype(np.uint8).reshape(len(delays), 2, nrows * NFFT)


def spectra64(seed, nrows, delays, phases, shared=0.5):
    """complex128 [A][2][nrows][4096]: the in-band numpy.fft.rfft rows of the voltages before digitising, in codes"""
    v = voltages(seed, nrows, delays, phases, shared) * SIGMA
    return np.fft.rfft(v, axis=-1)[..., CHANMIN:CHANMIN + NCHANOUT]
