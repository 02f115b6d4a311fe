"""A seeded array source with an undispersed burst, beside tests/array_synth.py: every antenna sees noise of its own, and
over the rows r0 .. r1 - 1 also a common Gaussian row -- circularly delayed by delays[a] samples as array_synth delays
it -- of `power` times the noise's power.  Outside the burst the antennas share nothing, so a coherent beam gains over a
single antenna only where the burst is.  Digitised as array_synth digitises.  The generator is numpy's."""
import numpy as np

from array_synth import MEAN, NFFT, SIGMA


def burst_antennas(seed, nrows, delays, r0, r1, power):
    """u8 [A][2][nrows * 12500]"""
    delays = np.asarray(delays, np.float64)
    A = delays.shape[0]
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((A, 2, nrows, NFFT))
    common = rng.standard_normal((2, r1 - r0, NFFT))
    k = np.arange(NFFT // 2 + 1, dtype=np.float64)
    spec = np.fft.rfft(common, axis=-1)
    for a in range(A):
        t = -k * (delays[a] / NFFT)
        factor = np.exp(2j * np.pi * (t - np.rint(t)))
        factor[0] = factor[-1] = 1.0
        c = np.fft.irfft(spec * factor, n=NFFT, axis=-1)
        v[a, :, r0:r1] += np.sqrt(power) * c / c.std(axis=-1, keepdims=True)
    g = v * SIGMA + MEAN
    g = np.where(g <= 0, 0, np.where(g >= 255, 255, np.floor(g)))
    return g.astype(np.uint8).reshape(A, 2, nrows * NFFT)
