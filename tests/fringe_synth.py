"""array_synth's seeded source with a delay and a phase that drift from row to row, for the tests of the fringe-stopping
correlator (pb_correlate_tracked): antenna a sees the common row t delayed by d0[a] + d1[a] t samples and turned by
p0[a] + p1[a] t turns.  Generator, band and digitiser are array_synth's: with d1 = p1 = 0 the voltages are
array_synth.voltages' bit for bit."""
import numpy as np

from array_synth import CHANMIN, MEAN, NCHANOUT, NFFT, SIGMA


def voltages(seed, nrows, d0, d1, p0, p1, shared=0.5):
    """float64 [A][2][nrows][12500], unit variance: sqrt(shared) of the common row, delayed by d0 + d1 t and turned by
    p0 + p1 t in row t, plus sqrt(1 - shared) of the antenna's own noise"""
    d0, d1, p0, p1 = (np.asarray(v, np.float64) for v in (d0, d1, p0, p1))
    assert d0.ndim == 1 and d1.shape == p0.shape == p1.shape == d0.shape and 0.0 <= shared <= 1.0
    A = d0.shape[0]
    rng = np.random.default_rng(seed)
    common = rng.standard_normal((2, nrows, NFFT))
    own = rng.standard_normal((A, 2, nrows, NFFT))
    k = np.arange(NFFT // 2 + 1, dtype=np.float64)
    spec = np.fft.rfft(common, axis=-1)
    rows = np.arange(nrows, dtype=np.float64)[:, None]
    out = np.empty((A, 2, nrows, NFFT))
    for a in range(A):
        t = (p0[a] + p1[a] * rows) - k * ((d0[a] + d1[a] * rows) / NFFT)      # [nrows][6251]
        factor = np.exp(2j * np.pi * (t - np.rint(t)))
        factor[:, 0] = factor[:, -1] = 1.0
        v = np.fft.irfft(spec * factor, n=NFFT, axis=-1)
        v = v / v.std(axis=-1, keepdims=True)
        out[a] = np.sqrt(shared) * v + np.sqrt(1.0 - shared) * own[a]
    return out


def drifting_antennas(seed, nrows, d0, d1, p0, p1, shared=0.5):
    """u8 [A][2][nrows * 12500]: voltages() digitised as array_synth.phased_antennas digitises"""
    g = voltages(seed, nrows, d0, d1, p0, p1, shared) * SIGMA + MEAN
    g = np.where(g <= 0, 0, np.where(g >= 255, 255, np.floor(g)))
    return g.astype(np.uint8).reshape(len(d0), 2, nrows * NFFT)


def spectra_of_codes(u8, nrows):
    """u8 [A][2][nrows * 12500] -> complex128 [A][2][nrows][4096]: the in-band numpy.fft.rfft rows of the codes - 128"""
    v = u8.astype(np.float64) - 128.0
    return np.fft.rfft(v.reshape(u8.shape[0], 2, nrows, NFFT), axis=-1)[..., CHANMIN:CHANMIN + NCHANOUT]


# ---- the drifting source that the CPU and the GPU tests share (three antennas, 24 rows) ----
SEED, ROWS, SHARED = 7, 24, 0.5
D0, D1 = (0.0, 58.25, 131.4), (0.0, 0.02, -0.035)
P0, P1 = (0.0, 0.1, -0.3), (0.0, 1.0 / 24, -2.0 / 24)


def model_of(d0, d1, p0, p1):
    """the pb_correlate_tracked model that stops a source made with (d0, d1, p0, p1): float64 [A][4]"""
    return np.stack([np.asarray(d0, float), np.asarray(d1, float), -np.asarray(p0, float), -np.asarray(p1, float)], axis=-1)


def band_coherence(vis, bls, prod=0):
    """vis complex [nbl][4][4096] of one gate in the correlator's baseline order (bls) -> {(i, j): |sum_c V(c)| /
    sum_c sqrt(auto_i(c) auto_j(c))} over the cross baselines, for product `prod`"""
    index = dict((b, k) for k, b in enumerate(bls))
    vis = np.asarray(vis, np.complex128)
    out = {}
    for (i, j), k in index.items():
        if i != j:
            norm = np.sqrt(vis[index[(i, i)], prod].real * vis[index[(j, j)], prod].real).sum()
            out[(i, j)] = abs(vis[k, prod].sum()) / norm
    return out
