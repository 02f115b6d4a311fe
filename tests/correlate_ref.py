"""CPU reference of the correlator (include/pb_hip.h: pb_correlate, pb_correlate_gated): a numpy
float32 restatement of the definition, one IEEE binary32 operation per numpy operation, on top of the spectra and row
weights of coherence_ref.spectra (which come from the oracle).  Also the seeded delayed-antenna voltages the delay
tests share."""
import numpy as np

import coherence_ref as CR
import synth

NFFT, NCHANOUT = 12500, 4096
F = np.float32


def baselines(A):
    return [(i, j) for i in range(A) for j in range(i, A)]


def batch_spectra(O, data, R, rfi_mode):
    """data u8 [A][nseg][2][R*12500] -> {stream: (X complex64 [A][2][nseg*R][4096], w float32 [A][nseg*R])}: the rows of
    a batch counted through its segments, the row weights after apply_kurtosis (the two pols share them)"""
    A, nseg = data.shape[0], data.shape[1]
    out = {}
    for a in range(A):
        for s in range(nseg):
            for st, (X, w) in CR.spectra(O, data[a, s], R, rfi_mode).items():
                assert np.array_equal(w[0], w[1])
                Xs, ws = out.setdefault(st, (np.zeros((A, 2, nseg * R, NCHANOUT), np.complex64), np.ones((A, nseg * R), F)))
                Xs[a, :, s * R:(s + 1) * R] = X
                ws[a, s * R:(s + 1) * R] = w[0]
    return out


def correlate(X, w, row0, nrows):
    """X complex64 [A][2][T][4096]; w [A][T] row weights, or None for the raw stream; row0 int [ngate][4096].
    -> vis complex64 [ngate][nbl][4][4096], rows_used int32 [ngate][nbl][4096]"""
    A, T = X.shape[0], X.shape[2]
    row0 = np.asarray(row0, np.int64)
    assert row0.min() >= 0 and row0.max() + nrows <= T
    bls = baselines(A)
    I = np.array([b[0] for b in bls])
    J = np.array([b[1] for b in bls])
    xr = np.ascontiguousarray(X.real, F)
    xi = np.ascontiguousarray(X.imag, F)
    ch = np.arange(NCHANOUT)
    ngate = row0.shape[0]
    vis = np.zeros((ngate, len(bls), 4, NCHANOUT), np.complex64)
    used = np.zeros((ngate, len(bls), NCHANOUT), np.int32)
    for g in range(ngate):
        acc_re = np.zeros((len(bls), 2, 2, NCHANOUT), F)
        acc_im = np.zeros((len(bls), 2, 2, NCHANOUT), F)
        for k in range(nrows):
            t = row0[g] + k
            vr, vi = xr[:, :, t, ch], xi[:, :, t, ch]             # [A][2][4096]
            ax, ay = vr[I][:, :, None, :], vi[I][:, :, None, :]   # antenna i, pol p
            bx, by = vr[J][:, None, :, :], vi[J][:, None, :, :]   # antenna j, pol q
            re = ax * bx + ay * by
            im = ay * bx - ax * by
            acc_re = acc_re + re
            acc_im = acc_im + im
        vis[g].real = acc_re.reshape(len(bls), 4, NCHANOUT)
        vis[g].imag = acc_im.reshape(len(bls), 4, NCHANOUT)
        if w is None:
            used[g] = nrows
        else:
            for b, (i, j) in enumerate(bls):
                P = np.concatenate([[0], np.cumsum((w[i] > 0) & (w[j] > 0))])
                used[g, b] = P[row0[g] + nrows] - P[row0[g]]
    return vis, used


def uniform_row0(T, int_rows):
    assert T % int_rows == 0
    return np.repeat(np.arange(T // int_rows, dtype=np.int64)[:, None] * int_rows, NCHANOUT, axis=1)


def delayed_antennas(seed, n, delays, shared=0.5):
    """u8 [A][2][n]: per pol a common Gaussian component carrying `shared` of the variance, antenna k seeing it
    delays[k] samples late, plus noise of its own; digitised like synth.baseband_u8 (mean 128.5, sigma 16.9 codes)"""
    delays = [int(d) for d in delays]
    lo, hi = min(delays), max(delays)
    out = np.empty((len(delays), 2, n), np.uint8)
    # synth.gauss(seed) hashes the counter seed + k: neighbouring seeds give the same sequence shifted by one sample, so
    # the independent components are taken 2^32 counts apart of one seed
    for p in range(2):
        common = synth.gauss(seed, n + hi - lo, offset=p << 32)
        for k, d in enumerate(delays):
            own = synth.gauss(seed, n, offset=(2 + 2 * k + p) << 32)
            v = np.sqrt(shared) * common[hi - d:hi - d + n] + np.sqrt(1 - shared) * own
            g = v * 16.9 + 128.5
            out[k, p] = np.where(g <= 0, 0, np.where(g >= 255, 255, np.floor(g))).astype(np.uint8)
    return out
