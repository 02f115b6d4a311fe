"""CPU reference of the beamformer (include/pb_hip.h: pb_beamform): a numpy restatement of the
definition, one IEEE binary32 (for the phase, binary64) operation per numpy operation, on spectra such as
correlate_ref.batch_spectra gives.  The phase and the rotation polynomial are the imager's (image_ref)."""
import numpy as np

import image_ref as IR

NCHANOUT = 4096
F = np.float32


def _params(A, delay, psi, gain):
    delay = np.atleast_2d(np.asarray(delay, np.float64))
    assert delay.shape[1] == A
    psi = None if psi is None else np.atleast_2d(np.asarray(psi, np.float64))
    gain = np.ones(delay.shape, F) if gain is None else np.atleast_2d(np.asarray(gain, F))
    assert gain.shape == delay.shape and (psi is None or psi.shape == delay.shape)
    return delay, psi, gain


def weights(delay, psi=None, gain=None):
    """delay, psi float64 [nbeam][A], gain float32 [nbeam][A] -> (wr, wi) float32 [nbeam][A][4096]"""
    delay, psi, gain = _params(np.atleast_2d(delay).shape[1], delay, psi, gain)
    cr, sr = IR.rotation(IR.phase(delay, psi))
    g = gain[..., None]
    return g * cr, g * sr


def detect(X, delay, psi=None, gain=None):
    """X complex64 [A][2][T][4096] -> the detected beam of every row, float32 [nbeam][T][4][4096] (AA, BB, CR, CI)"""
    A, T = X.shape[0], X.shape[2]
    wr, wi = weights(*_params(A, delay, psi, gain))
    xr = np.ascontiguousarray(X.real, F)
    xi = np.ascontiguousarray(X.imag, F)
    out = np.zeros((wr.shape[0], T, 4, NCHANOUT), F)
    for b in range(wr.shape[0]):
        yr = np.zeros((2, T, NCHANOUT), F)
        yi = np.zeros((2, T, NCHANOUT), F)
        for a in range(A):
            w_r, w_i = wr[b, a], wi[b, a]                  # [4096], the same for every pol and row
            tr = xr[a] * w_r - xi[a] * w_i
            ti = xi[a] * w_r + xr[a] * w_i
            yr = yr + tr
            yi = yi + ti
        ar, ai, br, bi = yr[0], yi[0], yr[1], yi[1]
        out[b, :, 0] = ar * ar + ai * ai
        out[b, :, 1] = br * br + bi * bi
        out[b, :, 2] = ar * br + ai * bi
        out[b, :, 3] = ai * br - ar * bi
    return out


def _starts(T, shift, tscr, nout):
    shift = np.zeros(NCHANOUT, np.int64) if shift is None else np.asarray(shift, np.int64)
    assert shift.shape == (NCHANOUT,) and shift.min() >= 0 and tscr >= 1 and nout >= 1
    assert shift.max() + nout * tscr <= T
    return shift[None, :] + (np.arange(nout, dtype=np.int64) * tscr)[:, None]          # [nout][4096]


def integrate(P, shift, tscr, nout):
    """P float32 [nbeam][T][4][4096] -> float32 [nbeam][nout][4][4096]: the rows of each window added in row order"""
    start = _starts(P.shape[1], shift, tscr, nout)
    ch = np.arange(NCHANOUT)
    out = np.zeros((P.shape[0], nout, 4, NCHANOUT), F)
    for k in range(tscr):
        rows = start + k
        for q in range(4):
            out[:, :, q] = out[:, :, q] + P[:, rows, q, ch]
    return out


def rows_used(w, T, gain, shift, tscr, nout):
    """w float32 [A][T] row weights, or None for the raw stream; gain float32 [nbeam][A] -> int32 [nbeam][nout][4096]"""
    gain = np.atleast_2d(np.asarray(gain, F))
    start = _starts(T, shift, tscr, nout)
    out = np.full((gain.shape[0], nout, NCHANOUT), tscr, np.int32)
    if w is None:
        return out
    for b in range(gain.shape[0]):
        ok = np.ones(T, bool)
        for a in range(gain.shape[1]):
            if gain[b, a] != 0:
                ok &= w[a, :T] > 0
        P = np.concatenate([[0], np.cumsum(ok)])
        out[b] = P[start + tscr] - P[start]
    return out


def beamform(X, w, delay, psi=None, gain=None, shift=None, tscr=1, nout=None, detected=None):
    """X complex64 [A][2][T][4096]; w [A][T] row weights, or None for the raw stream -> (beams float32
    [nbeam][nout][4][4096], rows_used int32 [nbeam][nout][4096]), both bit for bit what the library returns.
    detected: detect(X, delay, psi, gain) where the caller already has it."""
    A, T = X.shape[0], X.shape[2]
    delay, psi, gain = _params(A, delay, psi, gain)
    if nout is None:
        nout = (T - (0 if shift is None else int(np.max(shift)))) // tscr
    P = detect(X, delay, psi, gain) if detected is None else detected
    return integrate(P, shift, tscr, nout), rows_used(w, T, gain, shift, tscr, nout)
