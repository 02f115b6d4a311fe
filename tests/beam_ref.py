"""CPU reference of the beamformer (include/pb_hip.h: pb_beamform): a numpy restatement of the
definition, one IEEE binary32 (for the phase, binary64) operation per numpy operation, on spectra such as
correlate_ref.batch_spectra gives.  The phase and the rotation polynomial are the imager's (image_ref).  Then the same
beams stated twice in binary64 -- directly (beamform64) and as the quadratic form of the correlator's visibilities
(from_visibilities64) -- and the derived bound that holds the restatement to them (error_bound)."""
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


# ---- binary64 statements of the same beams, and the bound that holds the restatement to them

def weights64(delay, psi=None, gain=None):
    """complex128 [nbeam][A][4096]: w = gain exp(+2 pi i (psi + k delay / 12500)), the phase formed as the definition
    forms it (binary64, reduced by rint), the rotation numpy's"""
    delay, psi, gain = _params(np.atleast_2d(delay).shape[1], delay, psi, gain)
    psi = np.zeros_like(delay) if psi is None else psi
    t = psi[..., None] + IR.BINS * (delay / 12500.0)[..., None]
    return gain.astype(np.float64)[..., None] * np.exp(2j * np.pi * (t - np.rint(t)))


def beamform64(X, delay, psi=None, gain=None, shift=None, tscr=1, nout=None):
    """X complex [A][2][T][4096] -> float64 [nbeam][nout][4][4096]: complex128 throughout, a plain sum over the
    antennas, |.|^2 and A conj(B), the windows' rows added"""
    X = np.asarray(X, np.complex128)
    A, T = X.shape[0], X.shape[2]
    W = weights64(*_params(A, delay, psi, gain))
    if nout is None:
        nout = (T - (0 if shift is None else int(np.max(shift)))) // tscr
    start = _starts(T, shift, tscr, nout)
    ch = np.arange(NCHANOUT)
    out = np.zeros((W.shape[0], nout, 4, NCHANOUT))
    for b in range(W.shape[0]):
        y = (X * W[b][:, None, None, :]).sum(axis=0)                 # [2][T][4096]
        c = y[0] * np.conj(y[1])
        P = np.stack([np.abs(y[0]) ** 2, np.abs(y[1]) ** 2, c.real, c.imag], axis=1)      # [T][4][4096]
        for k in range(tscr):
            out[b] += np.moveaxis(P[start + k, :, ch], -1, 1)         # [nout][4096][4] -> [nout][4][4096]
    return out


def from_visibilities64(vis, delay, psi=None, gain=None):
    """vis complex [ngate][nbl][4][4096] in the correlator's baseline order (product 2p + q = X_i^p conj(X_j^q), autos
    included) -> float64 [nbeam][ngate][4][4096]: the beams whose windows are the gates, as the quadratic form of the
    visibilities.  With w_a = g_a exp(+2 pi i phi_a): y^p conj(y^q) = sum over every ordered pair (i, j) of
    w_i conj(w_j) V_ij^(pq), and V_ji^(pq) = conj(V_ij^(qp)) gives the pairs below the diagonal.
    AA is (p, q) = (0, 0), BB (1, 1), CR + i CI (0, 1)."""
    import correlate_ref as XR
    vis = np.asarray(vis, np.complex128)
    ngate, nbl = vis.shape[:2]
    A = int(round((np.sqrt(8 * nbl + 1) - 1) / 2))
    bls = XR.baselines(A)
    assert len(bls) == nbl and vis.shape[2:] == (4, NCHANOUT)
    W = weights64(*_params(A, delay, psi, gain))
    out = np.zeros((W.shape[0], ngate, 4, NCHANOUT))
    for b in range(W.shape[0]):
        acc = np.zeros((3, ngate, NCHANOUT), np.complex128)          # (0, 0), (1, 1), (0, 1)
        for k, (i, j) in enumerate(bls):
            ww = W[b, i] * np.conj(W[b, j])
            for n, (p, q) in enumerate(((0, 0), (1, 1), (0, 1))):
                acc[n] += ww * vis[:, k, 2 * p + q]
                if i != j:
                    acc[n] += np.conj(ww) * np.conj(vis[:, k, 2 * q + p])
        out[b, :, 0], out[b, :, 1], out[b, :, 2], out[b, :, 3] = acc[0].real, acc[1].real, acc[2].real, acc[2].imag
    return out


def moduli(X, gain, shift=None, tscr=1, nout=None):
    """S of DESIGN.md section 12, float64 [nbeam][nout][4][4096]: over a window's rows the sum of m^p m^q, where
    m^p = sum over the antennas of |gain_a| |x_a^p| bounds the modulus of every partial sum of a beam voltage;
    (p, q) = (0, 0), (1, 1), (0, 1), (0, 1) for AA, BB, CR, CI"""
    X = np.asarray(X, np.complex128)
    A, T = X.shape[0], X.shape[2]
    gain = np.abs(np.atleast_2d(np.asarray(gain, np.float64)))
    assert gain.shape[1] == A
    if nout is None:
        nout = (T - (0 if shift is None else int(np.max(shift)))) // tscr
    start = _starts(T, shift, tscr, nout)
    ch = np.arange(NCHANOUT)
    mod = np.abs(X)
    out = np.zeros((gain.shape[0], nout, 4, NCHANOUT))
    for b in range(gain.shape[0]):
        m = (mod * gain[b][:, None, None, None]).sum(axis=0)         # [2][T][4096]
        P = np.stack([m[0] * m[0], m[1] * m[1], m[0] * m[1], m[0] * m[1]], axis=1)
        for k in range(tscr):
            out[b] += np.moveaxis(P[start + k, :, ch], -1, 1)
    return out


def error_bound(X, gain, shift=None, tscr=1, nout=None, through="beam"):
    """The first-order bound of DESIGN.md section 12, float64 [nbeam][nout][4][4096], derived and not measured.
    through = "beam": the binary32 restatement (and the kernel, which equals it bit for bit) against beamform64 on the
    same spectra, 2^-24 (2 sqrt(2) (A + 11) + tscr + 1) S.
    through = "vis": from_visibilities64 of the binary32 correlator's visibilities (gates of tscr rows) against the
    same form of the exact ones, which is beamform64: 2^-24 sqrt(2) (tscr + 1) S.
    The two paths differ by at most the sum of the two."""
    A = np.asarray(X).shape[0]
    S = moduli(X, np.ones((1, A)) if gain is None else gain, shift, tscr, nout)
    if through == "beam":
        return 2.0 ** -24 * (2.0 * np.sqrt(2.0) * (A + 11) + tscr + 1) * S
    assert through == "vis"
    return 2.0 ** -24 * np.sqrt(2.0) * (tscr + 1) * S


def five_beams(A, seed):
    """the beams of the cross-checks: delays with fractional parts up to +-20000 samples (one on the ties of rint), psi
    of several turns, gains with zeros, a one-hot row and a negative gain
    -> (delay float64 [5][A], psi float64 [5][A], gain float32 [5][A])"""
    rng = np.random.default_rng(seed)
    delay = rng.uniform(-20000.0, 20000.0, (5, A))
    delay[0, A - 1] = 6250.0
    delay[4, 0] = -0.5
    psi = rng.uniform(-4.0, 4.0, (5, A))
    psi[2, 0] = 0.5
    gain = rng.uniform(0.5, 1.5, (5, A)).astype(F)
    gain[1] = 0
    gain[1, 1 % A] = 1
    gain[2, 0] = 0 if A > 1 else 1
    gain[3, A - 1] = -gain[3, A - 1]
    gain[4, A // 2] = 0 if A > 2 else gain[4, A // 2]
    return delay, psi, gain
