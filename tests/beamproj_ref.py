"""CPU reference of the projecting beamformer (include/pb_hip.h: pb_beamform_proj): a numpy
restatement of the definition, one IEEE binary32 operation per numpy operation, on spectra such as
correlate_ref.batch_spectra gives.  The steering weights, the integration and the row counts are beam_ref's functions,
called, not copied.  beam_ref.detect forms the voltage and detects it in one function with one weight for both pols, so
the voltage with a weight per pol -- the one thing the definition changes -- and the four detection lines behind it
are stated here; test_beamproj_ref_cpu holds them to beam_ref.detect as numbers (proj = the unit matrix).  Then the same
beams in binary64, directly (beamform64) and as the quadratic form w' V w'^H of the correlator's visibilities
(from_visibilities64), and the derived bound that holds the restatement to them (error_bound)."""
import numpy as np

import beam_ref as BR
import correlate_ref as XR

NCHANOUT = BR.NCHANOUT
F = np.float32


def _proj(proj, A):
    proj = np.asarray(proj)
    assert proj.shape == (2, NCHANOUT, A, A) and np.all(np.isfinite(proj))
    return proj.astype(np.complex64)


def weights(proj, delay, psi=None, gain=None):
    """proj complex64 [2][4096][A][A] -> (ur, ui) float32 [nbeam][2][A][4096]: w'[b][p][j][c], rows of proj ascending"""
    sr, si = BR.weights(delay, psi, gain)                      # [nbeam][A][4096]
    sr, si = np.asarray(sr, F), np.asarray(si, F)
    A = sr.shape[1]
    proj = _proj(proj, A)
    pr = np.ascontiguousarray(proj.real, F)
    pi = np.ascontiguousarray(proj.imag, F)
    ur = np.zeros((sr.shape[0], 2, A, NCHANOUT), F)
    ui = np.zeros_like(ur)
    for a in range(A):
        s_r, s_i = sr[:, None, a, None, :], si[:, None, a, None, :]          # [nbeam][1][1][4096]
        p_r = np.moveaxis(pr[:, :, a, :], 1, 2)[None]                         # [1][2][A (j)][4096]
        p_i = np.moveaxis(pi[:, :, a, :], 1, 2)[None]
        tr = s_r * p_r - s_i * p_i
        ti = s_i * p_r + s_r * p_i
        ur = ur + tr
        ui = ui + ti
    return ur, ui


def detect(X, ur, ui):
    """X complex64 [A][2][T][4096], (ur, ui) float32 [nbeam][2][A][4096] -> the detected beam of every row, float32
    [nbeam][T][4][4096] (AA, BB, CR, CI): beam_ref.detect's lines, pol p with its own weights"""
    A, T = X.shape[0], X.shape[2]
    xr = np.ascontiguousarray(X.real, F)
    xi = np.ascontiguousarray(X.imag, F)
    out = np.zeros((ur.shape[0], T, 4, NCHANOUT), F)
    for b in range(ur.shape[0]):
        yr = np.zeros((2, T, NCHANOUT), F)
        yi = np.zeros((2, T, NCHANOUT), F)
        for j in range(A):
            w_r, w_i = ur[b, :, j, None, :], ui[b, :, j, None, :]             # [2][1][4096]: per pol, every row
            tr = xr[j] * w_r - xi[j] * w_i
            ti = xi[j] * w_r + xr[j] * w_i
            yr = yr + tr
            yi = yi + ti
        ar, ai, br, bi = yr[0], yi[0], yr[1], yi[1]
        out[b, :, 0] = ar * ar + ai * ai
        out[b, :, 1] = br * br + bi * bi
        out[b, :, 2] = ar * br + ai * bi
        out[b, :, 3] = ai * br - ar * bi
    return out


def rows_used(w, T, nbeam, A, shift, tscr, nout):
    """every antenna of the handle counts, whatever the gains: beam_ref.rows_used with gains of one"""
    return BR.rows_used(w, T, np.ones((nbeam, A), F), shift, tscr, nout)


def beamform_proj(X, w, delay, proj, psi=None, gain=None, shift=None, tscr=1, nout=None, detected=None):
    """X complex64 [A][2][T][4096]; w [A][T] row weights, or None for the raw stream; proj complex64 [2][4096][A][A]
    -> (beams float32 [nbeam][nout][4][4096], rows_used int32 [nbeam][nout][4096]), both bit for bit what the library
    returns.  detected: detect(X, *weights(proj, delay, psi, gain)) where the caller already has it."""
    A, T = X.shape[0], X.shape[2]
    delay = np.atleast_2d(np.asarray(delay, np.float64))
    if nout is None:
        nout = (T - (0 if shift is None else int(np.max(shift)))) // tscr
    P = detect(X, *weights(proj, delay, psi, gain)) if detected is None else detected
    return BR.integrate(P, shift, tscr, nout), rows_used(w, T, delay.shape[0], A, shift, tscr, nout)


# ---- binary64 statements of the same beams, and the bound that holds the restatement to them

def weights64(proj, delay, psi=None, gain=None):
    """complex128 [nbeam][2][A][4096]: w' = s^T P with s = beam_ref.weights64 and the complex64 proj taken exactly"""
    s = BR.weights64(delay, psi, gain)                          # [nbeam][A][4096]
    P = _proj(proj, s.shape[1]).astype(np.complex128)
    return np.einsum("bac,pcaj->bpjc", s, P)


def _window_sum(P, T, shift, tscr, nout):
    """P [T][4][4096] -> [nout][4][4096]: the windows' rows added"""
    start = BR._starts(T, shift, tscr, nout)
    ch = np.arange(NCHANOUT)
    out = np.zeros((nout, 4, NCHANOUT))
    for k in range(tscr):
        out += np.moveaxis(P[start + k, :, ch], -1, 1)
    return out


def beamform64(X, W, shift=None, tscr=1, nout=None):
    """X complex [A][2][T][4096], W complex128 [nbeam][2][A][4096] (weights64) -> float64 [nbeam][nout][4][4096]"""
    X = np.asarray(X, np.complex128)
    T = X.shape[2]
    if nout is None:
        nout = (T - (0 if shift is None else int(np.max(shift)))) // tscr
    out = np.zeros((W.shape[0], nout, 4, NCHANOUT))
    for b in range(W.shape[0]):
        y = np.einsum("aptc,pac->ptc", X, W[b])
        c = y[0] * np.conj(y[1])
        P = np.stack([np.abs(y[0]) ** 2, np.abs(y[1]) ** 2, c.real, c.imag], axis=1)
        out[b] = _window_sum(P, T, shift, tscr, nout)
    return out


def from_visibilities64(vis, W):
    """vis complex [ngate][nbl][4][4096] in the correlator's baseline order, W complex128 [nbeam][2][A][4096] -> float64
    [nbeam][ngate][4][4096]: y^p conj(y^q) = sum over every ordered pair (i, j) of w'^p_i conj(w'^q_j) V_ij^(pq), with
    V_ji^(pq) = conj(V_ij^(qp)) below the diagonal; AA is (p, q) = (0, 0), BB (1, 1), CR + i CI (0, 1)"""
    vis = np.asarray(vis, np.complex128)
    ngate, nbl = vis.shape[:2]
    A = W.shape[2]
    bls = XR.baselines(A)
    assert len(bls) == nbl and vis.shape[2:] == (4, NCHANOUT)
    out = np.zeros((W.shape[0], ngate, 4, NCHANOUT))
    for b in range(W.shape[0]):
        acc = np.zeros((3, ngate, NCHANOUT), np.complex128)
        for k, (i, j) in enumerate(bls):
            for n, (p, q) in enumerate(((0, 0), (1, 1), (0, 1))):
                acc[n] += W[b, p, i] * np.conj(W[b, q, j]) * vis[:, k, 2 * p + q]
                if i != j:
                    acc[n] += W[b, p, j] * np.conj(W[b, q, i]) * np.conj(vis[:, k, 2 * q + p])
        out[b, :, 0], out[b, :, 1], out[b, :, 2], out[b, :, 3] = acc[0].real, acc[1].real, acc[2].real, acc[2].imag
    return out


def moduli(X, proj, gain, shift=None, tscr=1, nout=None):
    """S of DESIGN.md section 13, float64 [nbeam][nout][4][4096]: over a window's rows the sum of m^p m^q, where
    m^p = sum_j mu^p_j |x_j^p| and mu^p_j = sum_a |gain_a| |proj[p][c][a][j]| bounds the modulus of every partial sum of
    w'^p_j; (p, q) = (0, 0), (1, 1), (0, 1), (0, 1) for AA, BB, CR, CI"""
    X = np.asarray(X, np.complex128)
    A, T = X.shape[0], X.shape[2]
    gain = np.abs(np.atleast_2d(np.asarray(gain, np.float64)))
    aP = np.abs(_proj(proj, A).astype(np.complex128))           # [2][4096][A][A]
    if nout is None:
        nout = (T - (0 if shift is None else int(np.max(shift)))) // tscr
    mod = np.abs(X)
    out = np.zeros((gain.shape[0], nout, 4, NCHANOUT))
    for b in range(gain.shape[0]):
        mu = np.einsum("a,pcaj->pjc", gain[b], aP)
        m = np.einsum("jptc,pjc->ptc", mod, mu)
        P = np.stack([m[0] * m[0], m[1] * m[1], m[0] * m[1], m[0] * m[1]], axis=1)
        out[b] = _window_sum(P, T, shift, tscr, nout)
    return out


def error_bound(X, proj, gain, shift=None, tscr=1, nout=None, through="beam"):
    """The first-order bound of DESIGN.md section 13, float64 [nbeam][nout][4][4096], derived and not measured.
    through = "beam": the binary32 restatement (and the kernel, which equals it bit for bit) against beamform64 of
    weights64 on the same spectra, 2^-24 (2 sqrt(2) (A + 11) + 4 (A + 1) + tscr + 1) S: section 12's B_beam with the
    weight's error raised from 10 u to (10 + sqrt(2) (A + 1)) u by the A terms of two products and a sum.
    through = "vis": from_visibilities64 of the binary32 correlator's visibilities (gates of tscr rows) against the same
    form of the exact ones, which is beamform64: 2^-24 sqrt(2) (tscr + 1) S."""
    A = np.asarray(X).shape[0]
    nbeam = 1 if gain is None else np.atleast_2d(gain).shape[0]
    S = moduli(X, proj, np.ones((nbeam, A)) if gain is None else gain, shift, tscr, nout)
    if through == "beam":
        return 2.0 ** -24 * (2.0 * np.sqrt(2.0) * (A + 11) + 4.0 * (A + 1) + tscr + 1) * S
    assert through == "vis"
    return 2.0 ** -24 * np.sqrt(2.0) * (tscr + 1) * S


def random_proj(A, seed):
    """a non-Hermitian complex64 [2][4096][A][A] with exact zeros in about a tenth of its entries, one all-zero
    (pol, channel) and the unit matrix in another"""
    rng = np.random.default_rng(seed)
    P = (rng.standard_normal((2, NCHANOUT, A, A)) + 1j * rng.standard_normal((2, NCHANOUT, A, A))).astype(np.complex64)
    P[rng.random(P.shape) < 0.1] = 0
    P[0, 17] = 0
    P[1, 4000] = np.eye(A, dtype=np.complex64)
    return P


def identity(A):
    return np.broadcast_to(np.eye(A, dtype=np.complex64), (2, NCHANOUT, A, A)).copy()
