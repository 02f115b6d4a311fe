"""CPU reference of the fringe-stopping correlator (include/pb_hip.h: pb_correlate_tracked): a
numpy restatement of the definition -- the model's tables in binary64, the rotation of image_ref, the voltage lines in
binary32, then correlate_ref.correlate on the turned spectra -- and a binary64 evaluation of the same sums to bound it
with."""
import numpy as np

import correlate_ref as XR
import image_ref as IR

F = np.float32


def tables(model, T, row_base=0):
    """model float64 [A][4] = delay0, delay_rate, psi0, psi_rate -> (s, p) float64 [A][T]: the delay's slope in turns per
    bin and the phase in turns of every row, each operation rounded once"""
    model = np.asarray(model, np.float64)
    assert model.ndim == 2 and model.shape[1] == 4
    tau = (np.int64(row_base) + np.arange(T, dtype=np.int64)).astype(np.float64)[None, :]
    d = model[:, 0:1] + model[:, 1:2] * tau
    p = model[:, 2:3] + model[:, 3:4] * tau
    return d / 12500.0, p


def turns(model, T, row_base=0):
    """-> (turn float64 [A][T][4096], r float32 [A][T][4096])"""
    s, p = tables(model, T, row_base)
    turn = p[..., None] + IR.BINS * s[..., None]
    return turn, (turn - np.rint(turn)).astype(F)


def turned(X, model, row_base=0):
    """X complex64 [A][2][T][4096] -> X' complex64, the voltage lines in binary32, both pols sharing the rotation"""
    X = np.asarray(X, np.complex64)
    cr, sr = IR.rotation(turns(model, X.shape[2], row_base)[1])
    cr, sr = cr[:, None], sr[:, None]
    xr, xi = np.ascontiguousarray(X.real, F), np.ascontiguousarray(X.imag, F)
    out = np.empty_like(X)
    out.real = xr * cr - xi * sr
    out.imag = xi * cr + xr * sr
    return out


def correlate_tracked(X, w, row0, nrows, model, row_base=0):
    """what pb_correlate_tracked returns, bit for bit: (vis complex64 [ngate][nbl][4][4096], rows_used int32)"""
    return XR.correlate(turned(X, model, row_base), w, row0, nrows)


def turned64(X, model, row_base=0):
    """X complex [A][2][T][4096] -> X exp(+2 pi i turn) in binary64"""
    X = np.asarray(X, np.complex128)
    turn = turns(model, X.shape[2], row_base)[0]
    return X * np.exp(2j * np.pi * (turn - np.rint(turn)))[:, None]


def correlate64(X, row0, nrows, model=None, row_base=0):
    """the same sums evaluated directly in binary64 (model None: of X itself): vis complex128 [ngate][nbl][4][4096]"""
    Xt = np.asarray(X, np.complex128) if model is None else turned64(X, model, row_base)
    A = Xt.shape[0]
    row0 = np.asarray(row0, np.int64)
    bls = XR.baselines(A)
    ch = np.arange(XR.NCHANOUT)
    vis = np.zeros((row0.shape[0], len(bls), 4, XR.NCHANOUT), np.complex128)
    for g in range(row0.shape[0]):
        for k in range(nrows):
            v = Xt[:, :, row0[g] + k, ch]                       # [A][2][4096]
            for b, (i, j) in enumerate(bls):
                vis[g, b] += (v[i][:, None, :] * np.conj(v[j])[None, :, :]).reshape(4, -1)
    return vis
