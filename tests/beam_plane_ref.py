"""NumPy restatement of pb_beam_planes' definition (include/pb_hip.h), operation by operation, on what pb_beamform (or
pb_beamform_proj) returns for the same arguments: I = AA + BB, ratio = tscr / used, J = I * ratio in binary32; the level
per (beam, channel) as binary64 sums over chunks of 32 output samples in ascending order, the chunk sums added in
ascending order, over the count of samples with used > 0, rounded to binary32; plane = (J / Le - 1) * sqrtf(2 tscr) with
Le the caller's level or the planes' own, +0.0f where used == 0 or Le is not > 0."""
import numpy as np

CHUNK = 32
F = np.float32


def power(beams, used, tscr):
    """J float32 [nbeam][nout][nchan] (meaningless where used == 0)"""
    beams = np.asarray(beams, F)
    with np.errstate(all="ignore"):
        I = beams[:, :, 0] + beams[:, :, 1]
        ratio = F(tscr) / np.asarray(used).astype(F)
        J = I * ratio
    assert J.dtype == F
    return J


def level(J, used):
    """L float32 [nbeam][nchan]: the chunked binary64 sum over the samples with used > 0, over their number"""
    nbeam, nout, nchan = J.shape
    ok = np.asarray(used) > 0
    total = np.zeros((nbeam, nchan), np.float64)
    for s0 in range(0, nout, CHUNK):
        chunk = np.zeros((nbeam, nchan), np.float64)
        for s in range(s0, min(s0 + CHUNK, nout)):
            chunk = np.where(ok[:, s], chunk + J[:, s].astype(np.float64), chunk)
        total = total + chunk
    n = ok.sum(axis=1)
    with np.errstate(all="ignore"):
        return np.where(n > 0, (total / n.astype(np.float64)).astype(F), F(0)).astype(F)


def planes(beams, used, tscr, level_in=None):
    """beams float32 [nbeam][nout][4][nchan], used int32 [nbeam][nout][nchan] -> (plane float32 [nbeam][nout][nchan],
    L float32 [nbeam][nchan])"""
    used = np.asarray(used)
    J = power(beams, used, tscr)
    L = level(J, used)
    Le = L if level_in is None else np.asarray(level_in, F)
    g = np.sqrt(F(2 * tscr))
    assert g.dtype == F
    with np.errstate(all="ignore"):
        q = J / Le[:, None, :]
        d = q - F(1)
        v = d * g
    assert v.dtype == F
    return np.where((used > 0) & (Le[:, None, :] > 0), v, F(0)).astype(F), L
