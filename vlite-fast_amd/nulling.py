"""Spatial nulls for the beamformer: per (pol, channel) the antennas' correlation matrix over a stretch of data, its
dominant eigenvectors -- the interferers -- and the projector that takes them out of the antennas' spectra.

The matrices come from the correlator and the projectors go to the projecting beamformer (include/pb_hip.h:
pb_correlate*, pb_beamform_proj), both on the GPU; everything in this module is host-side numpy in binary64 on small
arrays (reference: analysis/baseband.py do_filter, :1015-1067, and apply_filter, :859-908):

  covariances(vis, nant)                the correlator's visibilities -> C[pol][channel][i][j], Hermitian
  projectors(cov, nnull, min_ratio)     P = I - sum_k v_k v_k^H over the nnull largest eigenvalues' eigenvectors
  filtered_vis(cov, proj)               P C P^H, apply_filter's second output
  gate_rows(row0, row1, rows_per_seg)   a stretch of rows as gates of at most one segment, for PbHandle.correlate_gated
  training_vis(h, stream, nseg, ...)    those gates correlated on the GPU and added in binary64

A matrix is one pol's: C[p][c][i][j] = sum over the rows of X_i^p conj(X_j^p), the correlator's product 2p + p.  The
pols' instrumental phases differ, so an interferer's direction vector differs between them and one projector from the
pol-summed matrix does not null it (DESIGN.md section 13 has the numbers); the reference filters one VDIF thread, which
is one pol, at a time.  The reference takes `evecs[np.argmax(evals)]`, a ROW of numpy.linalg.eigh's result; the
eigenvectors are its COLUMNS, and this module takes columns.
"""
import importlib

import numpy as np

NCHANOUT = 4096


def _baselines(nant):
    return importlib.import_module("vlite-fast_amd.correlate").baselines(nant)


def covariances(vis, nant):
    """vis complex [ngate][nbl][4][4096] (or [nbl][4][4096]) in the library's baseline order -> complex128
    [2][4096][nant][nant]: the gates added in binary64, pol p from product 2p + p, C[j][i] = conj(C[i][j]) below the
    diagonal"""
    vis = np.asarray(vis)
    if vis.ndim == 3:
        vis = vis[None]
    bls = _baselines(nant)
    if vis.ndim != 4 or vis.shape[1:] != (len(bls), 4, NCHANOUT):
        raise ValueError("vis must be [ngate][%d][4][%d]" % (len(bls), NCHANOUT))
    v = vis.astype(np.complex128).sum(axis=0)
    cov = np.zeros((2, NCHANOUT, nant, nant), np.complex128)
    for k, (i, j) in enumerate(bls):
        for p in range(2):
            cov[p, :, i, j] = v[k, 3 * p]
            if i != j:
                cov[p, :, j, i] = np.conj(v[k, 3 * p])
    return cov


def projectors(cov, nnull=1, min_ratio=None):
    """cov complex [2][4096][A][A], Hermitian -> (proj complex64 [2][4096][A][A], null_count int32 [2][4096]).
    Per (pol, channel) P = I - sum_k v_k v_k^H over the eigenvectors (columns of numpy.linalg.eigh's result, unit norm)
    of the nnull largest eigenvalues.  With min_ratio, a channel whose largest eigenvalue is below min_ratio times the
    mean of the others keeps the identity: a clean channel does not pay 1/A of its sensitivity.  A channel whose matrix
    is all zero (zapped, fully excised) keeps the identity too."""
    cov = np.asarray(cov, np.complex128)
    if cov.ndim != 4 or cov.shape[0] != 2 or cov.shape[2] != cov.shape[3]:
        raise ValueError("cov must be [2][nchan][A][A]")
    A = cov.shape[2]
    if not 0 <= nnull <= A - 1:
        raise ValueError("nnull must be 0 .. A - 1")
    if min_ratio is not None and not min_ratio > 0:
        raise ValueError("min_ratio must be positive")
    eye = np.eye(A, dtype=np.complex128)
    proj = np.broadcast_to(eye, cov.shape).copy()
    count = np.zeros(cov.shape[:2], np.int32)
    if nnull == 0:
        return proj.astype(np.complex64), count
    evals, evecs = np.linalg.eigh(cov)                     # ascending; evecs[..., :, k] belongs to evals[..., k]
    null = np.any(cov != 0, axis=(2, 3))
    if min_ratio is not None:
        others = evals[..., :-1].mean(axis=-1)
        null &= evals[..., -1] >= min_ratio * others
    v = evecs[..., :, A - nnull:]                          # [2][nchan][A][nnull]
    full = eye - np.einsum("pcik,pcjk->pcij", v, np.conj(v))
    proj[null] = full[null]
    count[null] = nnull
    return proj.astype(np.complex64), count


def filtered_vis(cov, proj):
    """P C P^H per (pol, channel), complex128 [2][4096][A][A]: the matrices of the projected spectra"""
    cov = np.asarray(cov, np.complex128)
    P = np.asarray(proj, np.complex128)
    return np.einsum("pcij,pcjk,pclk->pcil", P, cov, np.conj(P))


def gate_rows(row0, row1, rows_per_seg):
    """rows row0 .. row1 - 1 of a batch as gates of at most one segment: [(first rows, rows per gate)], one entry per
    call of correlate_gated (its gates are all of one length): the whole gates, then the rest"""
    if not 0 <= row0 < row1:
        raise ValueError("the training rows must be 0 <= ROW0 < ROW1")
    n = row1 - row0
    g = min(rows_per_seg, n)
    calls = [(list(range(row0, row0 + n // g * g, g)), g)]
    if n % g:
        calls.append(([row0 + n // g * g], n % g))
    return calls


def training_vis(h, stream, nseg, row0=0, row1=None):
    """the selected set's rows row0 .. row1 - 1 (by default the whole batch) correlated in gates of at most one segment
    and added on the host -> complex128 [nbl][4][4096]"""
    row1 = nseg * h.rows if row1 is None else row1
    if row1 > nseg * h.rows:
        raise ValueError("the training rows leave the batch's %d rows" % (nseg * h.rows))
    total = None
    for first, nrows in gate_rows(row0, row1, h.rows):
        gates = np.repeat(np.asarray(first, np.int32)[:, None], NCHANOUT, axis=1)
        vis, _ = h.correlate_gated(stream, nseg, gates, nrows)
        v = vis.astype(np.complex128).sum(axis=0)
        total = v if total is None else total + v
    return total
