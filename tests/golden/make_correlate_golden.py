#!/usr/bin/env python3
"""Generate tests/golden/reference_correlate.npz by IMPORTING the reference's Python analysis code.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):
    python tests/golden/make_correlate_golden.py

What is pinned:
  analysis/baseband.py:807  correlate(bbi, nchunk)      the per-channel correlation matrix over FFT chunks
  analysis/baseband.py:741  get_delays(cmatrix)         the lag of each baseline
  analysis/baseband.py:773  fit_delays(delays)          the per-antenna delays

Only the inputs' parameters (the voltages are regenerated from tests/correlate_ref.delayed_antennas, i.e. from
tests/golden/synth.py) and the reference's OUTPUTS are stored; no reference source text is copied.

Import shims: as in make_golden.py, plus two members of this file's own on the empty stand-in for the absent pyfftw --
`empty_aligned` (numpy.empty) and an `FFTW` callable backed by numpy.fft.rfft -- because correlate() runs its FFTs
through them.  correlate() is fed a duck-typed iterator (buff, nchunk, fsamp, __getitem__, samp_per_chunk) over 8-bit
voltages scaled as the GPU path scales them (u / 128 - 1).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import correlate_ref  # noqa: E402

NFFT, CHANMIN, NCHANOUT = 12500, 2155, 4096
CASES = (("b2", 41, (0, 58)), ("b3", 43, (0, 58, -61)))
NCHUNK = 8


class _FFTW(object):
    def __init__(self, a, b, **kw):
        pass

    def __call__(self, a, b):
        b[:] = np.fft.rfft(a)
        return b


class _Chunks(object):
    """beam k = pol 0 of antenna k of correlate_ref.delayed_antennas"""

    def __init__(self, u8):
        self.volts = (u8.astype(np.float32) / np.float32(128) - np.float32(1)).reshape(u8.shape[0], -1, NFFT)
        self.nchunk = self.volts.shape[1]
        self.fsamp = 128e6
        self.buff = np.empty((u8.shape[0], NFFT), np.float32)

    def __len__(self):
        return self.nchunk

    def __getitem__(self, idx):
        self.buff[:] = self.volts[:, idx]
        return self.buff

    def samp_per_chunk(self):
        return NFFT


def main():
    baseband, _, _ = make_golden.import_reference()
    pyfftw = sys.modules["pyfftw"]
    pyfftw.empty_aligned = lambda shape, dtype=None: np.empty(shape, dtype)
    pyfftw.FFTW = _FFTW
    out = {"nchunk": np.int64(NCHUNK)}
    for name, seed, delays in CASES:
        u8 = correlate_ref.delayed_antennas(seed, NCHUNK * NFFT, delays)[:, 0]
        cm = baseband.correlate(_Chunks(u8), nchunk=NCHUNK)
        band = np.ascontiguousarray(cm[:, :, CHANMIN:CHANMIN + NCHANOUT])
        d = baseband.get_delays(band.copy())
        m, model = baseband.fit_delays(d)
        iu = np.triu_indices(len(delays))
        out[name + "_seed"] = np.int64(seed)
        out[name + "_delays"] = np.array(delays, np.int64)
        out[name + "_cmatrix"] = band[iu].astype(np.complex64)        # [nbl][4096], i <= j row-major
        out[name + "_cmax"] = np.float64(np.abs(band).max())
        out[name + "_get_delays"] = d
        out[name + "_fit"] = m
        out[name + "_fit_model"] = model
    path = os.path.join(HERE, "reference_correlate.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), {k: v.tolist() for k, v in out.items() if k.endswith(("get_delays", "fit"))})


if __name__ == "__main__":
    main()
