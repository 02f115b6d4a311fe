"""The detection case that the periodicity search's CPU and GPU tests share: 64 channels, 4096 output samples, trial DMs 0,
20, 40, 60, 80, and a train of weak pulses of period 41.37 samples and width 2 dispersed at DM 40.  restated() gives what the
restatements alone (search_stats_ref, search_periodic_ref) make of it; it is computed once per process."""
import functools

import numpy as np

import search_periodic_ref as R
import search_stats_ref as S
import search_subband_ref as SB

TSAMP = 781.25e-6
NCHAN, TOUT, DMS = 64, 4096, (0.0, 20.0, 40.0, 60.0, 80.0)
FCH1, FOFF = 384.0, -1.0
PERIOD, WIDTH, AMP = 41.37, 2, 2.25           # samples, samples, codes per channel: 64 x 2.25 = 1.5 sigma of the series (8 x 12)
BINS = 32


@functools.lru_cache(maxsize=None)
def block(seed=0):
    """(codes [nsamp][nchan] u8, delay [ndm][nchan], nsamp): noise rint(N(96, 12)) plus the train at DM index 2"""
    delay = SB.delays(DMS, FCH1, FOFF, NCHAN, TSAMP)
    nsamp = TOUT + int(delay.max())
    g = np.random.default_rng(seed).normal(96.0, 12.0, (nsamp, NCHAN))
    n = 0
    while int(np.floor(n * PERIOD + 7.0)) + WIDTH <= TOUT:
        t0 = int(np.floor(n * PERIOD + 7.0))
        for c in range(NCHAN):
            g[t0 + delay[2, c]:t0 + delay[2, c] + WIDTH, c] += AMP
        n += 1
    x = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    x.setflags(write=False)
    return x, delay, nsamp


def series(x, delay):
    """the dedispersed series [ndm][TOUT] of a block, every channel unzapped"""
    t = np.arange(TOUT)
    return np.stack([sum(x[t + delay[d, c], c].astype(np.uint64) for c in range(NCHAN)) for d in range(len(DMS))])


@functools.lru_cache(maxsize=None)
def restated(seed=0):
    """dict(single: the largest single-pulse S/N over every DM and the boxcars 1 .. 64, best: the periodicity search's best
    tables per DM at BINS, octave 0, rms [ndm])"""
    x, delay, _ = block(seed)
    D = series(x, delay)
    single, best, rms = 0.0, [], []
    for d in range(len(DMS)):
        lvl, r, _ = S.series_stats(D[d], 0)
        single = max(single, float(S.boxcar_planes(D[d], lvl, r, 7, 0)[0].max()))
        rms.append(np.float32(r))
        best.append(R.search_series(D[d], np.float32(r), BINS, 0, 0))
    return dict(single=single, best=best, rms=np.array(rms, np.float32))
