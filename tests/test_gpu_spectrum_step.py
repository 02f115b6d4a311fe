"""The channelisers' spectrum step -- the real-input split, the injected pulse, |X|^2, the division by the row weight and
the two plane stores -- against the oracle, bit for bit, on rows chosen for the paths of that step: the division on the
bits and its one guard per four channels (a lane of a wave out of range, or none; all of them:
tests/test_spectrum_div4_cpu.py), the true division, the
rows that get a second transform and those that get none, with and without the injection code (the kernels without it
and their injecting twins), for the kernel that flags its own rows and the one that is told the flags, taps 1 and 4.
R = 8 rows per segment and 2 segments: the smallest shape with a row hand-over inside a workgroup and across a segment."""
import functools

import numpy as np
import pytest

import coherence_ref as CR
import pfb_ref
from helpers import NFFT, libpb, make_input, oracle_run

pytestmark = pytest.mark.gpu

R, NSEG = 8, 2
PULSE_DM = 17.7
ZERO_PATTERN = (192, 128, 64, 128, 192, 128, 128, 155, 128, 128)     # +a 0 -a 0 +a 0 0 +b 0 0: a = 0.5, b = 27 / 128


@functools.lru_cache(maxsize=None)
def _input():
    """u8 [2 segments][2 pols][8 rows x 12500], by row (both pols unless said otherwise):
         segment 0                                         segment 1
      0  noise                                             two codes 96 / 160
      1  noise + one impulsive 500-sample block (pol 0)    code 0 throughout (pol 0; pol 1 noise)
      2  code 0 throughout: every power exactly 0          every block flagged
      3  two codes 96 / 160: one loud channel (6250)       noise
         beside zeros and tiny values
      4  every block flagged (weight 0)                    codes 1 / 255
      5  codes 1 / 255: the largest powers                 noise + one impulsive block (pol 1)
      6  the ten-sample pattern ZERO_PATTERN               code 0 throughout
      7  noise + one impulsive block (pol 1)               ZERO_PATTERN (pol 1; pol 0 noise)
    The statistic flags the rows of one, two or three codes whole (their kurtosis is NaN or 1), so in RFI modes 1 and 2
    their powers -- zeros, tiny values, the largest ones -- reach the raw plane only.  ZERO_PATTERN is the row that
    takes zeros through the division on the bits: a sequence of period 10 whose kurtosis is 3.002, which no block is
    flagged for, and whose spectrum is four lines among powers of 1e-7 and less, one of them (test below) exactly 0
    beside non-zero neighbours of its group of four -- lanes of one wave on either side of the guard."""
    data = make_input(91, R, NSEG, rfi=False, dropped=False)
    n = np.arange(NFFT)

    def row(s, p, r):
        return data[s, p, r * NFFT:(r + 1) * NFFT]

    def impulse(s, p, r, blk):
        x = row(s, p, r)[blk * 500:(blk + 1) * 500]
        x[:] = np.where((np.arange(500) // 5) % 2 == 0, 230, 26)

    impulse(0, 0, 1, 7)
    impulse(0, 1, 7, 19)
    impulse(1, 1, 5, 3)
    for p in range(2):
        row(0, p, 2)[:] = 0
        row(1, p, 6)[:] = 0
        row(0, p, 3)[:] = np.where(n % 2 == 0, 96, 160)
        row(1, p, 0)[:] = np.where(n % 2 == 0, 96, 160)
        row(0, p, 4)[:] = np.where((n // 5) % 2 == 0, 220, 36)
        row(1, p, 2)[:] = np.where((n // 5) % 2 == 0, 220, 36)
        row(0, p, 5)[:] = np.where(n % 2 == 0, 1, 255)
        row(1, p, 4)[:] = np.where(n % 2 == 0, 1, 255)
    row(1, 0, 1)[:] = 0
    for s, p, r in ((0, 0, 6), (0, 1, 6), (1, 1, 7)):
        row(s, p, r)[:] = np.asarray(ZERO_PATTERN, np.uint8)[n % 10]
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def _delays(oracle):
    """the pulse's delays at PULSE_DM: rows 5.0 (top of the band) to 17.5, so that the window (the row of the delay,
    at times the next one too) lies inside the 16 rows for most channels and beyond them for the lowest ones"""
    return oracle.set_frb_delays(PULSE_DM, R)


@functools.lru_cache(maxsize=None)
def _reference(oracle, taps, rfi_mode, inject):
    """-> (raw codes, excised codes, weights as pb_fetch reports them, flags [rows x 25] u8)"""
    data = _input()
    delays = _delays(oracle) if inject else None
    if taps == 4:
        ref = pfb_ref.pfb_chain(oracle, data, R, rfi_mode, 1, 8, frb_delays=delays, inject_from=0 if inject else None)
        return ref.codes_raw, ref.codes_kur, ref.weights, ref.flags.astype(np.uint8).ravel()
    res, _, _ = oracle_run(oracle, data, R, rfi_mode=rfi_mode, npol=1, nbit=8, frb_delays=delays,
                           inject_now=1 if inject else 0)
    flags = np.concatenate([(r.dag[:R * 25] > 3.0).astype(np.uint8) for r in res])
    return (np.concatenate([r.codes_raw for r in res]), np.concatenate([r.codes_kur for r in res]),
            np.concatenate([r.weights[:R] for r in res]), flags)


def test_the_input_reaches_every_path(oracle):
    """the rows are what the docstring of _input says they are to the flagger, and the pulse's window covers some rows
    of some channels only"""
    _, _, w, flags = _reference(oracle, 1, 2, False)
    f = flags.reshape(NSEG * R, 25)
    full = np.float32(1.00000011920928955078125)
    for r in (0, 6, 11, 15):                               # unflagged: the division on the bits
        assert not f[r].any() and w[r] == full, (r, w[r])
    for r in (1, 7, 13):                                   # one flagged block: a second transform, the true division
        assert f[r].sum() == 1 and 0 < w[r] < 1, (r, w[r])
    for r in (2, 3, 4, 5, 8, 9, 10, 12, 14):               # every block flagged: no second transform, +inf plane
        assert f[r].all() and w[r] == 0, (r, w[r])
    # the unflagged row 6 has a channel of power exactly 0 whose group of four holds non-zero powers too
    volts = oracle.convertarray(np.array(_input()[0, 0, 6 * NFFT:7 * NFFT]))
    X = np.asarray(oracle.rfft(volts)).view(np.float32).reshape(-1, 2)
    p = (X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1])[2155:2155 + 4096].reshape(1024, 4)
    mixed = (p == 0).any(axis=1) & (p != 0).any(axis=1)
    assert mixed.any() and p.max() > 1e6 and ((p > 0) & (p < 1e-7)).sum() > 2048
    raw0, kur0, _, _ = _reference(oracle, 1, 2, False)
    raw1, kur1, _, _ = _reference(oracle, 1, 2, True)
    for a, b in ((raw0, raw1), (kur0, kur1)):
        changed = (a != b).reshape(NSEG * R // 8, 4096)
        assert changed.any() and not changed.all(axis=1).any() and (~changed).any(axis=0).sum() > 1024


@pytest.mark.parametrize("taps", [1, 4])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("inject", [False, True])
@pytest.mark.parametrize("rfi_mode", [0, 1, 2])
def test_codes_flags_and_weights_equal_the_oracle(oracle, monkeypatch, rfi_mode, inject, fuse, taps):
    lp = libpb()
    monkeypatch.setenv("PB_FUSE_KURTOSIS", str(fuse))
    data = _input()
    raw, kur, w, flags = _reference(oracle, taps, rfi_mode, inject)
    with lp.PbHandle(nbit=8, npol=1, rfi_mode=rfi_mode, taps=taps, rows_per_seg=R, max_seg=NSEG, inject_frb=inject) as h:
        if inject:
            h.set_frb_params(dm=PULSE_DM)
        for s in range(NSEG):
            h.submit_planar(0, s, data[s, 0], data[s, 1])
        h.process(NSEG, inject_now=1 if inject else 0)
        out = h.fetch(0, 0, NSEG, raw=rfi_mode != 1, kur=rfi_mode != 0, weights=rfi_mode != 0)
        got_flags = np.concatenate([h.debug_fetch(lp.DBG_FLAGS, 0, s) for s in range(NSEG)]) if rfi_mode else None
    if rfi_mode != 1:
        assert np.array_equal(out["raw"], raw), "raw-stream codes: %d bytes differ" % int((out["raw"] != raw).sum())
    if rfi_mode != 0:
        assert np.array_equal(got_flags, flags), "flags differ"
        assert np.array_equal(out["weights"].view(np.uint32), np.asarray(w, np.float32).view(np.uint32)), "weights differ"
        assert np.array_equal(out["kur"], kur), "excised-stream codes: %d bytes differ" % int((out["kur"] != kur).sum())


def test_coherence_output_is_unchanged(oracle):
    """the coherence twins share the spectrum step's code: RFI mode 2 with the pulse, both streams' AA, BB, CR, CI"""
    lp = libpb()
    data = _input()
    ref = CR.run(oracle, data, R, 2, 8, _delays(oracle), 1)
    with lp.PbHandle(nbit=8, npol=2, rfi_mode=2, rows_per_seg=R, max_seg=NSEG, inject_frb=True, coherence=True) as h:
        for s in range(NSEG):
            h.submit_planar(0, s, data[s, 0], data[s, 1])
        h.set_frb_params(dm=PULSE_DM)
        h.process(NSEG, inject_now=1)
        out = h.fetch(0, 0, NSEG)
    assert np.array_equal(out["raw"], ref[0][0]) and np.array_equal(out["kur"], ref[1][0])
