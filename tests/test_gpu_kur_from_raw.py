"""RFI mode 2: the excised plane holds only the rows that have flags; detect's excised stream takes every other row from
the RAW plane (k_detect2.hip, CONV) -- as it is with taps = 4, divided by 1 + 2^-23 in LDS with taps = 1.  Codes of both
streams, the weights and the final bandpass state against oracle.segment (taps 1) and tests/pfb_ref.py (taps 4), bit for
bit, on streams built so that

  * every chunk of detect's ring, and most groups of four rows (one LDS-DMA instruction), mix rows of both planes;
  * the stream is processed in TWO calls on the same buffer set, with the flagged rows elsewhere in the second call, so
    that the rows the second call leaves out of the excised plane hold the first call's values;
  * the rows that take a path of their own are there: every block flagged (+inf in the excised plane), a row of code 0
    (which the statistic flags whole), zero powers on a row WITHOUT flags (the conversion's division path), a channel
    eleven times above the bandpass on a row without flags (the excised stream's clip), a first segment that is
    entirely bad (the bandpass starts at 1), and with taps = 4 a window whose only flag sits in the faintest block of the
    window: its weight rounds to 1.0f although its excised spectrum differs from the raw one.

The tests without the gpu mark hold the inputs to those descriptions with the CPU oracle."""
import functools

import numpy as np
import pytest

import pfb_ref
from helpers import CHANMIN, NCHAN, NCHANOUT, NFFT, libpb, make_input

gpu = pytest.mark.gpu
NSEG = 2                       # segments per call; the stream is two calls long
FULL_W = np.float32(1.00000011920928955078125)
ZERO_PATTERN = (192, 128, 64, 128, 192, 128, 128, 155, 128, 128)     # tests/test_gpu_spectrum_step.py: kurtosis 3.002
TONE_BIN, TONE_AMP = 3000, 4.0                                       # 0.24 sigma: ~180 x the noise in one channel
SHAPES = (8, 24, 32, 64)
SEED1 = {8: 416, 24: 424, 32: 432, 64: 464}        # noise on which no special row collects a flag by chance
FAINT = {8: 13, 24: 13, 32: 13, 64: 5}             # taps 4: a row (8 q + 5) whose neighbours the statistic leaves alone


def _chunk(R):
    return 32 if R % 32 == 0 else 8


def _row(data, s, p, r):
    return data[s, p, r * NFFT:(r + 1) * NFFT]


def _impulse(data, s, p, r, blk):
    x = _row(data, s, p, r)[blk * 500:(blk + 1) * 500]
    x[:] = np.where((np.arange(500) // 5) % 2 == 0, 230, 26)


def _all_flagged(data, s, r):
    n = np.arange(NFFT)
    for p in range(2):
        _row(data, s, p, r)[:] = np.where((n // 5) % 2 == 0, 220, 36)


def _tone(data, s, r):
    n = np.arange(NFFT)
    for p in range(2):
        x = _row(data, s, p, r).astype(np.float64) + TONE_AMP * np.sin(2 * np.pi * TONE_BIN * n / NFFT)
        _row(data, s, p, r)[:] = np.clip(np.rint(x), 1, 255)


@functools.lru_cache(maxsize=None)
def _stream1(R, bad_first):
    """taps 1.  u8 [4 segments][2][R x 12500] and the rows with a path of their own {name: (segment, row)}.  One
    impulsive block in row 4 q + 1 of every group of four (4 q + 2 in the second call); segment 1 and segment 2 (the
    second call's first) carry the special rows, at different places."""
    data = make_input(SEED1[R], R, 2 * NSEG, rfi=False, dropped=False)
    for s in range(2 * NSEG):
        for q in range(R // 4):
            _impulse(data, s, (q + s) % 2, 4 * q + (1 if s < NSEG else 2), (7 * q + 3 * s) % 25)
    special = {}
    for s, (zero, bad, tone, code0) in ((1, (0, 3, 4, 7)), (2, (3, 4, 7, 0))):
        for p in range(2):
            _row(data, s, p, zero)[:] = np.asarray(ZERO_PATTERN, np.uint8)[np.arange(NFFT) % 10]
            _row(data, s, p, code0)[:] = 0
        _all_flagged(data, s, bad)
        _tone(data, s, tone)
        special[s] = dict(zero=zero, bad=bad, tone=tone, code0=code0)
    if bad_first:
        for r in range(R):
            _all_flagged(data, 0, r)
    data.setflags(write=False)
    return data, special


@functools.lru_cache(maxsize=None)
def _stream4(R):
    """taps 4.  A window is unflagged only when four consecutive rows are: one impulsive block every EIGHT rows of the
    stream (row 8 q + 1; 8 q + 2 in the second call), so that the windows 8 q + 1 .. 8 q + 4 have a flag and the next four
    have none unless the statistic flags a block of the noise itself.  Row FAINT[R]: block 0 alone -- the faintest block
    of the window two rows on.  One row with every block flagged."""
    data = make_input(451 + R, R, 2 * NSEG, rfi=False, dropped=False)
    rows = 2 * NSEG * R
    for g in range(rows):
        if g % 8 == (1 if g < NSEG * R else 2):
            _impulse(data, g // R, (g // 8) % 2, g % R, (5 * (g // 8) + 2) % 25)
    _impulse(data, FAINT[R] // R, 0, FAINT[R] % R, 0)
    g = NSEG * R + 11
    _all_flagged(data, g // R, g % R)
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def _ref1(oracle, R, bad_first, rfi_mode, npol, nbit):
    """-> per-segment oracle results and the bandpass state (raw, excised) BEFORE every segment and after the last"""
    data, _ = _stream1(R, bad_first)
    bp_raw, bp_kur = np.zeros(2 * NCHAN, np.float32), np.zeros(2 * NCHAN, np.float32)
    res, states = [], []
    for s in range(data.shape[0]):
        states.append((bp_raw.copy(), bp_kur.copy()))
        res.append(oracle.segment(data[s], R, bp_raw, bp_kur, rfi_mode=rfi_mode, npol=npol, nbit=nbit))
    states.append((bp_raw.copy(), bp_kur.copy()))
    return res, states


@functools.lru_cache(maxsize=None)
def _ref4(oracle, R, npol, nbit):
    return pfb_ref.pfb_chain(oracle, _stream4(R), R, 2, npol, nbit, keep_spectra=True)


def _mixing(in_raw, T):
    """in_raw: bool per row of the stream (its excised power comes from the raw plane).  -> (every chunk of T rows has
    rows of both planes, the share of groups of four rows that have)"""
    c = in_raw.reshape(-1, T)
    g = in_raw.reshape(-1, 4)
    return bool((c.any(axis=1) & ~c.all(axis=1)).all()), float((g.any(axis=1) & ~g.all(axis=1)).mean())


def _power(oracle, data, s, p, r):
    X = np.asarray(oracle.rfft(oracle.convertarray(np.array(_row(data, s, p, r))))).view(np.float32).reshape(-1, 2)
    return (X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1])[CHANMIN:CHANMIN + NCHANOUT]


@pytest.mark.parametrize("R", SHAPES)
def test_taps1_stream_is_what_it_claims(oracle, R):
    data, special = _stream1(R, False)
    res, states = _ref1(oracle, R, False, 2, 1, 8)
    w = np.concatenate([r.weights[:R] for r in res])
    flags = np.concatenate([(r.dag[:R * 25] > 3.0) for r in res]).reshape(-1, 25)
    in_raw = w.view(np.uint32) == FULL_W.view(np.uint32)
    assert np.array_equal(in_raw, ~flags.any(axis=1))        # the full weight <=> no flag: detect's test is the channeliser's
    every_chunk, groups = _mixing(in_raw, _chunk(R))
    assert every_chunk and groups >= 0.75, (every_chunk, groups)
    # the second call leaves other rows out of the excised plane than the first wrote
    first, second = in_raw[:NSEG * R], in_raw[NSEG * R:]
    assert (second & ~first).sum() >= R // 4 and (first & ~second).sum() >= R // 4
    for s, sp in special.items():
        g = s * R
        assert flags[g + sp["bad"]].all() and w[g + sp["bad"]] == 0
        assert flags[g + sp["code0"]].all() and w[g + sp["code0"]] == 0      # a dropped row is flagged whole: +inf too
        for p in range(2):
            assert (_power(oracle, data, s, p, sp["code0"]) == 0).all()
        # zeros on a row without flags, in groups of four channels with non-zero powers too: the division path
        assert in_raw[g + sp["zero"]]
        pz = _power(oracle, data, s, 0, sp["zero"]).reshape(-1, 4)
        assert ((pz == 0).any(axis=1) & (pz != 0).any(axis=1)).any()
        # the tone: a row without flags whose channel exceeds eleven times the excised bandpass before AND after the
        # segment (the state moves by less than a thousandth per row)
        assert in_raw[g + sp["tone"]]
        for p in range(2):
            pt = _power(oracle, data, s, p, sp["tone"])[TONE_BIN - CHANMIN] / FULL_W
            for st in (states[s], states[s + 1]):
                assert pt > 16.5 * st[1].reshape(2, NCHAN)[p, TONE_BIN], (s, p, pt)
    # the entirely bad first segment: the bandpass starts at 1 and the raw stream's does not
    res_b, states_b = _ref1(oracle, R, True, 2, 1, 8)
    assert (res_b[0].weights[:R] == 0).all()
    band = states_b[1][1].reshape(2, NCHAN)[:, CHANMIN:CHANMIN + NCHANOUT]
    assert (band == 1).all() and (states_b[1][0] != 1).any()


@pytest.mark.parametrize("R", SHAPES)
def test_taps4_stream_is_what_it_claims(oracle, R):
    ref = _ref4(oracle, R, 1, 8)
    # a complete window without flags (the stream's first three windows reach before its start)
    clean = np.array([g >= 3 and not ref.flags[g - 3:g + 1].any() for g in range(ref.w.size)])
    assert (ref.w[clean] == 1).all() and clean.sum() >= ref.w.size // 8
    T = _chunk(R)
    chunks = clean.reshape(-1, T)
    assert (chunks.any(axis=1) & ~chunks.all(axis=1)).mean() >= (1.0 if T == 32 else 0.5)
    assert _mixing(clean, T)[1] >= 0.3
    assert ((clean[NSEG * R:] != clean[:NSEG * R])).sum() >= R // 8       # the second call's clean windows lie elsewhere
    # its only flag is block 0 of tap 1: the weight cannot tell the window from a clean one
    f = FAINT[R]
    assert ref.flags[f, 0] and ref.flags[f - 1:f + 3].sum() == 1 and ref.w[f + 2] == 1 and not clean[f + 2]
    assert (ref.spec_raw[0, f + 2] != ref.spec_kur[0, f + 2]).any()
    g = NSEG * R + 11
    # (the window's energy sits in its last tap: only the window that ends three rows on loses its weight)
    assert ref.flags[g].all() and not clean[g:g + 4].any() and 0 < ref.w[g + 3] < np.float32(0.2)


def _run_two_calls(lp, data, R, rfi_mode, npol, nbit, taps):
    """the stream in two calls of NSEG segments on ONE buffer set -> (raw, kur, weights, (bp raw, bp kur))"""
    raw, kur, wts = [], [], []
    with lp.PbHandle(nbit=nbit, npol=npol, rfi_mode=rfi_mode, taps=taps, rows_per_seg=R, max_seg=NSEG, nsets=1) as h:
        for call in range(2):
            for s in range(NSEG):
                h.submit_planar(0, s, data[call * NSEG + s, 0], data[call * NSEG + s, 1])
            h.process(NSEG)
            o = h.fetch(0, 0, NSEG, raw=rfi_mode != 1, kur=True, weights=True)
            raw.append(o["raw"]), kur.append(o["kur"]), wts.append(o["weights"])
        bp = h.get_bandpass(0)
    return (np.concatenate(raw) if rfi_mode != 1 else None), np.concatenate(kur), np.concatenate(wts), bp


def _same_f32(got, ref):
    got, ref = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(ref, np.float32).ravel()
    return got.size == ref.size and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def _band(bp):
    return bp.reshape(2, NCHAN)[:, CHANMIN:CHANMIN + NCHANOUT]


def _check1(oracle, monkeypatch, R, depth, fuse, rfi_mode, npol, nbit, bad_first):
    lp = libpb()
    monkeypatch.setenv("PB_FUSE_KURTOSIS", str(fuse))
    monkeypatch.setenv("PB_DETECT_DEPTH", str(depth))
    data, _ = _stream1(R, bad_first)
    res, states = _ref1(oracle, R, bad_first, rfi_mode, npol, nbit)
    raw, kur, wts, bp = _run_two_calls(lp, data, R, rfi_mode, npol, nbit, 1)
    assert _same_f32(wts, np.concatenate([r.weights[:R] for r in res])), "weights differ"
    if rfi_mode == 2:
        ref_raw = np.concatenate([r.codes_raw for r in res])
        assert np.array_equal(raw, ref_raw), "raw-stream codes: %d bytes differ" % int((raw != ref_raw).sum())
        assert _same_f32(bp[0], _band(states[-1][0])), "raw bandpass state"
    ref_kur = np.concatenate([r.codes_kur for r in res])
    assert np.array_equal(kur, ref_kur), "excised-stream codes: %d bytes differ" % int((kur != ref_kur).sum())
    # (mode 1 normalises its one stream into the raw state: tests/test_gpu_pfb_matrix.py)
    assert _same_f32(bp[1], _band(states[-1][1 if rfi_mode == 2 else 0])), "excised bandpass state"


@gpu
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("R,depth", [(32, 2), (32, 3), (64, 2), (64, 3), (8, 0), (24, 0)])
def test_taps1_shapes_and_channelisers(oracle, monkeypatch, R, depth, fuse):
    """detect's chunks of 32 rows with two and three chunks requested ahead, its chunks of 8 rows; the channeliser that
    flags its own rows and the kurtosis kernel + channeliser pair"""
    _check1(oracle, monkeypatch, R, depth, fuse, 2, 1, 8, False)


@gpu
@pytest.mark.parametrize("npol,nbit", [(2, 8), (1, 2), (2, 2)])
@pytest.mark.parametrize("R,depth", [(32, 3), (8, 0)])
def test_taps1_formats(oracle, monkeypatch, R, depth, npol, nbit):
    _check1(oracle, monkeypatch, R, depth, 1, 2, npol, nbit, False)


@gpu
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("R", [32, 8])
def test_taps1_mode1_keeps_the_whole_excised_plane(oracle, monkeypatch, R, fuse):
    """RFI mode 1 has no raw plane to take rows from"""
    _check1(oracle, monkeypatch, R, 0, fuse, 1, 1, 8, False)


@gpu
@pytest.mark.parametrize("R,depth", [(32, 3), (32, 2), (8, 0)])
def test_taps1_first_segment_entirely_bad(oracle, monkeypatch, R, depth):
    _check1(oracle, monkeypatch, R, depth, 1, 2, 1, 8, True)


@gpu
@pytest.mark.parametrize("R,depth,npol,nbit", [(32, 2, 1, 8), (32, 3, 1, 8), (64, 0, 2, 2), (8, 0, 1, 2), (24, 0, 2, 8)])
def test_taps4_carried_history(oracle, monkeypatch, R, depth, npol, nbit):
    """the second call's first three windows reach into the first call's rows (and their flags)"""
    lp = libpb()
    monkeypatch.setenv("PB_DETECT_DEPTH", str(depth))
    ref = _ref4(oracle, R, npol, nbit)
    raw, kur, wts, bp = _run_two_calls(lp, _stream4(R), R, 2, npol, nbit, 4)
    assert _same_f32(wts, ref.weights), "window-energy weights differ"
    assert np.array_equal(raw, ref.codes_raw), "raw-stream codes: %d bytes differ" % int((raw != ref.codes_raw).sum())
    assert np.array_equal(kur, ref.codes_kur), "excised-stream codes: %d bytes differ" % int((kur != ref.codes_kur).sum())
    assert _same_f32(bp[0], _band(ref.bp_raw)) and _same_f32(bp[1], _band(ref.bp_kur)), "bandpass state"


@gpu
def test_taps4_mode1_is_unchanged(oracle):
    lp = libpb()
    R = 32
    ref = pfb_ref.pfb_chain(oracle, _stream4(R), R, 1, 1, 8)
    _, kur, wts, bp = _run_two_calls(lp, _stream4(R), R, 1, 1, 8, 4)
    assert _same_f32(wts, ref.weights) and np.array_equal(kur, ref.codes_kur)
    assert _same_f32(bp[1], _band(ref.bp_raw))
