"""k_detect2 on its 1-D grid in the dispatch order of d2_block_map.h (the excised stream's workgroups first): the whole
chain against the oracle (oracle.segment with taps = 1, tests/pfb_ref.py with taps = 4), bit for bit --
codes of both streams, weights, final bandpass state -- at the smallest shapes that select each shipped instantiation.

The 32-row template runs 64 rows per segment x 5 segments per call: 10 chunks per launch, so the 5-slot plane ring and the
8-entry ring of row weights and source words both wrap.  The 8-row template (rows per segment no multiple of 32) runs 24
rows x 5 segments: 15 chunks.  The stream is three such calls long, call c on buffer set c mod nsets, collected
nsets - 1 calls late; it holds rows without flags, rows with one flagged block (a fresh row of every group of four in
each call, so that with one buffer set the rows a call leaves out of the excised plane hold an earlier call's values), an
all-flagged row (+inf, weight 0) in most segments and an all-bad first segment (the excised bandpass starts at 1).  The
second antenna has its own noise and its flagged rows elsewhere.

The test without the gpu mark holds the streams to that description with the CPU oracle."""
import functools

import numpy as np
import pytest

import pfb_ref
from helpers import CHANMIN, NCHAN, NCHANOUT, NFFT, libpb, make_input

gpu = pytest.mark.gpu
NSEG, NCALL = 5, 3
FULL_W = np.float32(1.00000011920928955078125)


def _row(data, s, p, r):
    return data[s, p, r * NFFT:(r + 1) * NFFT]


@functools.lru_cache(maxsize=None)
def _stream(R, ant):
    """u8 [NCALL * NSEG][2][R x 12500]"""
    data = make_input(7100 + 10 * R + ant, R, NCALL * NSEG, rfi=False, dropped=False)
    n = np.arange(NFFT)
    for s in range(NCALL * NSEG):
        call = s // NSEG
        for q in range(R // 4):                     # one impulsive block in one row of every group of four
            x = _row(data, s, (q + s + ant) % 2, 4 * q + (1 + call + ant) % 4)
            blk = (7 * q + 3 * s + 11 * ant) % 25
            x[blk * 500:(blk + 1) * 500] = np.where((np.arange(500) // 5) % 2 == 0, 230, 26)
        if s % 2 == 1:                              # a row with every block flagged
            for p in range(2):
                _row(data, s, p, (3 * s + 2 * ant) % R)[:] = np.where((n // 5) % 2 == 0, 220, 36)
    for r in range(R):                              # the first segment entirely bad
        for p in range(2):
            _row(data, 0, p, r)[:] = np.where((n // 5) % 2 == 0, 220, 36)
    data.setflags(write=False)
    return data


def _band(bp):
    return bp.reshape(2, NCHAN)[:, CHANMIN:CHANMIN + NCHANOUT]


@functools.lru_cache(maxsize=None)
def _ref(oracle, taps, R, ant, nseg, rfi_mode, npol, nbit):
    """the first nseg segments of an antenna's stream -> (codes raw, codes excised, weights, band raw, band excised);
    None for what the mode does not have"""
    data = _stream(R, ant)[:nseg]
    if taps == 4:
        r = pfb_ref.pfb_chain(oracle, data, R, rfi_mode, npol, nbit)
        return r.codes_raw, r.codes_kur, r.weights, _band(r.bp_raw), _band(r.bp_kur)
    bp_raw, bp_kur = np.zeros(2 * NCHAN, np.float32), np.zeros(2 * NCHAN, np.float32)
    res = [oracle.segment(data[s], R, bp_raw, bp_kur, rfi_mode=rfi_mode, npol=npol, nbit=nbit) for s in range(nseg)]
    raw = np.concatenate([r.codes_raw for r in res]) if rfi_mode != 1 else None
    kur = np.concatenate([r.codes_kur for r in res]) if rfi_mode != 0 else None
    wts = np.concatenate([r.weights[:R] for r in res]) if rfi_mode != 0 else None
    return raw, kur, wts, _band(bp_raw), _band(bp_kur)


@pytest.mark.parametrize("ant", [0, 1])
@pytest.mark.parametrize("R", [64, 24])
def test_streams_are_what_they_claim(oracle, R, ant):
    data = _stream(R, ant)
    bp_raw, bp_kur = np.zeros(2 * NCHAN, np.float32), np.zeros(2 * NCHAN, np.float32)
    res = [oracle.segment(data[s], R, bp_raw, bp_kur, rfi_mode=2, npol=1, nbit=8) for s in range(NCALL * NSEG)]
    w = np.concatenate([r.weights[:R] for r in res]).reshape(-1, R)
    nflag = np.concatenate([(r.dag[:R * 25] > 3.0) for r in res]).reshape(-1, R, 25).sum(axis=2)
    in_raw = w.view(np.uint32) == FULL_W.view(np.uint32)
    assert np.array_equal(in_raw, nflag == 0)
    assert (nflag[0] == 25).all() and (w[0] == 0).all()                  # the all-bad first segment
    T = 32 if R % 32 == 0 else 8
    for s in range(1, NCALL * NSEG):
        assert in_raw[s].sum() >= R // 3 and (nflag[s] == 1).sum() >= R // 8, s
        c = in_raw[s].reshape(-1, T)
        assert (c.any(axis=1) & ~c.all(axis=1)).all(), s                 # every chunk mixes rows of both planes
        if s % 2 == 1:
            r = (3 * s + 2 * ant) % R
            assert nflag[s, r] == 25 and w[s, r] == 0
    for call in range(1, NCALL):                                         # other rows stay out of the excised plane
        a, b = in_raw[(call - 1) * NSEG + 1:call * NSEG], in_raw[call * NSEG + 1:(call + 1) * NSEG]
        assert (a & ~b).sum() >= R // 4 and (b & ~a).sum() >= R // 4


def _same_f32(got, ref):
    got, ref = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(ref, np.float32).ravel()
    return got.size == ref.size and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def _check(oracle, monkeypatch, taps, R, rfi_mode, npol, nbit, nant, nsets, ncall, depth):
    lp = libpb()
    monkeypatch.setenv("PB_DETECT_DEPTH", str(depth))
    got = [dict(raw=[], kur=[], wts=[]) for _ in range(nant)]

    def collect(h, call):
        h.select_set(call % nsets)
        for a in range(nant):
            o = h.fetch(a, 0, NSEG, raw=rfi_mode != 1, kur=rfi_mode != 0, weights=rfi_mode != 0)
            got[a]["raw"].append(o["raw"]), got[a]["kur"].append(o["kur"]), got[a]["wts"].append(o["weights"])

    with lp.PbHandle(nant=nant, nbit=nbit, npol=npol, rfi_mode=rfi_mode, taps=taps, rows_per_seg=R, max_seg=NSEG,
                     nsets=nsets) as h:
        for call in range(ncall):
            h.select_set(call % nsets)
            for a in range(nant):
                d = _stream(R, a)
                for s in range(NSEG):
                    h.submit_planar(a, s, d[call * NSEG + s, 0], d[call * NSEG + s, 1])
            h.process(NSEG)
            if call >= nsets - 1:
                collect(h, call - (nsets - 1))
        for call in range(max(0, ncall - (nsets - 1)), ncall):
            collect(h, call)
        bps = [h.get_bandpass(a) for a in range(nant)]
    for a in range(nant):
        raw, kur, wts, band_raw, band_kur = _ref(oracle, taps, R, a, ncall * NSEG, rfi_mode, npol, nbit)
        what = "antenna %d" % a
        if rfi_mode != 0:
            assert _same_f32(np.concatenate(got[a]["wts"]), wts), what + ": weights"
            g = np.concatenate(got[a]["kur"])
            assert np.array_equal(g, kur), what + ": excised-stream codes, %d bytes differ" % int((g != kur).sum())
        if rfi_mode != 1:
            g = np.concatenate(got[a]["raw"])
            assert np.array_equal(g, raw), what + ": raw-stream codes, %d bytes differ" % int((g != raw).sum())
            assert _same_f32(bps[a][0], band_raw), what + ": raw bandpass state"
        if rfi_mode == 2:
            assert _same_f32(bps[a][1], band_kur), what + ": excised bandpass state"
        elif rfi_mode == 1:          # mode 1 normalises its one stream into the raw state
            assert _same_f32(bps[a][1], band_raw), what + ": excised bandpass state"


@gpu
@pytest.mark.parametrize("nsets", [1, 2, 3])
@pytest.mark.parametrize("nant", [1, 2])
@pytest.mark.parametrize("rfi_mode", [0, 1, 2])
@pytest.mark.parametrize("taps", [1, 4])
def test_chain_antennas_modes_and_buffer_sets(oracle, monkeypatch, taps, rfi_mode, nant, nsets):
    """the 32-row template; two, three and the default number of chunks requested ahead, in turn with the buffer sets"""
    _check(oracle, monkeypatch, taps, 64, rfi_mode, 1, 8, nant, nsets, NCALL, (2, 3, 0)[nsets - 1])


@gpu
@pytest.mark.parametrize("npol,nbit", [(1, 8), (2, 8), (1, 4), (2, 4), (1, 2), (2, 2)])
@pytest.mark.parametrize("R,depth", [(64, 2), (64, 3), (24, 0)])
@pytest.mark.parametrize("taps,rfi_mode", [(1, 0), (1, 1), (1, 2), (4, 2)])
def test_every_instantiation(oracle, monkeypatch, taps, rfi_mode, R, depth, npol, nbit):
    """chunk length x ring depth x pols x bits x (mode, where the excised stream's rows come from): one call of 5 segments"""
    _check(oracle, monkeypatch, taps, R, rfi_mode, npol, nbit, 1, 1, 1, depth)
