"""The taps = 4 chain (k_channelize_pfb, k_pfb_weights, k_pfb_history, the two history slots and their ordering in
pb_process.hip) against tests/pfb_ref.py, an enumerated set of small cases, each chosen for one code path: every RFI mode,
one and two output pols, 8 / 4 / 2 bits; row counts with their own detect chunking and XCD row map; two antennas in
one handle; calls shorter than max_seg; reset_history / reset_bandpass of one antenna of two; a stream that starts
with no data and dropped frames in the carried rows; the injected pulse.  Every comparison is exact: the code bytes of
both streams, the weights pb_fetch reports and the final bandpass state as bit patterns."""
import functools

import numpy as np
import pytest

import pfb_ref
from helpers import NCHAN, libpb, make_input
from test_gpu_pfb import _run_many, _run_pipelined

pytestmark = pytest.mark.gpu
NFFT = 12500
CHANMIN = 2155


def _same_f32(got, ref):
    """bit patterns equal; NaNs (whose payload the two machines need not share) in the same places"""
    got, ref = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(ref, np.float32).ravel()
    if got.size != ref.size:
        return False
    ng, nr = np.isnan(got), np.isnan(ref)
    return np.array_equal(ng, nr) and np.array_equal(got.view(np.uint32)[~ng], ref.view(np.uint32)[~nr])


def _check(ref, rfi_mode, raw, kur, wts, bandpass, what=""):
    """one antenna's collected output against its reference, by test_gpu_fuzz.py's mode rules"""
    if rfi_mode != 1:
        assert raw.size == ref.codes_raw.size and np.array_equal(raw, ref.codes_raw), \
            "%s raw-stream codes: %d bytes differ" % (what, int((raw != ref.codes_raw).sum()))
    if rfi_mode != 0:
        assert np.array_equal(wts.view(np.uint32), ref.weights.view(np.uint32)), "%s window-energy weights differ" % what
        assert kur.size == ref.codes_kur.size and np.array_equal(kur, ref.codes_kur), \
            "%s excised-stream codes: %d bytes differ" % (what, int((kur != ref.codes_kur).sum()))
    if bandpass is not None:
        gr, gk = bandpass
        band = lambda bp: bp.reshape(2, NCHAN)[:, CHANMIN:]
        if rfi_mode != 1:
            assert _same_f32(gr, band(ref.bp_raw)), "%s raw bandpass state" % what
        if rfi_mode == 2:
            assert _same_f32(gk, band(ref.bp_kur)), "%s excised bandpass state" % what
        if rfi_mode == 1:
            assert _same_f32(gk, band(ref.bp_raw)), "%s bandpass state (mode 1)" % what


def _cat(x):
    return np.concatenate(x) if x and x[0] is not None else None


def _plant(data, seg, R, shift=0):
    """one flagged block in each of segment seg's last three rows (the square wave of
    test_pfb_three_sets_resident_input_history_ordering); shift moves the blocks, so that two antennas' carried
    flags differ"""
    for row, blk in ((R - 1, 7 + shift), (R - 2, 19 + shift), (R - 3, 3 + shift)):
        x = data[seg, 0, row * NFFT + blk * 500:row * NFFT + (blk + 1) * 500]
        x[:] = np.where((np.arange(500) // 5) % 2 == 0, 230, 26)


def _assert_planted(ref, R, last_segs):
    """the planted rows are flagged and weight the next segment's first three rows: strictly between 0 and 1"""
    for seg in last_segs:
        g = (seg + 1) * R
        assert ref.flags[g - 1].any() and ref.flags[g - 2].any() and ref.flags[g - 3].any(), seg
        first3 = ref.w[g:g + 3]
        assert ((first3 > 0) & (first3 < 1)).all(), (seg, first3)


# ---------------------------------------------------------------------------------------------------------
# a. formats

@functools.lru_cache(maxsize=None)
def _format_input():
    data = make_input(62, 16, 6)
    for p in range(2):                    # four wholly flagged rows (test_pfb_rfi_mode2_both_streams_bit_exact)
        seg = data[3, p, 4 * NFFT:8 * NFFT]
        seg[:] = np.where((np.arange(seg.size) // 5) % 2 == 0, 220, 36)
    data.setflags(write=False)
    return data


@pytest.mark.parametrize("nbit", [8, 4, 2])
@pytest.mark.parametrize("npol", [1, 2])
@pytest.mark.parametrize("rfi_mode", [0, 1, 2])
def test_formats(oracle, rfi_mode, npol, nbit):
    """Every RFI mode x output pols x bits, three batches of two segments through two buffer sets.  npol = 2 keeps the
    per-pol weights (no pscrunch_weights); the 2-bit, one-pol, mode-2 case is what process_baseband --taps 4 writes."""
    lp = libpb()
    R, S, NB = 16, 2, 3
    data = _format_input()
    ref = pfb_ref.pfb_chain(oracle, data, R, rfi_mode, npol, nbit)
    if rfi_mode:
        w = ref.w
        assert (w == 0).any() and ((w > 0) & (w < np.float32(0.2))).any() and ((w >= np.float32(0.2)) & (w < 1)).any()
    bp = []
    raw, kur, wts = _run_pipelined(lp, [data[k * S:(k + 1) * S] for k in range(NB)], R, rfi_mode, 2, nbit=nbit,
                                   npol=npol, bandpass=bp)
    _check(ref, rfi_mode, _cat(raw), _cat(kur), _cat(wts), bp[0])
    if rfi_mode == 2:
        assert (ref.codes_kur != ref.codes_raw).any()


# ---------------------------------------------------------------------------------------------------------
# b. shapes and antennas

@pytest.mark.parametrize("seed,Rr,S,nb,rfi_mode,nant,nbit", [
    (66, 8, 1, 9, 2, 1, 8),          # the three cases of test_pfb_buffer_set_counts_agree
    (66, 64, 2, 3, 1, 1, 8),
    (66, 24, 2, 3, 2, 2, 8),
    (67, 40, 1, 3, 2, 1, 2),         # odd R >> 3 in the channeliser's XCD row map
    (68, 72, 1, 3, 2, 1, 2)])
def test_shapes_and_antennas(oracle, seed, Rr, S, nb, rfi_mode, nant, nbit):
    """Row counts from one 8-row detect chunk to 72, RFI mode 1, two antennas in one handle (antenna a's stream is the
    data rolled by a segments; each antenna is held to the reference of its own stream: a wrong antenna stride in the
    history slots shows).  The last three rows of every batch but the last carry a flagged block each, in every
    antenna's stream and in other blocks for each antenna, so that the next batch's first three weights and excised
    rows depend on the carried flags of that very antenna."""
    lp = libpb()
    n = S * nb
    data = make_input(seed, Rr, n)
    streams = [[(i - a) % n for i in range(n)] for a in range(nant)]          # np.roll(data, a, axis=0), as indices
    last = [[k * S + S - 1 for k in range(nb - 1)] for a in range(nant)]       # stream positions of the planted rows
    for a in range(nant):
        for pos in last[a]:
            _plant(data, streams[a][pos], Rr, shift=2 * a)
    bp = []
    got = _run_many(lp, data, Rr, S, rfi_mode, nant, nsets=2, nbit=nbit, bandpass=bp)
    refs = [pfb_ref.pfb_chain(oracle, np.roll(data, a, axis=0), Rr, rfi_mode, 1, nbit) for a in range(nant)]
    for a in range(nant):
        _assert_planted(refs[a], Rr, last[a])
        for pos in last[a]:                        # no other antenna carries the same flags or gets the same weights
            g = (pos + 1) * Rr
            for o in range(a):
                assert (refs[a].flags[g - 3:g] != refs[o].flags[g - 3:g]).any(axis=1).all()
                assert (refs[a].w[g:g + 3] != refs[o].w[g:g + 3]).all()
        _check(refs[a], rfi_mode, got[a][0], got[a][1], got[a][2], bp[a], "antenna %d" % a)


# ---------------------------------------------------------------------------------------------------------
# c. uneven calls

@pytest.mark.parametrize("nsets", [1, 2])
def test_calls_shorter_than_max_seg(oracle, nsets):
    """max_seg = 3, calls of 3, 1 and 2 segments, each into slots 0 ..: the history kernel keeps the last three rows
    of the CALL (rows nseg * R - 3 ..), not of the buffer, whose later slots still hold an earlier call's segments."""
    lp = libpb()
    R, calls = 16, (3, 1, 2)
    data = make_input(70, R, sum(calls))
    ends = np.cumsum(calls)
    for e in ends:
        _plant(data, int(e) - 1, R)
    ref = pfb_ref.pfb_chain(oracle, data, R, 2, 1, 8)
    _assert_planted(ref, R, [int(e) - 1 for e in ends[:-1]])
    raw, kur, wts = [], [], []

    def collect(h, k):
        h.select_set(k % nsets)
        o = h.fetch(0, 0, calls[k], weights=True)
        raw.append(o["raw"]), kur.append(o["kur"]), wts.append(o["weights"])

    with lp.PbHandle(nbit=8, rfi_mode=2, taps=4, rows_per_seg=R, max_seg=3, nsets=nsets) as h:
        for k, n in enumerate(calls):
            h.select_set(k % nsets)
            s0 = int(ends[k]) - n
            for s in range(n):
                h.submit_planar(0, s, data[s0 + s, 0], data[s0 + s, 1])
            h.process(n)
            if k >= nsets - 1:
                collect(h, k - (nsets - 1))
        for k in range(max(0, len(calls) - (nsets - 1)), len(calls)):
            collect(h, k)
        bp = h.get_bandpass(0)
    _check(ref, 2, _cat(raw), _cat(kur), _cat(wts), bp)


# ---------------------------------------------------------------------------------------------------------
# d. reset

def _reset_case(oracle, nsets, rfi_mode, nant, reset_ant, after=2):
    """four batches of two segments; reset_history + reset_bandpass of reset_ant once `after` batches are queued"""
    lp = libpb()
    R, S, NB = 16, 2, 4
    n = S * NB
    cut = after * S                                # the first segment of the new observation
    data = make_input(71, R, n)
    for a in range(nant):                          # the last three rows before the reset, in every antenna's stream
        _plant(data, (cut - 1 - a) % n, R, shift=2 * a)

    def after_batch(h, k):
        if k == after - 1:
            h.reset_history(reset_ant)
            h.reset_bandpass(reset_ant)

    bp = []
    got = _run_many(lp, data, R, S, rfi_mode, nant, nsets=nsets, nbit=2, bandpass=bp, after_batch=after_batch)
    for a in range(nant):
        stream = np.roll(data, a, axis=0)
        ref = pfb_ref.pfb_chain(oracle, stream, R, rfi_mode, 1, 2, resets=(cut,) if a == reset_ant else ())
        whole = pfb_ref.pfb_chain(oracle, stream, R, rfi_mode, 1, 2) if a == reset_ant else ref
        _assert_planted(whole, R, [cut - 1])       # stale rows or flags would give `whole`'s weights and codes
        if a == reset_ant:
            g = cut * R
            assert not np.array_equal(ref.w[g:g + 3], whole.w[g:g + 3])
            assert not np.array_equal(ref.codes_kur, whole.codes_kur)
        _check(ref, rfi_mode, got[a][0], got[a][1], got[a][2], bp[a], "antenna %d" % a)


# pb_process flips the history slot it reads at every call, whatever the number of buffer sets: a reset after two
# batches is followed by a batch that reads slot 0, one after three batches by a batch that reads slot 1.
@pytest.mark.parametrize("after", [2, 3])
@pytest.mark.parametrize("nsets", [1, 2])
def test_reset_one_antenna_of_two(oracle, nsets, after):
    """reset_history(1) + reset_bandpass(1) between batches (RFI mode 2, 2-bit): antenna 0 goes on as one stream,
    antenna 1 restarts -- its first three rows see zero rows weighted as "everything flagged" in the history slot
    the next batch reads, not the planted flags of the rows before."""
    _reset_case(oracle, nsets, 2, 2, 1, after)


@pytest.mark.parametrize("after", [2, 3])
@pytest.mark.parametrize("nsets", [1, 2])
def test_reset_mode1(oracle, nsets, after):
    """the same with RFI mode 1 (one stream, normalised into the raw bandpass state) and one antenna"""
    _reset_case(oracle, nsets, 1, 1, 0, after)


# ---------------------------------------------------------------------------------------------------------
# e. no data

def _nodata_input(which):
    R = 16
    data = make_input(72, R, 6, dropped=False)
    if which == "first_segment":
        data[0] = 0                                # the stream starts with a segment of code 0
    else:
        a = (R - 2) * NFFT + 2500                  # a run of code 0 inside a row that the next batch carries
        data[1, 1, a:a + 5000] = 0
    return data


@pytest.mark.parametrize("nbit", [8, 2])
@pytest.mark.parametrize("rfi_mode", [0, 2])
@pytest.mark.parametrize("which", ["first_segment", "carried_row"])
def test_no_data(oracle, which, rfi_mode, nbit):
    """Code 0 is "no sample" = 0.0.  first_segment: every window of segment 0 is excised (weight 0, the +inf plane
    convention) and the bandpass initialises late; carried_row: the zero codes sit in a history row, which the
    channeliser patches itself (in mode 0 the input buffer is never patched, in mode 2 the kurtosis kernel has
    patched it -- the history kernel copies what it finds)."""
    lp = libpb()
    R, S, NB = 16, 2, 3
    data = _nodata_input(which)
    ref = pfb_ref.pfb_chain(oracle, data, R, rfi_mode, 1, nbit)
    if rfi_mode == 2 and which == "first_segment":
        # rows 16 - 18 see segment 1 through taps 1 - 3 only, which hold about 1e-6 of the window's energy
        first3 = ref.w[R:R + 3]
        assert (ref.w[:R] == 0).all() and ((first3 > 0) & (first3 < np.float32(0.2))).all(), ref.w[:R + 4]
    if rfi_mode == 2 and which == "carried_row":
        assert ref.flags[2 * R - 2, 5:15].all() and (ref.w[2 * R:2 * R + 3] < 1).any()
    bp = []
    raw, kur, wts = _run_pipelined(lp, [data[k * S:(k + 1) * S] for k in range(NB)], R, rfi_mode, 2, nbit=nbit,
                                   bandpass=bp)
    _check(ref, rfi_mode, _cat(raw), _cat(kur), _cat(wts), bp[0])


# ---------------------------------------------------------------------------------------------------------
# f. injection

@pytest.mark.parametrize("rfi_mode", [0, 2])
def test_injected_pulse(oracle, rfi_mode):
    """inject_frb with taps = 4: two calls of two segments, inject_now = 1 then 3 (the channeliser's own
    since = (inject_now - 1 + seg) * R); orc_segment's width and amplitude, DM 80."""
    lp = libpb()
    R, S = 16, 2
    data = make_input(73, R, 2 * S)
    delays = oracle.set_frb_delays(80.0, R)
    ref = pfb_ref.pfb_chain(oracle, data, R, rfi_mode, 1, 8, frb_delays=delays, inject_from=0)
    plain = pfb_ref.pfb_chain(oracle, data, R, rfi_mode, 1, 8)
    assert not np.array_equal(ref.codes_raw, plain.codes_raw)
    if rfi_mode == 2:
        assert not np.array_equal(ref.codes_kur, plain.codes_kur)
    raw, kur, wts = [], [], []
    with lp.PbHandle(nbit=8, rfi_mode=rfi_mode, taps=4, rows_per_seg=R, max_seg=S, nsets=2, inject_frb=True) as h:
        for k in range(2):
            h.select_set(k)
            for s in range(S):
                h.submit_planar(0, s, data[k * S + s, 0], data[k * S + s, 1])
            h.process(S, inject_now=1 + k * S)
        for k in range(2):
            h.select_set(k)
            o = h.fetch(0, 0, S, raw=True, kur=rfi_mode != 0, weights=rfi_mode != 0)
            raw.append(o["raw"]), kur.append(o["kur"]), wts.append(o["weights"])
        bp = h.get_bandpass(0)
    _check(ref, rfi_mode, _cat(raw), _cat(kur), _cat(wts), bp)
