"""Every instantiation of k_detect_coh<T, NBIT, MODE> (T = 32 when rows_per_seg % 32 == 0, else 8; 8 / 4 / 2 bits; RFI
mode 0 / 1 / 2) once, deterministically, against tests/coherence_ref.py: the four fp32 planes, the codes and the
bandpass state that the handle is left with, all exactly.  Three segments go through in two calls, two segments then
one, so that the second call is shorter than max_seg (the strides use the handle's S, the chunk count the call's nseg)
and continues from the first call's bandpass.  Rows per segment 40 and 64 add more than one chunk per segment to the
shuffled 4- and 2-bit packing; a reset of one antenna of two closes the file."""
import functools

import numpy as np
import pytest

import coherence_ref as CR
from coherence_cases import PRODUCTS, f32_diff, streams
from helpers import libpb, make_input, oracle_run

pytestmark = pytest.mark.gpu

NCO = 4096
NFFT = 12500
NAMES = {0: "raw", 1: "excised"}


def run_calls(lp, datas, R, rfi_mode, nbit, calls, max_seg, nsets=1, lag=0, keep_ave=True, inject=False, after_call=None):
    """datas: per antenna u8 [sum(calls)][2][R * 12500], submitted to one coherence handle in calls of calls[k] segments
    into buffer set k % nsets; call k is collected once call k + lag is queued (lag < nsets).  after_call(h, k) runs
    once call k is queued (and, with a lag, call k - lag collected).
    -> per antenna {stream: (codes, planes [segments][4][R/8][4096] or None)}, per antenna get_bandpass"""
    assert lag < nsets and max(calls) <= max_seg
    nant = len(datas)
    first = np.concatenate([[0], np.cumsum(calls)]).astype(int)
    got = [{st: ([], []) for st in (0, 1)} for _ in range(nant)]

    def collect(h, k):
        h.select_set(k % nsets)
        for a in range(nant):
            o = h.fetch(a, 0, calls[k], ave=keep_ave)
            for st, nm in ((0, "raw"), (1, "kur")):
                got[a][st][0].append(np.array(o[nm], copy=True))
                if keep_ave:
                    got[a][st][1].append(np.array(o["ave_" + nm], copy=True).reshape(calls[k], 4, R // 8, NCO))

    with lp.PbHandle(nant=nant, nbit=nbit, npol=2, rfi_mode=rfi_mode, rows_per_seg=R, max_seg=max_seg, nsets=nsets,
                     keep_ave=keep_ave, inject_frb=inject, coherence=True) as h:
        for k, n in enumerate(calls):
            h.select_set(k % nsets)
            for a in range(nant):
                for s in range(n):
                    h.submit_planar(a, s, datas[a][first[k] + s, 0], datas[a][first[k] + s, 1])
            h.process(n, inject_now=(1 + int(first[k])) if inject else 0)
            if k >= lag:
                collect(h, k - lag)
            if after_call is not None:
                after_call(h, k)
        for k in range(max(0, len(calls) - lag), len(calls)):
            collect(h, k)
        bps = [h.get_bandpass(a) for a in range(nant)]
    out = [{st: (np.concatenate(c), np.concatenate(p) if keep_ave else None) for st, (c, p) in g.items()} for g in got]
    return out, bps


def check(got, bandpass, ref_codes, ref_planes, ref_bp, rfi_mode, what, exact_nan=False):
    """one antenna against its reference, for every stream the mode runs: codes, planes (when kept) and bandpass.
    ref_codes / ref_planes / ref_bp: {stream: array}.  The handle keeps the excised stream's bandpass in the second
    array of pb_get_bandpass in RFI mode 1 as in mode 2 (k_detect_coh indexes the state by stream).  exact_nan: the
    floats must be the same bit patterns throughout (a reference without NaN)"""
    for st in streams(rfi_mode):
        codes, planes = got[st]
        where = "%s, %s stream" % (what, NAMES[st])
        if planes is not None:
            for k, pr in enumerate(PRODUCTS):
                g, r = planes[:, k], ref_planes[st][:, k]
                assert g.shape == r.shape, (where, pr, g.shape, r.shape)
                if exact_nan:
                    nd = int((np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(r).view(np.uint32)).sum())
                else:
                    nd = f32_diff(g, r)
                assert nd == 0, "%s, %s plane: %d of %d values differ" % (where, pr, nd, r.size)
        rc = ref_codes[st]
        assert codes.size == rc.size, (where, codes.size, rc.size)
        nt = ref_planes[st].shape[0] * ref_planes[st].shape[2]
        gc, rcv = codes.reshape(nt, 4, -1), rc.reshape(nt, 4, -1)
        for k, pr in enumerate(PRODUCTS):
            nd = int((gc[:, k] != rcv[:, k]).sum())
            assert nd == 0, "%s, %s codes: %d of %d bytes differ" % (where, pr, nd, rcv[:, k].size)
        gb = bandpass[st]
        if exact_nan:
            nd = int((np.ascontiguousarray(gb, np.float32).view(np.uint32) != ref_bp[st].view(np.uint32)).sum())
        else:
            nd = f32_diff(gb, ref_bp[st])
        assert nd == 0, "%s bandpass state: %d of %d values differ" % (where, nd, ref_bp[st].size)


@functools.lru_cache(maxsize=None)
def _input(R):
    data = make_input(61 + R, R, 3)
    data.setflags(write=False)
    return data


def _matrix_case(oracle, R, nbit, rfi_mode):
    lp = libpb()
    data = _input(R)
    ref = CR.run(oracle, data, R, rfi_mode, nbit)
    for st in streams(rfi_mode):
        assert not np.isnan(ref[st][1]).any() and not np.isnan(ref.state.bp[st]).any()
    got, bps = run_calls(lp, [data], R, rfi_mode, nbit, calls=(2, 1), max_seg=2)
    check(got[0], bps[0], {st: ref[st][0] for st in ref}, {st: ref[st][1] for st in ref}, ref.state.bp, rfi_mode,
          "R %d, %d bit, mode %d" % (R, nbit, rfi_mode), exact_nan=True)


@pytest.mark.parametrize("rfi_mode", [0, 1, 2])
@pytest.mark.parametrize("nbit", [8, 4, 2])
@pytest.mark.parametrize("R", [8, 32])
def test_every_instantiation(oracle, R, nbit, rfi_mode):
    """R = 8: T = 8, one chunk per segment, three quarters of phase B's lanes repeat the last group for the shuffles;
    R = 32: T = 32, four groups, the bandpass before groups 1 .. 3 read from the previous group's entry"""
    _matrix_case(oracle, R, nbit, rfi_mode)


@pytest.mark.parametrize("nbit", [4, 2])
@pytest.mark.parametrize("R", [40, 64])
def test_more_chunks_per_segment(oracle, R, nbit):
    """R = 40: T = 8, five chunks per segment, so a segment starts on either half of the LDS double buffer;
    R = 64: T = 32, two chunks per segment"""
    _matrix_case(oracle, R, nbit, 2)


def _thin_group_input(R):
    """two segments; in the second, seven of the eight rows of the last 8-row group are a square wave in both pols"""
    data = make_input(91 + R, R, 2, rfi=False, dropped=False)
    for p in range(2):
        seg = data[1, p, (R - 8) * NFFT:(R - 1) * NFFT]
        seg[:] = np.where((np.arange(seg.size) // 5) % 2 == 0, 220, 36)
    return data


@pytest.mark.parametrize("R", [8, 32])
def test_group_with_one_weighted_row_is_zero(oracle, R):
    """tscrunch_weights keeps a group only when (sum of the weights of its rows with w >= 0.2) / 8 >= 0.2: a group of
    seven flagged rows and one clean row has one row to sum and a mean weight of 1 / 8, so all four excised products
    are 0 (code of 0) there, not the one row's value -- a test on `any row summed` instead would pass everywhere else
    in this suite."""
    lp = libpb()
    data = _thin_group_input(R)
    res, _, _ = oracle_run(oracle, data, R, rfi_mode=2, npol=2, nbit=8)
    w = res[1].weights.reshape(2, R)[0, R - 8:]
    kept = w[w >= np.float32(0.2)]
    assert kept.size == 1 and float(kept.sum()) / 8 < 0.2, w
    for mode in (1, 2):
        ref = CR.run(oracle, data, R, mode, 8)
        last = ref[1][1][1, :, R // 8 - 1]                     # excised stream, segment 1, [4 products][4096]
        assert (last == 0).all() and (ref[1][1][0] != 0).any(axis=(1, 2)).all()
        if mode == 2:
            assert (ref[0][1][1, :, R // 8 - 1] != 0).any(axis=1).all()
        got, bps = run_calls(lp, [data], R, mode, 8, calls=(2,), max_seg=2)
        check(got[0], bps[0], {st: ref[st][0] for st in ref}, {st: ref[st][1] for st in ref}, ref.state.bp, mode,
              "R %d, mode %d" % (R, mode), exact_nan=True)


def test_reset_bandpass_of_one_antenna_of_two(oracle):
    """Two antennas with their own data, R = 32, RFI mode 2, 2 bit, two buffer sets, four batches of one segment;
    pb_reset_bandpass(1) once the second batch is queued.  Antenna 0 goes on as one stream; antenna 1 starts from a
    zero bandpass (initialised from the third batch's segment) in both streams."""
    lp = libpb()
    R, nbit, mode = 32, 2, 2
    datas = [make_input(81, R, 4), make_input(82, R, 4)]

    def after_call(h, k):
        if k == 1:
            h.reset_bandpass(1)

    got, bps = run_calls(lp, datas, R, mode, nbit, calls=(1, 1, 1, 1), max_seg=1, nsets=2, lag=1, after_call=after_call)
    whole = [CR.run(oracle, d, R, mode, nbit) for d in datas]
    head = CR.run(oracle, datas[1][:2], R, mode, nbit)
    tail = CR.run(oracle, datas[1][2:], R, mode, nbit, state=CR.CohState())
    cat = {st: (np.concatenate([head[st][0], tail[st][0]]), np.concatenate([head[st][1], tail[st][1]])) for st in (0, 1)}
    for st in (0, 1):                          # a reset that did nothing, or hit antenna 0, would give `whole`
        assert not np.array_equal(cat[st][0], whole[1][st][0]) and not np.array_equal(tail.state.bp[st], whole[1].state.bp[st])
    check(got[0], bps[0], {st: whole[0][st][0] for st in (0, 1)}, {st: whole[0][st][1] for st in (0, 1)},
          whole[0].state.bp, mode, "antenna 0", exact_nan=True)
    check(got[1], bps[1], {st: cat[st][0] for st in (0, 1)}, {st: cat[st][1] for st in (0, 1)}, tail.state.bp, mode,
          "antenna 1 (reset)", exact_nan=True)
