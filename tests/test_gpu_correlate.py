"""The correlator on the GPU (pb_correlate, pb_correlate_gated) against the CPU restatement of its definition
(tests/correlate_ref.py): visibilities and rows_used bit for bit, over antenna counts 1, 2, 3, 5 and 6, 7, 8 -- which
between them launch every kernel tile (the one- to four-antenna groups, the 4x1 and the 4x2 cross tiles) --, both
streams, gates that cross segments and gates whose first row differs per channel; pipelining, side effects, refusals,
and a delay recovered through the handle."""
import importlib

import numpy as np
import pytest

import correlate_ref as XR
from helpers import libpb, make_input

pytestmark = pytest.mark.gpu

NFFT, NCO = 12500, 4096


def _streams(rfi_mode):
    return (0,) if rfi_mode == 0 else (1,) if rfi_mode == 1 else (0, 1)


def _handle(lp, A, R, nseg, rfi_mode, **kw):
    return lp.PbHandle(nant=A, nbit=8, npol=2, rfi_mode=rfi_mode, rows_per_seg=R, max_seg=nseg, coherence=True, **kw)


def _submit(h, data):
    """data u8 [A][nseg][2][n]"""
    for a in range(data.shape[0]):
        for s in range(data.shape[1]):
            h.submit_planar(a, s, data[a, s, 0], data[a, s, 1])


def _same(got, ref):
    gv, gu = got
    rv, ru = ref
    assert gv.shape == rv.shape and gu.shape == ru.shape
    bad = np.argwhere(gv.view(np.uint32) != rv.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4])
    assert np.array_equal(gu, ru)


_cache = {}


def _case(oracle, A, R, nseg):
    """seeded inputs (RFI bursts, a fully flagged row, a dropped frame) and their spectra for both streams"""
    key = (A, R, nseg)
    if key not in _cache:
        data = np.stack([make_input(200 + 7 * a + R, R, nseg) for a in range(A)])
        _cache[key] = (data, XR.batch_spectra(oracle, data, R, 2))
    return _cache[key]


@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("R", [8, 16])
@pytest.mark.parametrize("A", [1, 2, 3, 5])
def test_ungated_bit_exact(oracle, A, R, nseg):
    lp = libpb()
    data, spec = _case(oracle, A, R, nseg)
    T = nseg * R
    int_rows = [1, 8, T] + ([12] if (R, nseg) == (8, 3) else [])
    ref = {}
    for st in (0, 1):
        X, w = spec[st]
        for n in int_rows:
            ref[st, n] = XR.correlate(X, w if st else None, XR.uniform_row0(T, n), n)
    for rfi_mode in (0, 1, 2):
        with _handle(lp, A, R, nseg, rfi_mode) as h:
            assert h.correlate_info() == (A * (A + 1) // 2, 4)
            _submit(h, data)
            h.process(nseg)
            for st in _streams(rfi_mode):
                for n in int_rows:
                    got = h.correlate(st, nseg, n)
                    _same(got, ref[st, n])
                    if st == 0:
                        assert np.all(got[1] == n)
                # the inputs hold a fully flagged row: the case cannot pass empty
                if st == 1:
                    assert ref[1, 8][1].min() < 8 and ref[1, 1][1].min() == 0 and ref[1, T][1].min() < T
                    assert ref[1, T][1].max() <= T


@pytest.mark.parametrize("A", [6, 7, 8])
def test_second_antenna_group_bit_exact(oracle, A):
    """beyond five antennas: the second group of four against itself with 2, 3 and 4 antennas, and group 0 against it
    two antennas at a time (one 4x2 cross tile; 4x2 + 4x1; two 4x2) -- with the grid above (a lone fifth antenna: the 4x1
    cross tile) every kernel tile has run.  Both streams, a gate that crosses a segment boundary, and per-channel first
    rows."""
    lp = libpb()
    R, nseg = 8, 3
    T = R * nseg
    data, spec = _case(oracle, A, R, nseg)
    row0 = np.random.default_rng(A).integers(0, T - 5 + 1, size=(2, NCO)).astype(np.int32)
    with _handle(lp, A, R, nseg, 2) as h:
        assert h.correlate_info() == (A * (A + 1) // 2, 4)
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            X, w = spec[st]
            ref = XR.correlate(X, w if st else None, XR.uniform_row0(T, 12), 12)
            _same(h.correlate(st, nseg, 12), ref)
            assert st == 0 or ref[1].min() < 12
            _same(h.correlate_gated(st, nseg, row0, 5), XR.correlate(X, w if st else None, row0, 5))


@pytest.fixture(scope="module")
def gated(oracle):
    """three antennas, three 16-row segments, both streams: the handle with its batch processed, and the spectra"""
    lp = libpb()
    A, R, nseg = 3, 16, 3
    data, spec = _case(oracle, A, R, nseg)
    h = _handle(lp, A, R, nseg, 2)
    _submit(h, data)
    h.process(nseg)
    yield h, spec, R * nseg, nseg
    h.close()


@pytest.mark.parametrize("nrows", [1, 5])
def test_gated_random_first_rows(gated, nrows):
    h, spec, T, nseg = gated
    row0 = np.random.default_rng(nrows).integers(0, T - nrows + 1, size=(3, NCO)).astype(np.int32)
    row0[0, 0], row0[1, 1] = 0, T - nrows
    for st in (0, 1):
        X, w = spec[st]
        ref = XR.correlate(X, w if st else None, row0, nrows)
        _same(h.correlate_gated(st, nseg, row0, nrows), ref)
    assert ref[1].min() < nrows


def test_gated_dedispersed(gated):
    h, spec, T, nseg = gated
    corr = importlib.import_module("vlite-fast_amd.correlate")
    nrows = 5
    row0 = np.stack([corr.dm_row0(0.3, t0, T - nrows + 1) for t0 in (0, 7, 14)])
    assert row0.max() - row0.min() > 20 and len(np.unique(row0[0])) > 10
    for st in (0, 1):
        X, w = spec[st]
        _same(h.correlate_gated(st, nseg, row0, nrows), XR.correlate(X, w if st else None, row0, nrows))


def test_constant_first_rows_give_the_ungated_bytes(gated):
    h, _, T, nseg = gated
    for st in (0, 1):
        a = h.correlate(st, nseg, 12)
        b = h.correlate_gated(st, nseg, XR.uniform_row0(T, 12), 12)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        # and a shorter batch of the same set: the first segment alone
        c = h.correlate(st, 1, 8)
        assert c[0].tobytes() == h.correlate(st, nseg, 8)[0][:2].tobytes()


def test_auto_cross_hand_is_the_unnormalised_coherence(gated):
    """product 1 of an auto = the sums over the gate's rows of the re / im lines of the coherence definition.  The two
    lines are restated here from the spectra (coherence_ref.detect computes them but returns only the normalised
    CR / CI), in the form coherence_ref writes them."""
    h, spec, T, nseg = gated
    F = np.float32
    for st in (0, 1):
        X, _ = spec[st]
        vis, _ = h.correlate(st, nseg, 12)
        for a, b in ((0, 0), (1, 3), (2, 5)):
            ax, ay, bx, by = X[a, 0].real, X[a, 0].imag, X[a, 1].real, X[a, 1].imag
            re = ax * bx + ay * by
            im = ay * bx - ax * by
            for g in range(T // 12):
                sr, si = np.zeros(NCO, F), np.zeros(NCO, F)
                for t in range(12 * g, 12 * g + 12):
                    sr = sr + re[t]
                    si = si + im[t]
                assert np.array_equal(vis[g, b, 1].real.view(np.uint32), sr.view(np.uint32))
                assert np.array_equal(vis[g, b, 1].imag.view(np.uint32), si.view(np.uint32))


def _batches(lp, data, R, per, nsets, stream, correlate):
    """data [A][nbatch * per][2][n] through a handle in batches of `per` segments -> per batch the correlation (if
    asked for) and what pb_fetch returns"""
    A = data.shape[0]
    out = []
    with _handle(lp, A, R, per, 2, nsets=nsets, keep_ave=True) as h:
        for b in range(data.shape[1] // per):
            h.select_set(b % nsets)
            _submit(h, data[:, b * per:(b + 1) * per])
            h.process(per)
            c = h.correlate(stream, per, R) if correlate else None
            if correlate:
                h.correlate_gated(stream, per, np.full((2, NCO), 3, np.int32), R - 3)
            f = [h.fetch(a, 0, per, ave=True) for a in range(A)]
            out.append((c, f))
    return out


def test_pipelining_and_side_effects(oracle):
    lp = libpb()
    A, R, per = 2, 16, 2
    data = np.stack([make_input(300 + a, R, 3 * per) for a in range(A)])
    one = _batches(lp, data, R, per, 1, 1, True)
    two = _batches(lp, data, R, per, 2, 1, True)
    plain = _batches(lp, data, R, per, 2, 1, False)
    X, w = XR.batch_spectra(oracle, data[:, :per], R, 2)[1]
    _same(one[0][0], XR.correlate(X, w, XR.uniform_row0(per * R, R), R))
    for b in range(3):
        assert one[b][0][0].tobytes() == two[b][0][0].tobytes() and np.array_equal(one[b][0][1], two[b][0][1])
        for a in range(A):
            for k in ("raw", "kur", "ave_raw", "ave_kur"):
                assert two[b][1][a][k].tobytes() == plain[b][1][a][k].tobytes(), (b, a, k)
                assert one[b][1][a][k].tobytes() == plain[b][1][a][k].tobytes(), (b, a, k)


def test_refusals():
    lp = libpb()
    R, nseg = 8, 2
    data = make_input(1, R, nseg)[None]
    with lp.PbHandle(nant=1, npol=2, rfi_mode=2, rows_per_seg=R, max_seg=nseg) as h:      # coherence = 0
        _submit(h, data)
        h.process(nseg)
        with pytest.raises(ValueError, match="coherence"):
            h.correlate(0, nseg, R)
    with _handle(lp, 9, R, 1, 0) as h:                                                    # nant > 8
        with pytest.raises(ValueError, match="8 antennas"):
            h.correlate(0, 1, R)
    for rfi_mode, stream in ((0, 1), (1, 0)):
        with _handle(lp, 1, R, nseg, rfi_mode) as h:
            _submit(h, data)
            h.process(nseg)
            with pytest.raises(ValueError, match="rfi_mode"):
                h.correlate(stream, nseg, R)
            with pytest.raises(ValueError, match="stream"):
                h.correlate(2, nseg, R)
    with _handle(lp, 1, R, nseg, 2, nsets=2) as h:
        with pytest.raises(lp.PbError, match="no pb_process"):
            h.correlate(0, nseg, R)
        _submit(h, data[:, :1])
        h.process(1)
        with pytest.raises(lp.PbError, match="more segments"):
            h.correlate(0, 2, R)
        h.select_set(1)                                      # the other set has seen no batch
        with pytest.raises(lp.PbError, match="no pb_process"):
            h.correlate(0, 1, R)
        h.select_set(0)
        for bad in (0, -1, 3, 2 * R):
            with pytest.raises(ValueError, match="int_rows"):
                h.correlate(0, 1, bad)
        with pytest.raises(ValueError, match="nseg"):
            h.correlate(0, 0, R)
        ok = np.zeros((1, NCO), np.int32)
        for nrows in (0, -2):
            with pytest.raises(ValueError, match="positive"):
                h.correlate_gated(0, 1, ok, nrows)
        with pytest.raises(ValueError, match="positive"):
            h.correlate_gated(0, 1, np.zeros((0, NCO), np.int32), 1)
        for r0, nrows in ((-1, 1), (R, 1), (R - 2, 3), (0, R + 1)):
            row0 = ok.copy()
            row0[0, 4095] = r0
            with pytest.raises(ValueError, match="window"):
                h.correlate_gated(0, 1, row0, nrows)
        h.correlate_gated(0, 1, np.full((1, NCO), R - 3, np.int32), 3)         # the last window that fits
        assert h.correlate_timers()[0] > 0


def test_delay_through_the_handle():
    """antenna 1 = antenna 0's common component 58 samples late: lag bin 19 of 4096 (58 * 4096 / 12500 = 19.005)"""
    lp = libpb()
    corr = importlib.import_module("vlite-fast_amd.correlate")
    R = 8
    u8 = XR.delayed_antennas(5, R * NFFT, (0, 58))
    with _handle(lp, 2, R, 1, 0) as h:
        _submit(h, u8[:, None])
        h.process(1)
        vis, used = h.correlate(0, 1, R)
    lag = corr.lag_delays(vis[0], used[0])
    for k in range(2):
        assert lag.cycles[k, 0, 1] == 19 / 4096.0
        assert lag.peak[k, 0, 1] >= 10 * lag.third[k, 0, 1], (lag.peak[k, 0, 1], lag.third[k, 0, 1])
