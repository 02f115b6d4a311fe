"""The fringe-stopping correlator on the GPU (pb_correlate_tracked) against the CPU restatement of its definition
(tests/correlate_track_ref.py): visibilities and rows_used bit for bit over antenna counts 1 .. 6 -- which between them
launch every kernel tile --, both streams, uniform gates (the workgroup's first rows equal: the loop with scalar table
reads), gates whose first row differs per channel (the other loop), several row_base, ties of rint; the zero model
against pb_correlate_gated; the effect on a drifting source through the channeliser; a model continued over batches;
side effects, pipelining and refusals."""
import importlib
import re

import numpy as np
import pytest

import correlate_ref as XR
import correlate_track_ref as TR
import fringe_synth as FS
from helpers import libpb, make_input

pytestmark = pytest.mark.gpu

NFFT, NCO = 12500, 4096


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
    """test_gpu_correlate's seeded inputs (RFI bursts, a fully flagged row, a dropped frame) and their spectra"""
    key = (A, R, nseg)
    if key not in _cache:
        data = np.stack([make_input(200 + 7 * a + R, R, nseg) for a in range(A)])
        _cache[key] = (data, XR.batch_spectra(oracle, data, R, 2))
    return _cache[key]


def _model(A, seed):
    """non-zero entries in all four columns for every antenna: delays of up to 200 samples drifting by up to 0.05 a row,
    phases of up to a turn drifting by up to a tenth of a turn a row"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1, 1, (A, 4)) * np.array([200.0, 0.05, 1.0, 0.1])
    assert np.all(m != 0)
    return m


@pytest.mark.parametrize("A", [1, 2, 3, 4, 5, 6])
def test_bit_exact(oracle, A):
    """1 .. 4: a group against itself; 5: the 4 x 1 cross tile; 6: the 4 x 2 cross tile"""
    lp = libpb()
    R, nseg = 8, 3
    T = R * nseg
    data, spec = _case(oracle, A, R, nseg)
    model = _model(A, 10 + A)
    ties = np.zeros((A, 4))
    ties[A // 2, 2] = 0.5                                       # turn = 0.5 exactly in every channel: rint's tie
    assert np.all(TR.turns(ties, T)[0][A // 2] == 0.5) and np.all(TR.turns(ties, T)[1][A // 2] == np.float32(0.5))
    rnd = np.random.default_rng(A).integers(0, T - 5 + 1, size=(2, NCO)).astype(np.int32)
    rnd[0, 0], rnd[1, 1] = 0, T - 5
    with _handle(lp, A, R, nseg, 2) as h:
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            X, w = spec[st]
            w = w if st else None
            # uniform gates of 1, 8, 24 and 12 rows (the 12-row gates cross a segment boundary), over the row bases
            for nrows, base, m in ((1, 0, model), (8, 24, model), (24, -7, model), (12, 0, model), (12, 24, ties)):
                ref = TR.correlate_tracked(X, w, XR.uniform_row0(T, nrows), nrows, m, base)
                _same(h.correlate_tracked(st, nseg, m, base, nrows=nrows), ref)
                assert st == 0 or nrows < 8 or ref[1].min() < nrows      # the inputs hold a fully flagged row
            # the same through an explicit row0, and first rows that differ per channel
            u12 = XR.uniform_row0(T, 12).astype(np.int32)
            _same(h.correlate_tracked(st, nseg, model, -7, row0=u12, nrows=12),
                  TR.correlate_tracked(X, w, u12, 12, model, -7))
            _same(h.correlate_tracked(st, nseg, model, 24, row0=rnd, nrows=5), TR.correlate_tracked(X, w, rnd, 5, model, 24))


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


def test_gated_dedispersed(gated):
    h, spec, T, nseg = gated
    corr = importlib.import_module("vlite-fast_amd.correlate")
    nrows, model = 5, _model(3, 3)
    row0 = np.stack([corr.dm_row0(0.3, t0, T - nrows + 1) for t0 in (0, 7, 14)])
    assert row0.max() - row0.min() > 20 and len(np.unique(row0[0])) > 10
    # some workgroups of this gate have equal first rows and some have not: both loops run in one launch
    blocks = row0[0].reshape(-1, 64)
    assert (blocks.min(axis=1) == blocks.max(axis=1)).any() and (blocks.min(axis=1) != blocks.max(axis=1)).any()
    for st in (0, 1):
        X, w = spec[st]
        for base in (0, -7):
            _same(h.correlate_tracked(st, nseg, model, base, row0=row0, nrows=nrows),
                  TR.correlate_tracked(X, w if st else None, row0, nrows, model, base))


def test_zero_model_is_the_gated_call(gated):
    """r = 0 gives (cr, sr) = (1, 0): only signs of zero may differ, and numpy's == does not tell them apart"""
    h, _, T, nseg = gated
    zero = np.zeros((3, 4))
    rnd = np.random.default_rng(5).integers(0, T - 5 + 1, size=(2, NCO)).astype(np.int32)
    for st in (0, 1):
        for row0, nrows in ((XR.uniform_row0(T, 12).astype(np.int32), 12), (rnd, 5)):
            gv, gu = h.correlate_gated(st, nseg, row0, nrows)
            for base in (0, 1000):
                tv, tu = h.correlate_tracked(st, nseg, zero, base, row0=row0, nrows=nrows)
                assert np.array_equal(tv, gv) and np.array_equal(tu, gu)
        assert np.abs(gv).max() > 0


def _drifting_batch(lp, u8, R, nseg, model, row_base=0):
    """u8 [A][2][nseg * R * 12500] through a coherence handle, raw stream, one gate of the whole batch -> vis [nbl][4][4096]"""
    A = u8.shape[0]
    with _handle(lp, A, R, nseg, 0) as h:
        _submit(h, u8.reshape(A, 2, nseg, R * NFFT).transpose(0, 2, 1, 3))
        h.process(nseg)
        vis, used = h.correlate_tracked(0, nseg, model, row_base)
        assert vis.shape[0] == 1 and np.all(used == nseg * R)
        return vis[0]


def test_effect_through_the_channeliser():
    """test_correlate_track_ref_cpu's source as 3 antennas x 3 segments of 8 rows: the same two inequalities for the
    kernel's output (measured there in binary64: 0.507, 0.503, 0.505 tracked; 0.094, 0.068, 0.055 with the static model)"""
    lp = libpb()
    u8 = FS.drifting_antennas(FS.SEED, FS.ROWS, FS.D0, FS.D1, FS.P0, FS.P1, FS.SHARED)
    full = FS.model_of(FS.D0, FS.D1, FS.P0, FS.P1)
    bls = XR.baselines(3)
    tracked = FS.band_coherence(_drifting_batch(lp, u8, 8, 3, full), bls)
    static = FS.band_coherence(_drifting_batch(lp, u8, 8, 3, full * np.array([1.0, 0.0, 1.0, 0.0])), bls)
    print("tracked", tracked, "static model", static)
    for b in ((0, 1), (0, 2), (1, 2)):
        assert tracked[b] >= 0.45, (b, tracked[b])
        assert static[b] <= 0.2, (b, static[b])


def test_continuing_a_model():
    """two successive 24-row batches of one source whose phase on antenna 1 drifts by 1/48 turn a row (and whose delay
    by 0.002 samples a row): with row_base 0 and then 24 the band-coherent phase of baseline 0-1 is the same in both
    batches; with row_base 0 twice the second batch is 24 / 48 = 0.5 turn off (the delay's 0.048 samples add at most
    0.024 turn across the band)"""
    lp = libpb()
    d0, d1, p0, p1 = (0.0, 58.25), (0.0, 0.002), (0.0, 0.1), (0.0, 1.0 / 48)
    u8 = FS.drifting_antennas(11, 48, d0, d1, p0, p1).reshape(2, 2, 2, 24 * NFFT)         # [A][pol][batch][n]
    model = FS.model_of(d0, d1, p0, p1)

    def phase(batch, row_base):
        vis = _drifting_batch(lp, np.ascontiguousarray(u8[:, :, batch]), 8, 3, model, row_base)
        z = vis[1, 0].astype(np.complex128).sum()
        assert abs(z) / np.sqrt(vis[0, 0].real.astype(float) * vis[2, 0].real.astype(float)).sum() >= 0.45
        return np.angle(z) / (2 * np.pi)

    def apart(a, b):
        return abs((a - b + 0.5) % 1.0 - 0.5)

    first, second, second_from_zero = phase(0, 0), phase(1, 24), phase(1, 0)
    print("phases of baseline 0-1 in turns:", first, second, second_from_zero)
    assert apart(first, second) <= 0.05
    assert apart(first, second_from_zero) >= 0.4


def _device_bytes(lp, h):
    s = lp.PbSizes()
    h._chk(h._L.pb_query(h._h, s))
    return int(s.device_bytes)


def test_side_effects_and_pipelining(oracle):
    lp = libpb()
    A, R, per = 2, 16, 2
    T = per * R
    data = np.stack([make_input(300 + a, R, 2 * per) for a in range(A)])
    model = _model(A, 2)
    nbl = A * (A + 1) // 2
    results = {}
    for nsets in (1, 2):
        with _handle(lp, A, R, per, 2, nsets=nsets, keep_ave=True) as h:
            for b in range(2):
                h.select_set(b % nsets)
                _submit(h, data[:, b * per:(b + 1) * per])
                h.process(per)
                fetched = [h.fetch(a, 0, per, ave=True) for a in range(A)]
                plain = h.correlate(1, per, R)
                timers = h.correlate_timers()
                before = _device_bytes(lp, h)
                got = h.correlate_tracked(1, per, model, b * T, nrows=R)
                grown = _device_bytes(lp, h) - before
                if b == 0:
                    # the visibilities, rows_used, the first rows, the tables and the excised stream's row counts
                    assert grown == per * nbl * NCO * (32 + 4) + per * NCO * 4 + T * A * 16 + nbl * (T + 1) * 4
                else:
                    assert grown == 0
                assert h.correlate_tracked_timers()[1] > 0 and h.correlate_timers() == timers
                h.correlate_tracked(1, per, model, b * T, nrows=R)
                assert _device_bytes(lp, h) == before + grown
                again = h.correlate(1, per, R)
                assert again[0].tobytes() == plain[0].tobytes() and again[1].tobytes() == plain[1].tobytes()
                for a in range(A):
                    f = h.fetch(a, 0, per, ave=True)
                    for k in ("raw", "kur", "ave_raw", "ave_kur"):
                        assert f[k].tobytes() == fetched[a][k].tobytes(), (b, a, k)
                results[nsets, b] = got
    X, w = XR.batch_spectra(oracle, data[:, :per], R, 2)[1]
    _same(results[1, 0], TR.correlate_tracked(X, w, XR.uniform_row0(T, R), R, model, 0))
    for b in range(2):
        assert results[1, b][0].tobytes() == results[2, b][0].tobytes() and np.array_equal(results[1, b][1], results[2, b][1])


def test_refusals():
    lp = libpb()
    R, nseg = 8, 2
    data = make_input(1, R, nseg)[None]
    ok = np.zeros((1, 4))
    with lp.PbHandle(nant=1, npol=2, rfi_mode=2, rows_per_seg=R, max_seg=nseg) as h:      # coherence = 0
        _submit(h, data)
        h.process(nseg)
        with pytest.raises(ValueError, match="coherence"):
            h.correlate_tracked(0, nseg, ok)
    with _handle(lp, 9, R, 1, 0) as h:                                                    # nant > 8
        with pytest.raises(ValueError, match="8 antennas"):
            h.correlate_tracked(0, 1, np.zeros((9, 4)))
    for rfi_mode, stream in ((0, 1), (1, 0)):
        with _handle(lp, 1, R, nseg, rfi_mode) as h:
            _submit(h, data)
            h.process(nseg)
            with pytest.raises(ValueError, match="rfi_mode"):
                h.correlate_tracked(stream, nseg, ok)
            with pytest.raises(ValueError, match="stream"):
                h.correlate_tracked(2, nseg, ok)
    with _handle(lp, 1, R, nseg, 2, nsets=2) as h:
        with pytest.raises(lp.PbError, match="no pb_process"):
            h.correlate_tracked(0, nseg, ok)
        _submit(h, data[:, :1])
        h.process(1)
        with pytest.raises(lp.PbError, match="more segments"):
            h.correlate_tracked(0, 2, ok)
        h.select_set(1)                                      # the other set has seen no batch
        with pytest.raises(lp.PbError, match="no pb_process"):
            h.correlate_tracked(0, 1, ok)
        h.select_set(0)
        before = h.correlate(0, 1, R)
        bytes_before = _device_bytes(lp, h)

        def refused(text, *a, **kw):
            with pytest.raises(ValueError, match=re.escape(text)):
                h.correlate_tracked(*a, **kw)
            assert text in h._L.pb_last_error(h._h).decode()
            assert _device_bytes(lp, h) == bytes_before                      # nothing was allocated, nothing queued
            again = h.correlate(0, 1, R)
            assert again[0].tobytes() == before[0].tobytes() and np.array_equal(again[1], before[1])

        refused("nseg", 0, 0, ok)
        for bad in (0, -1, 3, 2 * R):                                            # uniform gates that do not fit
            refused("positive" if bad <= 0 else "divide", 0, 1, ok, nrows=bad)
        L, i32p, f64p = h._L, lp.C.POINTER(lp.C.c_int32), lp.C.POINTER(lp.C.c_double)
        vis, used = np.empty((1, 1, 4, NCO), np.complex64), np.empty((1, 1, NCO), np.int32)

        def raw(row0, ngate, nrows, model):
            return L.pb_correlate_tracked(h._h, 0, 1, row0.ctypes.data_as(i32p) if row0 is not None else None, ngate, nrows,
                                          model.ctypes.data_as(f64p) if model is not None else None, 0,
                                          vis.ctypes.data_as(lp.C.POINTER(lp.C.c_float)), used.ctypes.data_as(i32p))

        assert raw(None, 2, R, ok) == -22 and "quotient" in L.pb_last_error(h._h).decode()      # ngate is not T / nrows
        assert raw(None, 1, R, None) == -22 and "model is null" in L.pb_last_error(h._h).decode()
        assert raw(np.zeros((1, NCO), np.int32), 0, 1, ok) == -22 and "positive" in L.pb_last_error(h._h).decode()
        zero = np.zeros((1, NCO), np.int32)
        for nrows in (0, -2):
            refused("positive", 0, 1, ok, row0=zero, nrows=nrows)
        for r0, nrows in ((-1, 1), (R, 1), (R - 2, 3), (0, R + 1)):
            row0 = zero.copy()
            row0[0, 4095] = r0
            refused("window", 0, 1, ok, row0=row0, nrows=nrows)
        for col in range(4):
            for v in (np.nan, np.inf, -np.inf):
                m = ok.copy()
                m[0, col] = v
                refused("not finite", 0, 1, m)
        big = 2.0 ** 24
        # |d| or |p| above 2^24 at the batch's first row, at its last row, and through row_base
        for m, base in (([big + 2, 0, 0, 0], 0), ([0, 0, -big - 2, 0], 0), ([big, 1.0, 0, 0], 0), ([0, 0, big, 1.0], 0),
                        ([0, 1.0, 0, 0], 2 ** 24 + 1), ([0, 0, 0, -1.0], 2 ** 24 + 1), ([0, 1.0, 0, 0], -2 ** 24 - 1)):
            refused("2^24", 0, 1, np.array([m], np.float64), base)
        refused("row_base", 0, 1, ok, 2 ** 63 - 1)
        # the largest values that pass: 2^24 at the last row
        h.correlate_tracked(0, 1, np.array([[big - (R - 1), 1.0, -big, 0.0]]))
        h.correlate_tracked(0, 1, ok, row0=np.full((1, NCO), R - 3, np.int32), nrows=3)      # the last window that fits
        assert all(t > 0 for t in h.correlate_tracked_timers())
