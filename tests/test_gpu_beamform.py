"""The beamformer on the GPU (pb_beamform) against the CPU restatement of its definition (tests/beam_ref.py): beams and
rows_used bit for bit, over every antenna count 1 .. 8, one beam, a full tile of four and one beam past it, windows
of 1, 3, 8 and all rows, both streams under every rfi_mode, fractional and negative delays, phases on ties of rint, gains
with zeros and a one-hot row, per-channel shifts; then the correlator's autos as a second GPU path, pipelining and side
effects, the sign of the delays through the handle, refusals and timers."""
import importlib

import numpy as np
import pytest

import beam_ref as BR
import correlate_ref as XR
from helpers import libpb, make_input

pytestmark = pytest.mark.gpu

NFFT, NCO = 12500, 4096
F = np.float32


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
    gb, gu = got
    rb, ru = ref
    assert gb.shape == rb.shape and gu.shape == ru.shape
    bad = np.argwhere(gb.view(np.uint32) != rb.view(np.uint32))
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


def _beams(A, seed):
    """five beams: delays with fractional parts up to +-20000 samples, some of them on ties of rint (6250 samples put
    every odd bin on a half turn), a psi, gains with zeros and a one-hot row"""
    rng = np.random.default_rng(seed)
    delay = rng.uniform(-20000.0, 20000.0, (5, A))
    delay[0, A - 1] = 6250.0
    delay[2, 0] = -6250.0
    delay[3, 0] = 18750.0
    delay[4, A - 1] = -0.5
    psi = rng.uniform(-2.0, 2.0, (5, A))
    psi[2, 0] = 0.5
    psi[3, 0] = 0.0
    gain = rng.uniform(0.5, 1.5, (5, A)).astype(F)
    gain[1] = 0
    gain[1, 1 % A] = 1
    gain[2, 0] = 0 if A > 1 else 1
    gain[3, A - 1] = 0
    return delay, psi, gain


@pytest.mark.parametrize("A,R", [(1, 8), (2, 16), (3, 8), (4, 16), (5, 16), (6, 8), (7, 16), (8, 8)])
def test_bit_exact(oracle, A, R):
    """R = 16: 48 rows, more than one workgroup's run of rows at every tscr below T"""
    lp = libpb()
    corr = importlib.import_module("vlite-fast_amd.correlate")
    nseg = 3
    T = nseg * R
    data, spec = _case(oracle, A, R, nseg)
    delay, psi, gain = _beams(A, 10 * A + R)
    rng = np.random.default_rng(A)
    random_shift = rng.integers(0, 6, NCO).astype(np.int32)
    dm_shift = corr.dm_row0(0.12 if R == 8 else 0.25, 0, T)           # rows 0 .. about T / 2
    assert dm_shift[0] == 0 and dm_shift.max() >= R - 2 and len(np.unique(dm_shift)) > 5
    # per nbeam: the optional arguments it is called with
    variants = {1: (None, None, None), 4: (psi, gain, random_shift), 5: (psi, gain, dm_shift)}
    ref, below = {}, False
    for st in (0, 1):
        X, w = spec[st]
        for nbeam, (ps, ga, sh) in variants.items():
            cut = lambda v: None if v is None else v[:nbeam]
            P = BR.detect(X, delay[:nbeam], cut(ps), cut(ga))
            for tscr in (1, 3, 8, T):
                s = None if tscr == T else sh
                ref[st, nbeam, tscr] = BR.beamform(X, w if st else None, delay[:nbeam], cut(ps), cut(ga), s, tscr, detected=P)
                if st == 1 and tscr > 1:
                    below = below or ref[st, nbeam, tscr][1].min() < tscr
    # the inputs hold a fully flagged row: rows_used of the excised stream falls below tscr
    assert below
    # and windows of the dispersed shift cross a segment boundary: a window of 3 rows that starts in a segment's last two
    starts = dm_shift[None, :] + 3 * np.arange(ref[0, 5, 3][0].shape[1])[:, None]
    assert np.any(starts % R > R - 3)
    for rfi_mode in (0, 1, 2):
        with _handle(lp, A, R, nseg, rfi_mode) as h:
            _submit(h, data)
            h.process(nseg)
            for st in _streams(rfi_mode):
                for nbeam, (ps, ga, sh) in variants.items():
                    cut = lambda v: None if v is None else v[:nbeam]
                    for tscr in (1, 3, 8, T):
                        s = None if tscr == T else sh
                        got = h.beamform(st, nseg, delay[:nbeam], cut(ps), cut(ga), s, tscr)
                        _same(got, ref[st, nbeam, tscr])
                        if st == 0:
                            assert np.all(got[1] == tscr)


def test_one_hot_beam_equals_the_correlators_auto(oracle):
    """two GPU paths: a one-hot beam of antenna a with delay 0 against products 0, 3 and 1 of that antenna's auto"""
    lp = libpb()
    A, R, nseg, tscr = 3, 8, 3, 8
    data, _ = _case(oracle, A, R, nseg)
    with _handle(lp, A, R, nseg, 2) as h:
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            beams, used = h.beamform(st, nseg, np.zeros((A, A)), gain=np.eye(A, dtype=F), tscr=tscr)
            vis, vused = h.correlate(st, nseg, tscr)
            assert beams.shape == (A, nseg * R // tscr, 4, NCO)
            for a in range(A):
                bl = XR.baselines(A).index((a, a))
                for q, v in enumerate((vis[:, bl, 0].real, vis[:, bl, 3].real, vis[:, bl, 1].real, vis[:, bl, 1].imag)):
                    assert np.array_equal(beams[a, :, q].view(np.uint32), np.ascontiguousarray(v).view(np.uint32)), (st, a, q)
                assert np.array_equal(used[a], vused[:, bl])
            assert st == 0 or used.min() < tscr


def _batches(lp, data, R, per, nsets, stream, beamform, delay):
    """data [A][nbatch * per][2][n] through a handle in batches of `per` segments -> per batch the beams (if asked for)
    and what pb_fetch returns"""
    A = data.shape[0]
    out = []
    with _handle(lp, A, R, per, 2, nsets=nsets, keep_ave=True) as h:
        for b in range(data.shape[1] // per):
            h.select_set(b % nsets)
            _submit(h, data[:, b * per:(b + 1) * per])
            h.process(per)
            c = h.beamform(stream, per, delay, tscr=R) if beamform else None
            if beamform:
                h.beamform(stream, per, delay[:1], shift=np.full(NCO, 3, np.int32), tscr=5)
            f = [h.fetch(a, 0, per, ave=True) for a in range(A)]
            out.append((c, f))
    return out


def test_pipelining_and_side_effects(oracle):
    lp = libpb()
    A, R, per = 2, 16, 2
    data = np.stack([make_input(300 + a, R, 3 * per) for a in range(A)])
    delay = np.array([[0.0, 17.25], [-3.5, 2.0]])
    one = _batches(lp, data, R, per, 1, 1, True, delay)
    two = _batches(lp, data, R, per, 2, 1, True, delay)
    plain = _batches(lp, data, R, per, 2, 1, False, delay)
    X, w = XR.batch_spectra(oracle, data[:, :per], R, 2)[1]
    _same(one[0][0], BR.beamform(X, w, delay, tscr=R))
    for b in range(3):
        assert one[b][0][0].tobytes() == two[b][0][0].tobytes() and np.array_equal(one[b][0][1], two[b][0][1])
        for a in range(A):
            for k in ("raw", "kur", "ave_raw", "ave_kur"):
                assert two[b][1][a][k].tobytes() == plain[b][1][a][k].tobytes(), (b, a, k)
                assert one[b][1][a][k].tobytes() == plain[b][1][a][k].tobytes(), (b, a, k)


def test_delays_through_the_handle():
    """the sign of the delays: the beam at delayed_antennas' true delays holds the three antennas' common half coherently,
    A s + (1 - s) = 2.0 times the sum of the single-antenna beams; at the negated delays only that sum"""
    lp = libpb()
    R = 8
    d = np.array([0.0, 58.0, 131.0])
    u8 = XR.delayed_antennas(5, R * NFFT, d)
    with _handle(lp, 3, R, 1, 0) as h:
        _submit(h, u8[:, None])
        h.process(1)
        beams, used = h.beamform(0, 1, np.concatenate([[d, -d], np.zeros((3, 3))]),
                                 gain=np.concatenate([np.ones((2, 3), F), np.eye(3, dtype=F)]), tscr=R)
    assert beams.shape == (5, 1, 4, NCO) and np.all(used == R)
    aa = beams[:, 0, 0].astype(np.float64).sum(axis=-1)
    print("coherent / incoherent AA: true %.4f  negated %.4f" % (aa[0] / aa[2:].sum(), aa[1] / aa[2:].sum()))
    assert aa[0] >= 1.9 * aa[2:].sum()
    assert aa[1] <= 1.1 * aa[2:].sum()


def test_refusals():
    lp = libpb()
    R, nseg = 8, 2
    data = make_input(1, R, nseg)[None]
    d1 = np.zeros((1, 1))
    with lp.PbHandle(nant=1, npol=2, rfi_mode=2, rows_per_seg=R, max_seg=nseg) as h:      # coherence = 0
        _submit(h, data)
        h.process(nseg)
        with pytest.raises(ValueError, match="coherence"):
            h.beamform(0, nseg, d1)
    with _handle(lp, 9, R, 1, 0) as h:                                                    # nant > 8
        with pytest.raises(ValueError, match="8 antennas"):
            h.beamform(0, 1, np.zeros((1, 9)))
    for rfi_mode, stream in ((0, 1), (1, 0)):
        with _handle(lp, 1, R, nseg, rfi_mode) as h:
            _submit(h, data)
            h.process(nseg)
            with pytest.raises(ValueError, match="rfi_mode"):
                h.beamform(stream, nseg, d1)
            with pytest.raises(ValueError, match="stream"):
                h.beamform(2, nseg, d1)
    with _handle(lp, 1, R, nseg, 2, nsets=2) as h:
        with pytest.raises(lp.PbError, match="no pb_process"):
            h.beamform(0, nseg, d1)
        _submit(h, data[:, :1])
        h.process(1)
        with pytest.raises(lp.PbError, match="more segments"):
            h.beamform(0, 2, d1)
        h.select_set(1)                                      # the other set has seen no batch
        with pytest.raises(lp.PbError, match="no pb_process"):
            h.beamform(0, 1, d1)
        h.select_set(0)
        with pytest.raises(ValueError, match="nseg"):
            h.beamform(0, 0, d1, nout=1)
        for tscr, nout in ((0, 1), (-1, 1), (1, 0), (1, -3)):
            with pytest.raises(ValueError, match="tscr and nout"):
                h.beamform(0, 1, d1, tscr=tscr, nout=nout)
        for nbeam in (0, 65):
            with pytest.raises(ValueError, match="nbeam"):
                h.beamform(0, 1, np.zeros((nbeam, 1)), nout=1)
        assert h._L.pb_beamform(h._h, 0, 1, 1, None, None, None, None, 1, 1, None, None) == -22
        assert "delay is null" in h._L.pb_last_error(h._h).decode()
        for bad in (np.nan, np.inf, -np.inf):
            with pytest.raises(ValueError, match="delay is not finite"):
                h.beamform(0, 1, np.full((1, 1), bad))
            with pytest.raises(ValueError, match="psi is not finite"):
                h.beamform(0, 1, d1, psi=np.full((1, 1), bad))
            with pytest.raises(ValueError, match="gain is not finite"):
                h.beamform(0, 1, d1, gain=np.full((1, 1), bad, F))
        for bad in (2.0 ** 24 + 2, -2.0 ** 24 - 2):
            with pytest.raises(ValueError, match="2\\^24"):
                h.beamform(0, 1, np.full((1, 1), bad))
        h.beamform(0, 1, np.full((1, 1), 2.0 ** 24))                             # the largest delay taken
        shift = np.zeros(NCO, np.int32)
        shift[4095] = -1
        with pytest.raises(ValueError, match="shift is negative"):
            h.beamform(0, 1, d1, shift=shift, nout=1)
        for top, tscr, nout in ((0, 1, R + 1), (0, 3, 3), (1, 1, R), (R, 1, 1), (3, 3, 2), (0, 2 ** 20, 2 ** 11)):
            shift[4095] = top
            with pytest.raises(ValueError, match="window"):
                h.beamform(0, 1, d1, shift=shift, tscr=tscr, nout=nout)
        shift[4095] = R - 3
        beams, used = h.beamform(0, 1, d1, shift=shift, tscr=3)                  # the last window that fits
        assert beams.shape == (1, 1, 4, NCO) and used.shape == (1, 1, NCO)
        assert h.beamform_timers()[1] > 0
        # 64 beams x 513 samples x 64 KiB
        assert h._L.pb_beamform(h._h, 0, 1, 64, np.zeros(64).ctypes.data_as(h._L.pb_beamform.argtypes[4]), None, None, None,
                                1, 513, None, None) == -22
        assert "2 GiB" in h._L.pb_last_error(h._h).decode()


def test_device_bytes_grow_and_either_output_may_be_null():
    import ctypes as C
    lp = libpb()
    R = 8
    data = make_input(3, R, 1)[None]
    with _handle(lp, 1, R, 1, 2) as h:
        _submit(h, data)
        h.process(1)
        s = lp.PbSizes()
        h._chk(h._L.pb_query(h._h, s))
        before = int(s.device_bytes)
        delay = np.array([[0.25], [-7.5]])
        beams, used = h.beamform(1, 1, delay, tscr=2)
        h._chk(h._L.pb_query(h._h, s))
        # the parameters, the shifts, the weights, the beams, rows_used and the row counts
        assert int(s.device_bytes) - before >= beams.nbytes + used.nbytes + 2 * NCO * 8 + 2 * (R + 1) * 4
        assert used.min() < 2
        f64p, fp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
        only_b, only_u = np.zeros_like(beams), np.zeros_like(used)
        h._chk(h._L.pb_beamform(h._h, 1, 1, 2, delay.ctypes.data_as(f64p), None, None, None, 2, R // 2,
                                only_b.ctypes.data_as(fp), None))
        h._chk(h._L.pb_beamform(h._h, 1, 1, 2, delay.ctypes.data_as(f64p), None, None, None, 2, R // 2, None,
                                only_u.ctypes.data_as(i32p)))
        assert only_b.tobytes() == beams.tobytes() and np.array_equal(only_u, used)
