"""The projecting beamformer on the GPU (pb_beamform_proj) against the CPU restatement of its definition
(tests/beamproj_ref.py): beams and rows_used bit for bit over every antenna count 1 .. 8, 1, 2, 3 and 5 beams (a
pair, one past a pair, one past the tile of four), windows of 1, 3 and all rows, both streams, per-channel shifts, fewer output samples than fit, random non-Hermitian matrices with exact zeros and an
all-zero channel; the unit matrix against pb_beamform; rows_used over every antenna; refusals and side effects; and the
physical test of DESIGN.md section 13 through the library's channeliser and correlator."""
import ctypes as C
import importlib

import numpy as np
import pytest

import beam_ref as BR
import beamproj_ref as PR
import correlate_ref as XR
import null_synth as NS
from helpers import libpb, make_input

pytestmark = pytest.mark.gpu

NFFT, NCO = 12500, 4096
F = np.float32
R = 16


def _handle(lp, A, nseg, rfi_mode=2, **kw):
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


def _case(oracle, A, nseg):
    """seeded inputs (RFI bursts, a fully flagged row, a dropped frame) and their spectra for both streams"""
    key = (A, nseg)
    if key not in _cache:
        data = np.stack([make_input(600 + 7 * a, R, nseg) for a in range(A)])
        _cache[key] = (data, XR.batch_spectra(oracle, data, R, 2))
    return _cache[key]


@pytest.mark.parametrize("A", [1, 2, 3, 4, 5, 6, 7, 8])
def test_bit_exact(oracle, A):
    """48 rows: more than one workgroup's run of rows at every tscr below T"""
    lp = libpb()
    corr = importlib.import_module("vlite-fast_amd.correlate")
    nseg = 3
    T = nseg * R
    data, spec = _case(oracle, A, nseg)
    delay, psi, gain = BR.five_beams(A, 90 + A)
    proj = PR.random_proj(A, 95 + A)
    rng = np.random.default_rng(A)
    random_shift = rng.integers(0, 6, NCO).astype(np.int32)
    assert np.any(np.diff(random_shift) != 0)
    dm_shift = corr.dm_row0(0.25, 0, T)
    assert dm_shift.max() >= R - 2 and len(np.unique(dm_shift)) > 5
    # per nbeam: psi and gain or not, the shift, and how many output samples fewer than fit
    variants = {1: (False, None, 0), 2: (True, random_shift, 0), 3: (True, dm_shift, 1), 5: (True, random_shift, 2)}
    with _handle(lp, A, nseg) as h:
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            X, w = spec[st]
            for nbeam, (full, sh, fewer) in variants.items():
                ps, ga = (psi[:nbeam], gain[:nbeam]) if full else (None, None)
                P = PR.detect(X, *PR.weights(proj, delay[:nbeam], ps, ga))
                for tscr in (1, 3, T):
                    s = None if tscr == T else sh
                    nout = None if tscr == T or not fewer else (T - int(s.max())) // tscr - fewer
                    ref = PR.beamform_proj(X, w if st else None, delay[:nbeam], proj, ps, ga, s, tscr, nout, detected=P)
                    got = h.beamform_proj(st, nseg, delay[:nbeam], proj, ps, ga, s, tscr, nout)
                    assert nout is None or got[0].shape[1] == nout
                    _same(got, ref)
                    assert st == 1 or np.all(got[1] == tscr)
            assert st == 0 or ref[1].min() < T                     # the inputs hold flagged rows
        assert h.beamform_proj_timers()[1] > 0


@pytest.mark.parametrize("A", [3, 6])
def test_unit_matrix_gives_pb_beamforms_beams(oracle, A):
    """as numbers (signs of zero may differ), both streams; on the raw stream rows_used too"""
    lp = libpb()
    nseg = 3
    data, _ = _case(oracle, A, nseg)
    delay, psi, gain = BR.five_beams(A, 20 + A)
    shift = (np.arange(NCO) % 5).astype(np.int32)
    with _handle(lp, A, nseg) as h:
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            want, wused = h.beamform(st, nseg, delay, psi, gain, shift, 4)
            got, used = h.beamform_proj(st, nseg, delay, PR.identity(A), psi, gain, shift, 4)
            assert np.abs(want).max() > 0 and np.array_equal(got, want)
            if st == 0:
                assert np.array_equal(used, wused)


def test_rows_used_counts_every_antenna(oracle):
    """the excised stream: a window's rows whose weight is > 0 for every antenna, one of gain 0 included, where
    pb_beamform counts the antennas of non-zero gain only"""
    lp = libpb()
    A, nseg, tscr = 3, 3, 4
    # antenna 2 alone has further rows flagged: a burst that the kurtosis excises
    data = np.stack([make_input(600 + 7 * a, R, nseg) for a in range(A)]).copy()
    rng = np.random.default_rng(9)
    burst = slice(5 * NFFT, 7 * NFFT)
    data[2, 1, :, burst] = np.where(rng.random((2, 2 * NFFT)) < 0.5, 0, 255).astype(np.uint8)
    spec = XR.batch_spectra(oracle, data, R, 2)
    X, w = spec[1]
    gain = np.array([[1, 1, 0], [1, 0, 0], [1, 1, 1]], F)
    delay = np.zeros((3, A))
    ref = PR.rows_used(w, nseg * R, 3, A, None, tscr, nseg * R // tscr)
    plain = BR.rows_used(w, nseg * R, gain, None, tscr, nseg * R // tscr)
    assert ref.min() < tscr and np.any(ref[0] < plain[0])          # antenna 2's rows make a difference
    with _handle(lp, A, nseg) as h:
        _submit(h, data)
        h.process(nseg)
        _, used = h.beamform_proj(1, nseg, delay, PR.identity(A), gain=gain, tscr=tscr)
        assert np.array_equal(used, ref)
        assert np.array_equal(used[0], used[1]) and np.array_equal(used[0], used[2])
        _, pused = h.beamform(1, nseg, delay, gain=gain, tscr=tscr)
        assert np.array_equal(pused, plain) and np.array_equal(pused[2], used[2])


def test_refusals_leave_the_handle_as_it_was():
    lp = libpb()
    nseg = 2
    data = make_input(1, R, nseg)[None]
    d1 = np.zeros((1, 1))
    eye = PR.identity(1)
    name = "pb_beamform_proj: "
    with lp.PbHandle(nant=1, npol=2, rfi_mode=2, rows_per_seg=R, max_seg=nseg) as h:      # coherence = 0
        _submit(h, data)
        h.process(nseg)
        with pytest.raises(ValueError, match=name + ".*coherence"):
            h.beamform_proj(0, nseg, d1, eye)
    with _handle(lp, 9, 1, 0) as h:                                                       # nant > 8
        with pytest.raises(ValueError, match=name + "at most 8 antennas"):
            h.beamform_proj(0, 1, np.zeros((1, 9)), PR.identity(9))
    for rfi_mode, stream in ((0, 1), (1, 0)):
        with _handle(lp, 1, nseg, rfi_mode) as h:
            _submit(h, data)
            h.process(nseg)
            with pytest.raises(ValueError, match=name + ".*rfi_mode"):
                h.beamform_proj(stream, nseg, d1, eye)
            with pytest.raises(ValueError, match=name + "stream"):
                h.beamform_proj(2, nseg, d1, eye)
    with _handle(lp, 1, nseg, 2, nsets=2, keep_ave=True) as h:
        with pytest.raises(lp.PbError, match=name + "no pb_process"):
            h.beamform_proj(0, nseg, d1, eye)
        _submit(h, data[:, :1])
        h.process(1)
        before = h.fetch(0, 0, 1, weights=True, ave=True)
        with pytest.raises(lp.PbError, match=name + "more segments"):
            h.beamform_proj(0, 2, d1, eye)
        h.select_set(1)                                      # the other set has seen no batch
        with pytest.raises(lp.PbError, match=name + "no pb_process"):
            h.beamform_proj(0, 1, d1, eye)
        h.select_set(0)
        with pytest.raises(ValueError, match=name + "nseg"):
            h.beamform_proj(0, 0, d1, eye, nout=1)
        for tscr, nout in ((0, 1), (-1, 1), (1, 0), (1, -3)):
            with pytest.raises(ValueError, match=name + "tscr and nout"):
                h.beamform_proj(0, 1, d1, eye, tscr=tscr, nout=nout)
        for nbeam in (0, 65):
            with pytest.raises(ValueError, match=name + "nbeam"):
                h.beamform_proj(0, 1, np.zeros((nbeam, 1)), eye, nout=1)
        fp, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
        eye_p = eye.ctypes.data_as(fp)
        assert h._L.pb_beamform_proj(h._h, 0, 1, 1, None, None, None, eye_p, None, 1, 1, None, None) == -22
        assert name + "delay is null" in h._L.pb_last_error(h._h).decode()
        assert h._L.pb_beamform_proj(h._h, 0, 1, 1, d1.ctypes.data_as(f64p), None, None, None, None, 1, 1, None, None) == -22
        assert name + "proj is null" in h._L.pb_last_error(h._h).decode()
        for bad in (np.nan, np.inf, -np.inf):
            with pytest.raises(ValueError, match=name + "a delay is not finite"):
                h.beamform_proj(0, 1, np.full((1, 1), bad), eye)
            with pytest.raises(ValueError, match=name + "a psi is not finite"):
                h.beamform_proj(0, 1, d1, eye, psi=np.full((1, 1), bad))
            with pytest.raises(ValueError, match=name + "a gain is not finite"):
                h.beamform_proj(0, 1, d1, eye, gain=np.full((1, 1), bad, F))
            for value in (complex(bad, 0.0), complex(1.0, bad)):
                p = eye.copy()
                p[1, 4095, 0, 0] = value
                with pytest.raises(ValueError, match=name + "a proj value is not finite"):
                    h.beamform_proj(0, 1, d1, p)
        for bad in (2.0 ** 24 + 2, -2.0 ** 24 - 2):
            with pytest.raises(ValueError, match=name + ".*2\\^24"):
                h.beamform_proj(0, 1, np.full((1, 1), bad), eye)
        with pytest.raises(ValueError, match="proj must be"):
            h.beamform_proj(0, 1, d1, np.zeros((2, NCO, 2, 2), np.complex64))
        shift = np.zeros(NCO, np.int32)
        shift[4095] = -1
        with pytest.raises(ValueError, match=name + "a shift is negative"):
            h.beamform_proj(0, 1, d1, eye, shift=shift, nout=1)
        for top, tscr, nout in ((0, 1, R + 1), (0, 3, 6), (1, 1, R), (R, 1, 1), (2, 5, 3), (0, 2 ** 20, 2 ** 11)):
            shift[4095] = top
            with pytest.raises(ValueError, match=name + "a window"):
                h.beamform_proj(0, 1, d1, eye, shift=shift, tscr=tscr, nout=nout)
        # 64 beams x 513 samples x 64 KiB
        assert h._L.pb_beamform_proj(h._h, 0, 1, 64, np.zeros(64).ctypes.data_as(f64p), None, None, eye_p, None, 1, 513,
                                     None, None) == -22
        assert name + "outputs beyond 2 GiB" in h._L.pb_last_error(h._h).decode()
        # nothing of all that reached the handle
        after = h.fetch(0, 0, 1, weights=True, ave=True)
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k
        # and a call that is taken leaves pb_fetch's outputs alone too; its buffers show in device_bytes
        s = lp.PbSizes()
        h._chk(h._L.pb_query(h._h, s))
        bytes0 = int(s.device_bytes)
        shift[4095] = R - 3
        beams, used = h.beamform_proj(1, 1, d1, eye, shift=shift, tscr=3)          # the last window that fits
        assert beams.shape == (1, 1, 4, NCO) and used.shape == (1, 1, NCO)
        h._chk(h._L.pb_query(h._h, s))
        # the matrices, the weights, the beams, rows_used and the row counts
        assert int(s.device_bytes) - bytes0 >= beams.nbytes + used.nbytes + 2 * NCO * 8 + 2 * NCO * 8 + (R + 1) * 4
        after = h.fetch(0, 0, 1, weights=True, ave=True)
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k
        # either output may be left out
        only_b, only_u = np.zeros_like(beams), np.zeros_like(used)
        i32p = C.POINTER(C.c_int32)
        args = (h._h, 1, 1, 1, d1.ctypes.data_as(f64p), None, None, eye_p, shift.ctypes.data_as(i32p), 3, 1)
        h._chk(h._L.pb_beamform_proj(*(args + (only_b.ctypes.data_as(fp), None))))
        h._chk(h._L.pb_beamform_proj(*(args + (None, only_u.ctypes.data_as(i32p)))))
        assert only_b.tobytes() == beams.tobytes() and np.array_equal(only_u, used)


def test_nulls_take_the_interferer_out_of_the_beam(oracle):
    """null_synth through the library's channeliser; the training gates from pb_correlate_gated, added on the host;
    nulling.projectors; pb_beamform_proj: the two thresholds of the CPU test.  Then the closure: the nulled beams over
    gates of a segment against the quadratic form of pb_correlate's visibilities, within the derived bound."""
    lp = libpb()
    nulling = importlib.import_module("vlite-fast_amd.nulling")
    A, nseg = 4, 4
    T = nseg * R
    assert T == NS.CASE["nrows"]
    u8 = NS.case_antennas()
    data = np.ascontiguousarray(u8.reshape(A, 2, nseg, R * NFFT).transpose(0, 2, 1, 3))
    delay = np.array([NS.CASE["sky_delays"]])
    with _handle(lp, A, nseg, 0) as h:
        _submit(h, data)
        h.process(nseg)

        def gates(first, nrows):
            return h.correlate_gated(0, nseg, np.repeat(np.asarray(first, np.int32)[:, None], NCO, axis=1), nrows)[0]

        NS.physical_checks(A, lambda: h.beamform(0, nseg, delay)[0], lambda proj: h.beamform_proj(0, nseg, delay, proj)[0],
                           gates)
        # nulling.training_vis is those gates
        vis = nulling.training_vis(h, 0, nseg, *NS.TRAIN)
        want = sum(gates(first, nrows).astype(np.complex128).sum(axis=0) for first, nrows in nulling.gate_rows(0, 48, R))
        assert np.array_equal(vis, want)
        proj, _ = nulling.projectors(nulling.covariances(vis, A), 1)
        beams, _ = h.beamform_proj(0, nseg, delay, proj, tscr=R)
        gate_vis, _ = h.correlate(0, nseg, R)
    X = XR.batch_spectra(oracle, data, R, 0)[0][0]
    form = PR.from_visibilities64(gate_vis, PR.weights64(proj, delay))
    bound = PR.error_bound(X, proj, None, None, R) + PR.error_bound(X, proj, None, None, R, through="vis")
    assert beams.shape == form.shape == bound.shape and bound.min() > 0
    worst = (np.abs(form - beams) / bound).max()
    print("pb_beamform_proj against the form of pb_correlate's visibilities: largest error / bound = %.4f" % worst)
    assert worst <= 1.0
