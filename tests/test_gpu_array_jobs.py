"""The host side that correlator, beamformer and imager share (csrc/pb_job.h): buffers that grow between calls keep
nothing stale, device_bytes follows them, the stage timers, which refusal wins when a call breaks several rules, and
teardown.  The arithmetic is pinned elsewhere (test_gpu_correlate.py, test_gpu_beamform.py, test_gpu_image.py); here every
result is held, bit for bit, to the same call on a fresh handle fed the same bytes."""
import ctypes as C

import numpy as np
import pytest

import beamproj_ref as PR
from helpers import libpb, make_input

pytestmark = pytest.mark.gpu

A, R, S, NCO = 2, 8, 2, 4096
T = R * S


def _handle(lp, rfi_mode=2, coherence=True):
    return lp.PbHandle(nant=A, nbit=8, npol=2, rfi_mode=rfi_mode, rows_per_seg=R, max_seg=S, coherence=coherence)


_data = []


def _fed(lp, rfi_mode=2):
    """a handle whose selected set holds one processed batch of the module's seeded random bytes"""
    if not _data:
        _data.append(np.stack([make_input(900 + a, R, S) for a in range(A)]))
    h = _handle(lp, rfi_mode)
    for a in range(A):
        for s in range(S):
            h.submit_planar(a, s, _data[0][a, s, 0], _data[0][a, s, 1])
    h.process(S)
    return h


def _device_bytes(lp, h):
    s = lp.PbSizes()
    h._chk(h._L.pb_query(h._h, C.byref(s)))
    return int(s.device_bytes)


def _calls():
    """the issue's sequence: (name, what to call on a handle)"""
    rng = np.random.default_rng(5)
    d1 = rng.uniform(-300.0, 300.0, (1, A))
    d5 = rng.uniform(-300.0, 300.0, (5, A))
    psi5 = rng.uniform(-1.0, 1.0, (5, A))
    g5 = rng.uniform(0.5, 1.5, (5, A)).astype(np.float32)
    row0 = rng.integers(0, T - 5 + 1, (3, NCO)).astype(np.int32)
    p1, p5 = PR.random_proj(A, 6), PR.random_proj(A, 7)
    return [("beam 1 x tscr 4", lambda h: h.beamform(0, S, d1, tscr=4)),
            ("corr int_rows 8", lambda h: h.correlate(0, S, 8)),
            ("proj 1 x tscr 4", lambda h: h.beamform_proj(0, S, d1, p1, tscr=4)),
            ("beam 5 x tscr 1", lambda h: h.beamform(1, S, d5, psi5, g5, tscr=1)),
            ("corr int_rows 2", lambda h: h.correlate(1, S, 2)),
            ("proj 5 x tscr 1", lambda h: h.beamform_proj(1, S, d5, p5, psi5, g5, tscr=1)),
            ("gated raw", lambda h: h.correlate_gated(0, S, row0, 5)),
            ("gated kur", lambda h: h.correlate_gated(1, S, row0, 5))]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_growth_keeps_nothing_stale():
    lp = libpb()
    calls = _calls()
    with _fed(lp) as h:
        got = [f(h) for _, f in calls]
    assert got[0][0].shape == got[2][0].shape == (1, 4, 4, NCO) and got[3][0].shape == got[5][0].shape == (5, 16, 4, NCO)
    assert got[1][0].shape == (2, 3, 4, NCO) and got[4][0].shape == (8, 3, 4, NCO) and got[6][0].shape == (3, 3, 4, NCO)
    # the seeded bytes hold flagged rows: the excised stream's counts differ from the raw stream's
    assert got[4][1].min() < 2 and got[1][1].min() == 8
    for (name, f), g in zip(calls, got):
        with _fed(lp) as fresh:
            ref = f(fresh)
        for x, y in zip(g, ref):
            assert x.shape == y.shape and x.dtype == y.dtype, name
            assert np.array_equal(_bits(x), _bits(y)), name


@pytest.mark.parametrize("small,large", [(1, 4), (0, 3), (2, 5)], ids=["correlate", "beamform", "beamform_proj"])
def test_device_bytes_follow_the_buffers(small, large):
    lp = libpb()
    calls = _calls()
    with _fed(lp) as h:
        seen = [_device_bytes(lp, h)]
        for k in (small, large, small):
            calls[k][1](h)
            seen.append(_device_bytes(lp, h))
    assert all(b >= a for a, b in zip(seen, seen[1:])), seen       # never lower after a call than before it
    assert seen[1] > seen[0] and seen[2] > seen[1] and seen[3] == seen[2], seen
    with _fed(lp) as fresh:
        calls[large][1](fresh)
        assert _device_bytes(lp, fresh) == seen[2]


def test_timers():
    lp = libpb()
    calls = _calls()
    with _fed(lp) as h:
        assert h.correlate_timers() == (0.0, 0.0) and h.beamform_timers() == (0.0, 0.0, 0.0)
        assert h.beamform_proj_timers() == (0.0, 0.0, 0.0)
        calls[1][1](h)
        assert h.beamform_timers() == (0.0, 0.0, 0.0)
        calls[0][1](h)
        assert h.beamform_proj_timers() == (0.0, 0.0, 0.0)          # a plain call leaves the projecting call's alone
        calls[2][1](h)
        ct, bt, pt = h.correlate_timers(), h.beamform_timers(), h.beamform_proj_timers()
    assert len(ct) == 2 and len(bt) == 3 and len(pt) == 3
    assert all(np.isfinite(v) and v >= 0 for v in ct + bt + pt), (ct, bt, pt)
    assert ct[0] > 0 and bt[1] > 0 and pt[1] > 0, (ct, bt, pt)      # the kernel stages


def test_which_refusal_wins():
    lp = libpb()
    d = np.zeros((1, A))
    with _handle(lp) as h:                                           # nothing processed on the set
        with pytest.raises(ValueError, match="tscr and nout"):
            h.beamform(0, S, d, tscr=0)
        with pytest.raises(lp.PbError, match="no pb_process"):
            h.correlate(0, S, 3)
        with pytest.raises(lp.PbError, match="no pb_process"):
            h.beamform(0, S, d, tscr=4)
    with _handle(lp, coherence=False) as h:
        with pytest.raises(ValueError, match="coherence"):
            h.beamform(7, 0, d, tscr=0)
        with pytest.raises(ValueError, match="coherence"):
            h.correlate(7, 0, 3)
        with pytest.raises(ValueError, match="coherence"):
            h.correlate_gated(7, 0, np.zeros((1, NCO), np.int32), 0)


def test_lifetime():
    lp = libpb()
    h = _fed(lp)
    for _, f in _calls():
        f(h)
    h.close()
    _handle(lp).close()                                              # used none of them
    lp.PbImager(3, 16).close()                                       # never got set_vis
    with _fed(lp) as h:                                              # and the device still serves a new handle
        v, u = h.correlate(0, S, T)
    assert np.isfinite(v.view(np.float32)).all() and int(u.min()) == T
