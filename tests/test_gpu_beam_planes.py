"""pb_beam_planes on the GPU against the CPU restatement of its definition (tests/beam_plane_ref.py) applied to what
pb_beamform / pb_beamform_proj return for the same arguments -- planes and level_out bit for bit, over antenna counts,
beam counts around the beam kernel's tile, windows of 1, 3, 8 and all rows, both streams, output lengths around the
32-sample chunk, samples and whole columns without a valid row, with and without a level handed in, random and dispersed
shifts; then the device copy against the host copy through the search's quantiser, side effects, refusals, timers, and the
channel order of the planes against the filterbank's own."""
import importlib

import numpy as np
import pytest

import beam_plane_ref as PR
from helpers import libpb, make_input

pytestmark = pytest.mark.gpu

NFFT, NCO = 12500, 4096
F = np.float32


def _handle(lp, A, R, nseg, rfi_mode, **kw):
    return lp.PbHandle(nant=A, nbit=8, npol=2, rfi_mode=rfi_mode, rows_per_seg=R, max_seg=nseg, coherence=True, **kw)


def _submit(h, data):
    """data u8 [A][nseg][2][n]"""
    for a in range(data.shape[0]):
        for s in range(data.shape[1]):
            h.submit_planar(a, s, data[a, s, 0], data[a, s, 1])


_inputs = {}


def _data(A, R, nseg):
    """seeded inputs with RFI bursts, a fully flagged row and a dropped frame (helpers.make_input), made once"""
    if (A, R, nseg) not in _inputs:
        _inputs[A, R, nseg] = np.stack([make_input(200 + 7 * a + R, R, nseg) for a in range(A)])
    return _inputs[A, R, nseg]


def _beams(A, seed):
    """five beams: fractional delays, a psi, gains with zeros and a one-hot row"""
    rng = np.random.default_rng(seed)
    delay = rng.uniform(-20000.0, 20000.0, (5, A))
    psi = rng.uniform(-2.0, 2.0, (5, A))
    gain = rng.uniform(0.5, 1.5, (5, A)).astype(F)
    gain[1] = 0
    gain[1, 1 % A] = 1
    gain[3, A - 1] = 0 if A > 1 else 1
    return delay, psi, gain


def _level_in(L, seed):
    """a level to hand in: the planes' own times a factor per (beam, channel), with zeros"""
    rng = np.random.default_rng(seed)
    lev = (L * rng.uniform(0.5, 2.0, L.shape).astype(F)).astype(F)
    lev[0, :7] = 0
    return lev


def _same(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype == F, what
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, (what, len(bad), bad[:4])


def _check(h, st, nseg, delay, psi, gain, shift, tscr, nout, seed, proj=None):
    """one set of arguments: the planes and level_out without and with a level handed in, against the restatement on
    h.beamform's (h.beamform_proj's) outputs.  -> rows_used"""
    if proj is None:
        beams, used = h.beamform(st, nseg, delay, psi, gain, shift, tscr, nout)
    else:
        beams, used = h.beamform_proj(st, nseg, delay, proj, psi, gain, shift, tscr, nout)
    ref, L = PR.planes(beams, used, tscr)
    planes, ptr, lev = h.beam_planes(st, nseg, delay, psi, gain, proj, shift, tscr, nout)
    what = (st, delay.shape, tscr, nout)
    _same(planes, ref, what)
    _same(lev, L, what)
    assert ptr % 16 == 0
    level = _level_in(L, seed)
    ref2, _ = PR.planes(beams, used, tscr, level)
    planes, _, lev = h.beam_planes(st, nseg, delay, psi, gain, proj, shift, tscr, nout, level=level)
    _same(planes, ref2, what + ("level_in",))
    _same(lev, L, what + ("level_in",))
    assert np.all(planes[0, :, :7].view(np.uint32) == 0) and np.isfinite(planes).all()
    return used


@pytest.mark.parametrize("A,R", [(1, 8), (4, 16), (8, 16)])
def test_bit_exact(A, R):
    """R = 16: 48 rows; tscr = 1 gives 48 output samples, a whole chunk and a short one"""
    lp = libpb()
    corr = importlib.import_module("vlite-fast_amd.correlate")
    nseg = 3
    T = nseg * R
    data = _data(A, R, nseg)
    delay, psi, gain = _beams(A, 10 * A + R)
    rng = np.random.default_rng(A)
    random_shift = rng.integers(0, 6, NCO).astype(np.int32)
    dm_shift = corr.dm_row0(0.12 if R == 8 else 0.25, 0, T)
    variants = {1: (None, None, None), 4: (psi, gain, random_shift), 5: (psi, gain, dm_shift)}
    below = False
    with _handle(lp, A, R, nseg, 2) as h:
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            for nbeam, (ps, ga, sh) in variants.items():
                cut = lambda v: None if v is None else v[:nbeam]
                for tscr in (1, 3, 8, T):
                    s = None if tscr == T else sh
                    used = _check(h, st, nseg, delay[:nbeam], cut(ps), cut(ga), s, tscr, None, 100 * st + nbeam + tscr)
                    if st == 0:
                        assert np.all(used == tscr)
                    else:
                        below = below or used.min() < tscr
            if R == 16:
                for nout in (33, 32, 1):                     # around the chunk of 32 output samples
                    _check(h, st, nseg, delay[:2], None, None, None, 1, nout, nout)
        # the inputs hold a fully flagged row: rows_used of the excised stream falls below tscr
        assert below


def test_sample_and_column_without_rows():
    """the excised stream's fully flagged row, seen by a one-hot beam on its antenna at tscr = 1: a sample with used == 0
    among samples with rows, and, with shifts that put output sample 0 on that row and nout = 1, a whole (beam, channel)
    column with used == 0, whose level is 0 and whose plane is +0.0f"""
    lp = libpb()
    A, R, nseg = 3, 8, 3
    data = _data(A, R, nseg)
    with _handle(lp, A, R, nseg, 2) as h:
        _submit(h, data)
        h.process(nseg)
        delay, gain = np.zeros((2, A)), np.array([[1, 0, 0], [1, 1, 1]], F)
        used = _check(h, 1, nseg, delay, None, gain, None, 1, None, 5)
        rows = np.nonzero((used[0] == 0).all(axis=1))[0]
        assert rows.size > 0 and used[0].max() == 1            # make_input's flagged row, among rows that count
        planes, _, lev = h.beam_planes(1, nseg, delay, None, gain, None, None, 1)
        assert np.all(planes[0, rows[0]].view(np.uint32) == 0) and np.all(lev[0] > 0)
        shift = np.full(NCO, rows[0], np.int32)
        used = _check(h, 1, nseg, delay, None, gain, shift, 1, 1, 6)
        assert used.max() == 0
        planes, _, lev = h.beam_planes(1, nseg, delay, None, gain, None, shift, 1, 1)
        assert np.all(lev == 0) and np.all(planes.view(np.uint32) == 0)


def test_bit_exact_projecting():
    """three antennas, random finite matrices: against pb_beamform_proj's outputs"""
    lp = libpb()
    A, R, nseg = 3, 16, 3
    data = _data(A, R, nseg)
    delay, psi, gain = _beams(A, 77)
    rng = np.random.default_rng(78)
    proj = (rng.normal(0, 1, (2, NCO, A, A)) + 1j * rng.normal(0, 1, (2, NCO, A, A))).astype(np.complex64)
    shift = rng.integers(0, 6, NCO).astype(np.int32)
    below = False
    with _handle(lp, A, R, nseg, 2) as h:
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            for nbeam, tscr in ((1, 1), (4, 3), (5, 8)):
                used = _check(h, st, nseg, delay[:nbeam], psi[:nbeam], gain[:nbeam], shift, tscr, None, nbeam, proj=proj)
                below = below or (st == 1 and used.min() < tscr)
        assert below
        # the plain call's state is its own: its planes after the projecting call are what they were
        _check(h, 1, nseg, delay[:2], None, None, None, 3, None, 9)


def test_device_and_host_copies_agree():
    """to_host=False and Searcher.push_plane(device_ptr=...) per beam fill the gulp block byte for byte as
    push_plane(plane=host_planes[b]) does; every beam's block is 16-byte aligned"""
    lp = libpb()
    search = importlib.import_module("vlite-fast_amd.search")
    A, R, nseg, tscr, nbeam = 2, 16, 3, 1, 3
    data = _data(A, R, nseg)
    delay, psi, gain = _beams(A, 31)
    nout = nseg * R // tscr
    with _handle(lp, A, R, nseg, 2) as h, \
            search.Searcher(nchan=NCO, max_samples=256, dm_min=0, dm_max=6, dm_step=2, boxcar_max=4) as s:
        s.set_gulp(8)
        _submit(h, data)
        h.process(nseg)
        host, _, lev_host = h.beam_planes(1, nseg, delay[:nbeam], psi[:nbeam], gain[:nbeam], tscr=tscr)
        none, ptr, lev_dev = h.beam_planes(1, nseg, delay[:nbeam], psi[:nbeam], gain[:nbeam], tscr=tscr, to_host=False)
        assert none is None and host.shape == (nbeam, nout, NCO) and np.array_equal(lev_host, lev_dev)
        for b in range(nbeam):
            at = ptr + b * nout * NCO * 4
            assert at % 16 == 0
            assert s.push_plane(device_ptr=at, nsamp=nout) == nout
            from_dev = s.gulp_fetch()
            s.gulp_advance(0)
            assert s.push_plane(plane=host[b]) == nout
            from_host = s.gulp_fetch()
            s.gulp_advance(0)
            assert from_dev.shape == (NCO, nout) and np.array_equal(from_dev, from_host), b
            assert len(np.unique(from_dev)) > 50


def _device_bytes(lp, h):
    s = lp.PbSizes()
    h._chk(h._L.pb_query(h._h, s))
    return int(s.device_bytes)


def test_no_side_effects_and_device_bytes():
    lp = libpb()
    A, R, nseg, tscr = 2, 8, 3, 3
    data = _data(A, R, nseg)
    delay, psi, gain = _beams(A, 41)
    delay, psi, gain = delay[:2], psi[:2], gain[:2]
    sizes = []
    for _ in range(2):                                       # the second handle: device_bytes across destroy and create
        with _handle(lp, A, R, nseg, 2, keep_ave=True) as h:
            _submit(h, data)
            h.process(nseg)
            fetched = [h.fetch(a, 0, nseg, ave=True) for a in range(A)]
            beams, used = h.beamform(1, nseg, delay, psi, gain, None, tscr)
            timers = h.beamform_timers()
            before = _device_bytes(lp, h)
            planes, _, lev = h.beam_planes(1, nseg, delay, psi, gain, None, None, tscr)
            after = _device_bytes(lp, h)
            nout = planes.shape[1]
            # the planes, two levels' worth at most, a chunk sum and a count per (beam, chunk, channel)
            assert after - before >= planes.nbytes + lev.nbytes + 2 * NCO * (8 + 4)
            assert after - before <= planes.nbytes + 2 * lev.nbytes + 2 * NCO * (8 + 4) * ((nout + 31) // 32)
            h.beam_planes(1, nseg, delay, psi, gain, None, None, tscr, level=lev)
            assert _device_bytes(lp, h) == after + lev.nbytes                    # level_in's buffer, once
            h.beam_planes(1, nseg, delay, psi, gain, None, None, tscr, level=lev)
            assert _device_bytes(lp, h) == after + lev.nbytes
            assert h.beamform_timers() == timers
            again = [h.fetch(a, 0, nseg, ave=True) for a in range(A)]
            for a in range(A):
                for k in ("raw", "kur", "ave_raw", "ave_kur"):
                    assert fetched[a][k].tobytes() == again[a][k].tobytes(), (a, k)
            b2, u2 = h.beamform(1, nseg, delay, psi, gain, None, tscr)
            assert b2.tobytes() == beams.tobytes() and np.array_equal(u2, used)
            t = h.beam_planes_timers()
            print("beam_planes timers (ms):", t)
            assert len(t) == 4 and all(np.isfinite(x) and x >= 0 for x in t) and t[1] > 0 and t[2] > 0
            sizes.append((before, after))
    assert sizes[0] == sizes[1]


def test_refusals():
    lp = libpb()
    R, nseg = 8, 2
    data = make_input(1, R, nseg)[None]
    d1 = np.zeros((1, 1))
    with lp.PbHandle(nant=1, npol=2, rfi_mode=2, rows_per_seg=R, max_seg=nseg) as h:      # coherence = 0
        _submit(h, data)
        h.process(nseg)
        with pytest.raises(ValueError, match="pb_beam_planes: .*coherence"):
            h.beam_planes(0, nseg, d1)
    with _handle(lp, 1, R, nseg, 2) as h:
        with pytest.raises(lp.PbError, match="pb_beam_planes: no pb_process"):
            h.beam_planes(0, nseg, d1)
        _submit(h, data)
        h.process(nseg)
        assert h.beam_planes_timers() == (0.0, 0.0, 0.0, 0.0)
        with pytest.raises(ValueError, match="pb_beam_planes: a window"):                  # inherited, under the new name
            h.beam_planes(0, nseg, d1, tscr=3, nout=nseg * R // 3 + 1)
        with pytest.raises(ValueError, match="pb_beam_planes: a delay is not finite"):
            h.beam_planes(0, nseg, np.full((1, 1), np.nan))
        for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-30):
            level = np.ones((1, NCO), F)
            level[0, 4095] = bad
            with pytest.raises(ValueError, match="pb_beam_planes: a level_in value is not finite or is negative"):
                h.beam_planes(0, nseg, d1, level=level)
        proj = np.zeros((2, NCO, 1, 1), np.complex64)
        proj[1, 17, 0, 0] = np.inf
        with pytest.raises(ValueError, match="pb_beam_planes: a proj value is not finite"):
            h.beam_planes(0, nseg, d1, proj=proj)
        level = np.zeros((1, NCO), F)                          # zeros and -0.0 are taken
        level[0, 1] = -0.0
        planes, ptr, lev = h.beam_planes(0, nseg, d1, level=level)
        assert np.all(planes.view(np.uint32) == 0) and np.all(lev > 0) and ptr
        # every output may be left out
        assert h._L.pb_beam_planes(h._h, 0, nseg, 1, d1.ctypes.data_as(h._L.pb_beam_planes.argtypes[4]), None, None, None,
                                   None, 1, 1, None, None, None, None) == 0


def test_channel_order_is_the_filterbanks():
    """a carrier at FFT bin 2155 + c0 in one antenna's voltages: the strongest channel of that antenna's one-hot beam plane
    is the strongest channel of a filterbank handle's own fp32 plane (npol = 1, keep_ave) on the same bytes, and it is c0:
    the tool may describe the beam planes with the filterbank's fch1 and foff.  The filterbank divides by a running
    bandpass, which would take a steady carrier out: its handle sees the noise alone first, then the batch with the carrier,
    and the plane's largest value over time is compared."""
    lp = libpb()
    A, R, nseg, tscr, c0 = 2, 8, 2, 8, 1234
    data = np.stack([make_input(900 + a, R, nseg, rfi=False, dropped=False) for a in range(A)])
    n = np.arange(R * NFFT, dtype=np.float64)
    tone = 12.0 * np.cos(2 * np.pi * (2155 + c0) * n / NFFT)
    noise = data[1:].copy()
    data[1] = np.clip(np.rint(data[1].astype(np.float64) + tone), 0, 255).astype(np.uint8)
    with _handle(lp, A, R, nseg, 0) as h:
        _submit(h, data)
        h.process(nseg)
        planes, _, _ = h.beam_planes(0, nseg, np.zeros((1, A)), gain=np.array([[0, 1]], F), tscr=tscr,
                                     level=np.full((1, NCO), 1.0, F))
    with lp.PbHandle(nant=1, nbit=8, npol=1, rfi_mode=0, rows_per_seg=R, max_seg=nseg, keep_ave=True) as f:
        for batch in (noise, data[1:]):
            _submit(f, batch)
            f.process(nseg)
            ave = f.fetch(0, 0, nseg, ave=True)["ave_raw"].reshape(nseg * R // 8, NCO)
    beam_c, fb_c = int(planes[0].max(axis=0).argmax()), int(ave.max(axis=0).argmax())
    print("carrier at channel %d: beam plane %d, filterbank plane %d" % (c0, beam_c, fb_c))
    assert beam_c == fb_c == c0
