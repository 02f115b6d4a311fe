"""The argument handling of the search's Python driver (Searcher.run / peaks / push / push_plane, GulpSearch(gulp=N).feed /
feed_plane, and the stages' refusals while they are off): what a host array or a device address + nsamp turns into, and
which exception says what.  Every criterion is equality or an exception's type and text.

Geometry: the smallest that reaches every path -- 64 channels, blocks of at most 512 samples, three trial DMs (0, 10,
20: a largest delay of a few samples), boxcars up to 4; a second searcher with set_pol() on for the 4-row blocks."""
import importlib

import numpy as np
import pytest

from helpers import libpb
from search_rfi_ref import pack

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")

NCHAN, MAXS, NS = 64, 512, 200
GEOM = dict(nchan=NCHAN, max_samples=MAXS, dm_min=0, dm_max=20, dm_step=10, boxcar_max=4, zap=())


def values(seed, nsamp, nbit, nrow=NCHAN):
    return np.random.default_rng(seed).integers(0, 1 << nbit, (nsamp, nrow)).astype(np.uint8)


def to_device(host):
    """a host array's bytes on the GPU: (the tensor that owns them, their device address)"""
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).ravel().copy()).cuda()
    torch.cuda.synchronize()                               # the search's stream waits for no other
    return dev, dev.data_ptr()


def point_set(pk):
    return (pk["tout"], pk["total"], sorted(zip(pk["dmi"].tolist(), pk["t"].tolist(), pk["snr"].view(np.uint32).tolist(),
                                                pk["width_log2"].tolist())))


@pytest.fixture(scope="module")
def s():
    with search.Searcher(**GEOM) as s:
        assert s.max_delay < 64 and s.ndm == 3
        s.set_gulp(8)
        yield s


@pytest.fixture(scope="module")
def s4():
    with search.Searcher(**GEOM) as s4:
        s4.set_pol(off_len=16, guard=2, rm=(-10.0, 1.0, 21), max_cands=2)
        yield s4


@pytest.fixture
def gulp(s):
    """a GulpSearch(gulp=400) on the plain searcher, its accumulated block empty"""
    s.gulp_advance(0)
    g = search.GulpSearch(s, threshold=50.0, gulp=400)
    yield g
    s.gulp_advance(0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. nsamp inferred from a host array; a device address needs it

@pytest.mark.parametrize("nbit", [8, 4, 2])
def test_searcher_infers_nsamp_from_a_host_array(s, nbit):
    codes = pack(values(10 + nbit, NS, nbit), nbit)
    assert codes.size == NS * NCHAN * nbit // 8
    assert s.run(codes, nbit=nbit)["tout"] == NS - s.max_delay
    assert s.peaks(codes, 3.0, nbit=nbit)["tout"] == NS - s.max_delay
    assert s.push(codes, nbit=nbit) == NS and s.push(codes.reshape(NS, -1), nbit=nbit) == 2 * NS
    s.gulp_advance(0)
    assert s.push_plane(np.ones((NS, NCHAN), np.float32)) == NS and s.push_plane(np.ones(3 * NCHAN, np.float32)) == NS + 3
    s.gulp_advance(0)


def test_searcher_infers_a_quarter_of_the_rows_with_polarisation_on(s4):
    rows = values(14, 4 * NS, 8)                            # [nsamp][4][nchan] as 4 nsamp rows of nchan
    assert s4.run(rows)["tout"] == NS - s4.max_delay
    assert s4.peaks(rows, 3.0)["tout"] == NS - s4.max_delay
    assert s4.pol_fetch(3).shape == (NCHAN, NS)


def test_searcher_device_ptr_needs_nsamp(s, s4):
    keep, ptr = to_device(values(15, NS, 8))
    for call in (lambda: s.run(None, device_ptr=ptr), lambda: s.peaks(None, 3.0, device_ptr=ptr), lambda: s.push(device_ptr=ptr),
                 lambda: s.push_plane(device_ptr=ptr), lambda: s4.run(None, device_ptr=ptr), lambda: s4.peaks(None, 3.0, device_ptr=ptr)):
        with pytest.raises(ValueError, match="device_ptr needs nsamp"):
            call()
    assert s.gulp_fill() == 0


@pytest.mark.parametrize("nbit", [8, 4, 2])
def test_gulp_search_infers_nsamp_from_a_host_array(s, gulp, nbit):
    codes = pack(values(20 + nbit, 100, nbit), nbit)
    assert gulp.feed(codes, nbit=nbit) == [] and s.gulp_fill() == 100
    assert gulp.feed(codes.reshape(100, -1)[:37], nbit=nbit) == [] and s.gulp_fill() == 137
    assert gulp.feed_plane(np.ones((50, NCHAN), np.float32)) == [] and s.gulp_fill() == 187
    assert (gulp.since, gulp.fill) == (187, 187)


def test_gulp_search_device_ptr_needs_nsamp(s, gulp):
    keep, ptr = to_device(values(25, 100, 8))
    for call in (lambda: gulp.feed(device_ptr=ptr), lambda: gulp.feed(nbit=2, device_ptr=ptr), lambda: gulp.feed_plane(device_ptr=ptr)):
        with pytest.raises(ValueError, match="device_ptr needs nsamp"):
            call()
    assert s.gulp_fill() == 0 and gulp.since == 0
    assert gulp.feed(device_ptr=ptr, nsamp=100) == [] and gulp.feed_plane(device_ptr=ptr, nsamp=25) == [] and s.gulp_fill() == 125


# ---------------------------------------------------------------------------------------------------------------------
# 2. a host array shorter than an explicit nsamp; run() and peaks() go by the array

@pytest.mark.parametrize("nbit", [8, 4, 2])
def test_short_host_arrays_are_refused(s, gulp, nbit):
    codes = pack(values(30 + nbit, 100, nbit), nbit)
    plane = np.ones(100 * NCHAN, np.float32)
    for call in (lambda: s.push(codes[:-1], nbit=nbit, nsamp=100), lambda: s.push_plane(plane[:-1], nsamp=100),
                 lambda: gulp.feed(codes[:-1], nbit=nbit, nsamp=100), lambda: gulp.feed_plane(plane[:-1], nsamp=100)):
        with pytest.raises(ValueError, match="fewer than nsamp"):
            call()
    assert s.gulp_fill() == 0 and gulp.since == 0
    # an array longer than nsamp samples is taken up to nsamp
    assert s.push(codes, nbit=nbit, nsamp=99) == 99 and s.push_plane(plane, nsamp=98) == 197
    s.gulp_advance(0)
    assert gulp.feed(codes, nbit=nbit, nsamp=97) == [] and gulp.feed_plane(plane, nsamp=96) == [] and s.gulp_fill() == 193


def test_run_and_peaks_go_by_the_host_array_whatever_nsamp_says(s, s4):
    x = values(35, NS, 8)
    for nsamp in (7, NS - 50, NS + 50):
        assert s.run(x, nsamp=nsamp)["tout"] == NS - s.max_delay
        assert s.peaks(x, 3.0, nsamp=nsamp)["tout"] == NS - s.max_delay
    rows = values(36, 4 * NS, 8)
    assert s4.run(rows, nsamp=7)["tout"] == NS - s4.max_delay and s4.peaks(rows, 3.0, nsamp=7)["tout"] == NS - s4.max_delay


# ---------------------------------------------------------------------------------------------------------------------
# 3. a bit depth that is none of 8, 4, 2 (the types and texts are the ones these calls gave before the driver was split)

def test_bad_nbit(s):
    PbError = libpb().PbError
    x = values(40, NS, 8)
    for nbit in (3, 16):
        with pytest.raises(Exception) as e:
            s.run(x, nbit=nbit)
        print("run", nbit, type(e.value).__name__, e.value)
        if nbit == 3:
            assert type(e.value) is PbError and str(e.value) == "pb_search_run failed (-22): pb_search_run: block too long or bad nbit"
        else:
            assert type(e.value) is ValueError
            assert str(e.value) == "block shorter than the largest dispersion delay (%d samples)" % s.max_delay
        with pytest.raises(Exception) as e:
            s.peaks(x, 3.0, nbit=nbit)
        print("peaks", nbit, type(e.value).__name__, e.value)
        assert type(e.value) is PbError and str(e.value) == "pb_search_peaks failed (-22): pb_search_run: block too long or bad nbit"
        with pytest.raises(Exception) as e:
            s.push(x, nbit=nbit)
        print("push", nbit, type(e.value).__name__, e.value)
        assert type(e.value) is PbError and str(e.value) == "pb_search_push failed (-22): pb_search_push: nbit must be 8, 4 or 2"
    assert s.gulp_fill() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. a stage that is off refuses, before its set_* call and after set_*(max = 0)

SET = dict(_cut=("set_cutouts", dict(nsub=8, nt=8, ndmrow=2, max_cands=2), dict(max_cands=0)),
           _pol=("set_pol", dict(off_len=16, guard=2, rm=(-10.0, 1.0, 21), max_cands=2), dict(max_cands=0)),
           _ref=("set_refine", dict(nstep=4, half_window=16, wmax=8, max_cands=2), dict(max_cands=0)),
           _sub=("set_subbands", dict(nsb=2, max_points=64), dict(nsb=0)),
           _gi=("set_giants", dict(max_giants=64), dict(max_giants=0)))
CALLS = [("_cut", "cutouts", (0, 10, 1)), ("_pol", "pol", (0, 10, 1)), ("_ref", "refine_raw", (10, 1, 0.0, 1.0)),
         ("_ref", "refine", (0, 10, 0)), ("_sub", "subbands", (5.0,)), ("_sub", "subband_dm", (0,)), ("_gi", "giants", (5.0,))]


def test_a_stage_that_is_off_refuses():
    PbError = libpb().PbError
    with search.Searcher(**GEOM) as s:
        s.run(values(50, NS, 8))
        for attr, name, args in CALLS:
            setter, on, off = SET[attr]
            assert getattr(s, attr) is None
            with pytest.raises(PbError, match="not switched on"):
                getattr(s, name)(*args)
            getattr(s, setter)(**on)
            assert getattr(s, attr) is not None
            getattr(s, setter)(**off)
            assert getattr(s, attr) is None
            with pytest.raises(PbError, match="not switched on"):
                getattr(s, name)(*args)
        # pol_cutouts needs both of its stages
        need = r"needs set_cutouts\(\) and set_pol\(\)"
        with pytest.raises(PbError, match=need):
            s.pol_cutouts(0, 10, 1)
        for first, second in (("_cut", "_pol"), ("_pol", "_cut")):
            getattr(s, SET[first][0])(**SET[first][1])
            assert getattr(s, first) is not None and getattr(s, second) is None
            with pytest.raises(PbError, match=need):
                s.pol_cutouts(0, 10, 1)
            getattr(s, SET[second][0])(**SET[second][1])
            getattr(s, SET[first][0])(**SET[first][2])
            assert getattr(s, first) is None and getattr(s, second) is not None
            with pytest.raises(PbError, match=need):
                s.pol_cutouts(0, 10, 1)
            getattr(s, SET[second][0])(**SET[second][2])
            assert s._cut is None and s._pol is None


# ---------------------------------------------------------------------------------------------------------------------
# 5. the same bytes from the host and from the device

@pytest.mark.parametrize("nbit", [8, 4, 2])
def test_host_and_device_input_give_the_same_planes_and_points(s, nbit):
    codes = pack(values(60 + nbit, NS, nbit), nbit)
    keep, ptr = to_device(codes)
    host, dev = s.run(codes, nbit=nbit, want_series=True), s.run(None, nbit=nbit, want_series=True, device_ptr=ptr, nsamp=NS)
    assert host["tout"] == dev["tout"] == NS - s.max_delay
    for k in ("snr", "width_log2", "stats", "series"):
        assert host[k].dtype == dev[k].dtype and np.array_equal(host[k], dev[k]), k
    ph, pd = s.peaks(codes, 2.0, nbit=nbit), s.peaks(None, 2.0, nbit=nbit, device_ptr=ptr, nsamp=NS)
    assert ph["total"] > 0 and point_set(ph) == point_set(pd)


def test_host_and_device_input_agree_with_polarisation_on(s4):
    rows = values(70, 4 * NS, 8)
    keep, ptr = to_device(rows)
    host, dev = s4.run(rows), s4.run(None, device_ptr=ptr, nsamp=NS)
    for k in ("snr", "width_log2", "stats"):
        assert np.array_equal(host[k], dev[k]), k
    ph, pd = s4.peaks(rows, 2.0), s4.peaks(None, 2.0, device_ptr=ptr, nsamp=NS)
    assert ph["total"] > 0 and point_set(ph) == point_set(pd)
