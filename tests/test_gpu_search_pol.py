"""The polarisation stage of the search (pb_search_set_pol / pb_search_pol / pb_search_pol_cutouts, Searcher.set_pol / pol /
pol_cutouts, GulpSearch(pol=...)) on the GPU against the NumPy restatement tests/search_pol_ref.py: planes, images and
spectra exactly, the RM synthesis to the rounding of double worked out below.
Geometry: 96 channels (one and a half 64-channel tiles) from 384 MHz down in steps of 0.5 MHz -- 48 MHz, 0.19 m^2 of
lambda^2 --, 781.25 us samples, trial DMs 0..60 in steps of 2, channels 0..2 and 90..95 zapped, boxcars up to 64; blocks of
2500 and 2501 samples (neither a multiple of 64; 2501 not one of 4)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import search_pol_ref as R

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")
libpb = importlib.import_module("vlite-fast_amd.libpb")

NCHAN, FCH1, FOFF, TSAMP = 96, 384.0, -0.5, 781.25e-6
ZAP = ((0, 3), (90, 96))
DMS = np.arange(0.0, 61.0, 2.0)
DELAY = R.delays(DMS, FCH1, FOFF, NCHAN, TSAMP)
ZAPPED = R.zap_mask(NCHAN, ZAP)
LAM2 = R.lambda2(FCH1, FOFF, NCHAN)
MAXD = int(DELAY[:, ~ZAPPED].max())
NACT = int((~ZAPPED).sum())
KW = dict(nchan=NCHAN, fch1=FCH1, foff=FOFF, tsamp=TSAMP, dm_min=0.0, dm_max=60.0, dm_step=2.0, boxcar_max=64, zap=ZAP)
EINVAL = -22
SPEC = ("on", "non", "off", "noff")


def _random_block(seed, nsamp):
    """random codes with runs of 0 and of 255 in every product (the I-code rule's corners among them)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (nsamp, 4, NCHAN)).astype(np.uint8)
    x[100:140] = 255
    x[300:330] = 0
    x[500:520, 0], x[500:520, 1] = 255, 254
    x[600:620, 0], x[600:620, 1] = 0, 1
    x[:, :, 70][700:900] = 255
    return x


def _noise_block(seed, nsamp):
    return R.quantise8(np.random.default_rng(seed).standard_normal((nsamp, 4, NCHAN)))


@pytest.mark.parametrize("nsamp", [2500, 2501])
def test_planes_equal_the_restatement(nsamp):
    import torch
    x = _random_block(11, nsamp)
    p4, xt = R.planes(x)
    with search.Searcher(max_samples=2501, **KW) as s:
        assert s.max_delay == MAXD == 604 and s.ndm == 31
        s.set_pol(max_cands=4)
        r = s.run(x)
        assert r["tout"] == nsamp - MAXD
        for k in range(4):
            assert np.array_equal(s.pol_fetch(k), p4[k]), k
        assert np.array_equal(s.fetch_clean(), xt)
        # a device block at an odd address goes byte by byte, one at a multiple of 4 in dwords: the same planes
        for shift in (1, 4):
            d = torch.zeros(x.size + 8, dtype=torch.uint8, device="cuda")
            d[shift:shift + x.size] = torch.from_numpy(x.ravel()).cuda()
            torch.cuda.synchronize()
            r2 = s.run(None, device_ptr=d.data_ptr() + shift, nsamp=nsamp)
            for k in range(4):
                assert np.array_equal(s.pol_fetch(k), p4[k]), (shift, k)
            assert np.array_equal(s.fetch_clean(), xt) and np.array_equal(r2["snr"], r["snr"])
        assert s.pol_timers()["transpose"] > 0


@pytest.mark.parametrize("rfi", [False, True])
def test_the_search_itself_is_untouched(rfi):
    x = R.simulate(21, 2501, NCHAN, FCH1, FOFF, DELAY[15], [dict(t=900, w=8, amp=1.5, p=0.5, rm=10.0, chi0=0.0)])
    x[1500:1503] = np.minimum(x[1500:1503].astype(int) + 60, 255).astype(np.uint8)        # a broadband burst
    x[200:260, :, 40] = 250                                                                # and a channel's outliers
    p4, xt = R.planes(x)
    out = []
    for pol in (True, False):
        with search.Searcher(max_samples=2501, **KW) as s:
            if rfi:
                s.set_rfi()
            if pol:
                s.set_pol()
            r = s.run(x if pol else np.ascontiguousarray(xt.T), want_series=True)
            out.append((r, s.fetch_clean(), s.rfi_info(), [s.pol_fetch(k) for k in range(4)] if pol else None))
    (a, xa, ia, pa), (b, xb, ib, _) = out
    for k in ("snr", "width_log2", "series", "stats"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(xa, xb) and ia["n_narrow"] == ib["n_narrow"] and ia["n_broad_samples"] == ib["n_broad_samples"]
    assert (ia["n_narrow"] > 0 and ia["n_broad_samples"] > 0 and not np.array_equal(xa, xt)) if rfi else np.array_equal(xa, xt)
    for k in range(4):                                  # cleaning changes xt only: the product planes are what the block held
        assert np.array_equal(pa[k], p4[k]), k
    assert a["snr"][15].max() > 10                      # the pulse is there


def test_images_equal_cutouts_of_each_plane():
    nsamp, nsub, nt = 2501, 8, 16
    x = _random_block(31, nsamp)
    p4, _ = R.planes(x)
    tout = nsamp - MAXD
    # the first request's bins run off the block's start, the last one's off its end (delays up to 604 at DM 60)
    reqs = [(30, 3, 8), (15, 700, 1), (7, 701, 2), (0, 1000, 8), (30, tout - 1, 8), (30, tout - 1, 1), (0, 0, 2)]
    with search.Searcher(max_samples=nsamp, **KW) as s, search.Searcher(max_samples=nsamp, **KW) as s1:
        s.set_pol(max_cands=8)
        s.set_cutouts(nsub=nsub, nt=nt, ndmrow=4, max_cands=8)
        s1.set_cutouts(nsub=nsub, nt=nt, ndmrow=4, max_cands=8)
        s.run(x)
        got = s.pol_cutouts(*zip(*reqs))
        assert got["pft"].shape == (len(reqs), 4, nsub, nt) and got["pft"].dtype == np.uint32
        for k in range(4):
            s1.run(np.ascontiguousarray(p4[k].T))
            ref = s1.cutouts(*zip(*reqs))
            assert np.array_equal(got["pft"][:, k], ref["ft"]), k
            assert np.array_equal(got["pft_hits"], ref["ft_hits"]), k
        assert got["pft_hits"][0, :, 0].sum() < NACT * 8 and got["pft_hits"][4, :, -1].sum() < NACT * 8     # bins cut by the block
        assert got["pft_hits"][1].sum() == NACT * nt
        one = s.pol_cutouts(*reqs[2])
        assert np.array_equal(one["pft"][0], got["pft"][2])
        # a change of either set call remakes the buffers
        s.set_cutouts(nsub=4, nt=8, ndmrow=4, max_cands=3)
        s1.set_cutouts(nsub=4, nt=8, ndmrow=4, max_cands=3)
        s1.run(np.ascontiguousarray(p4[3].T))
        assert np.array_equal(s.pol_cutouts(*zip(*reqs[:3]))["pft"][:, 3], s1.cutouts(*zip(*reqs[:3]))["ft"])
        with pytest.raises(libpb.PbError, match="max_cands"):
            s.pol_cutouts(*zip(*reqs[:4]))
        s.set_cutouts(max_cands=0)
        with pytest.raises(libpb.PbError):
            s.pol_cutouts(0, 0, 1)


@pytest.mark.parametrize("nsamp,L,g", [(2500, 64, 8), (2501, 1, 0), (2501, 1024, 1024)])
def test_spectra_are_exact(nsamp, L, g):
    x = _random_block(41, nsamp)
    p4, _ = R.planes(x)
    tout = nsamp - MAXD
    reqs = [(d, t, w) for d in (0, 30) for t in (0, tout - 1, 947) for w in (1, 7, 64)]
    with search.Searcher(max_samples=2501, **KW) as s:
        s.set_pol(off_len=L, guard=g, rm=(-10.0, 1.0, 21), max_cands=len(reqs))
        s.run(x)
        got = s.pol(*zip(*reqs))
    ref = R.pol(p4, DELAY, ZAPPED, LAM2, reqs, L, g, -10.0, 1.0, 21)
    for k in SPEC:
        assert got[k].dtype == np.int32 and np.array_equal(got[k].astype(np.int64), ref[k]), k
    assert np.all(got["on"][:, :, ZAPPED] == 0) and np.all(got["noff"][:, ZAPPED] == 0)
    assert got["non"][:, ~ZAPPED].min() < 64 and got["noff"][0, 3] == L            # windows cut by the block's ends
    assert np.array_equal(got["summary"][:, 0], ref["summary"][:, 0])              # W
    assert np.array_equal(got["kbest"] < 0, ref["kbest"] < 0)
    assert np.array_equal(got["rms"], -10.0 + np.arange(21)) and np.array_equal(got["freqs"], FCH1 + FOFF * np.arange(NCHAN))


def _f_bound(ref, i):
    """The bound on |F_gpu[k] - F_ref[k]| of request i, per trial.  Both sides add the same terms in the same order; term c
    of trial k is (q_c + i u_c) exp(-i theta), theta = (2 phi_k) (lambda2_c - lambda0^2).  On either side theta carries one
    rounding of the product, |theta| 2^-53 (and lambda0^2 -- sequential sums of the same doubles in the same order -- is the
    same number on both); the two libraries' sines and cosines are each within a few ulp of the true ones: together a
    relative error of the term of at most (|theta| + 8) 2^-52 between the sides.  The two products, their sum and the
    accumulation over the nact terms add at most nact 2^-53 of the terms' magnitudes (first order).  So
        |dF[k]| <= (1 / W) sum_c w_c |q_c + i u_c| ((|theta_kc| + 8) 2^-52 + nact 2^-53)."""
    w = ref["w"][i]
    mag = np.where(w, np.hypot(np.where(w, ref["q"][i], 0.0), np.where(w, ref["u"][i], 0.0)), 0.0)
    W = ref["summary"][i, 0]
    bound = (mag[None, :] * ((np.abs(ref["theta"][i]) + 8) * 2.0 ** -52 + NACT * 2.0 ** -53)).sum(axis=1) / W
    assert np.all(bound < 1e-9 * mag.sum() / W)
    return bound, mag.sum() / W


def test_rm_synthesis_of_a_simulated_pulse():
    """RM_FIXTURE of tests/search_pol_ref.py: a pulse at DM 30, t_pk 700, w 8, RM 37, chi0 0.4, p 0.8 on unit-variance noise
    in all four products, quantised with the reference's 8-bit rule; trials -200..200 in steps of 1.  The restatement's
    best two trials are 8.3e-3 apart in relative |F|^2, far above the bound on F, so kbest must agree; its position
    angle at lambda0 lies 0.0086 rad from RM lambda0^2 + chi0."""
    (seed, nsamp), pulse = R.RM_FIXTURE
    x = R.simulate(seed, nsamp, NCHAN, FCH1, FOFF, DELAY[15], [pulse])
    p4, _ = R.planes(x)
    reqs = [(15, 700, 8), (15, 1200, 8), (14, 702, 4)]              # the pulse; noise alone; the pulse, a little off
    with search.Searcher(max_samples=nsamp, **KW) as s:
        s.set_pol(rm=(-200.0, 1.0, 401), max_cands=4)
        pk = s.peaks(x, 8.0)
        got = s.pol(*zip(*reqs))
        tm = s.pol_timers()
    best = int(np.argmax(pk["snr"]))
    assert abs(int(pk["dmi"][best]) - 15) <= 1 and abs(int(pk["t"][best]) - 700) <= 8      # the search finds it in I
    ref = R.pol(p4, DELAY, ZAPPED, LAM2, reqs, 64, 8, -200.0, 1.0, 401)
    for k in SPEC:
        assert np.array_equal(got[k].astype(np.int64), ref[k]), k
    worst = 0.0
    for i in range(len(reqs)):
        bound, scale = _f_bound(ref, i)
        err = np.hypot(got["F"][i, :, 0] - ref["F"][i, :, 0], got["F"][i, :, 1] - ref["F"][i, :, 1])
        worst = max(worst, float((err / bound).max()))
        print("request", i, "largest |dF| / bound", float((err / bound).max()), "largest |dF|", float(err.max()), "scale", scale)
        assert np.all(err <= bound), i
        assert got["kbest"][i] == ref["kbest"][i], i
        rel = bound.max() / scale                                   # the same relative bound for the summary
        gs, rs = got["summary"][i], ref["summary"][i]
        print("request", i, "summary", gs.tolist(), "reference", rs.tolist())
        assert gs[0] == rs[0] == NACT and gs[5] == rs[5]
        assert abs(gs[1] - rs[1]) <= rel * rs[1] and abs(gs[4] - rs[4]) <= rel * scale
        # the means of i and v: sequential sums of nact terms, relative to the mean |i_c| (|v_c|)
        iv = _stokes_iv(p4, reqs[i])
        for j in (0, 1):
            assert abs(gs[2 + j] - rs[2 + j]) <= rel * np.abs(iv[j][ref["w"][i]]).mean(), (i, j)
    print("largest ratio of error to bound", worst)
    assert got["kbest"][0] == 237 and got["summary"][0, 5] == 37.0 and got["rms"][237] == 37.0
    l0 = got["summary"][0, 1]
    ang = 0.5 * np.arctan2(got["F"][0, 237, 1], got["F"][0, 237, 0])
    d = (ang - (37.0 * l0 + 0.4) + np.pi / 2) % np.pi - np.pi / 2
    print("position angle at lambda0 off by", d)
    assert abs(d) < 0.05                                            # observed: -0.0086 (the restatement's, seed 2)
    assert 0.6 < got["summary"][0, 4] / got["summary"][0, 2] < 1.0  # L/I: p = 0.8 and the noise's bias
    assert got["summary"][1, 4] < 0.3 * got["summary"][0, 4]        # noise alone has little L
    assert tm["kernels"] > 0 and tm["with_copy"] >= tm["kernels"]


def _stokes_iv(p4, req):
    on, non, off, noff = R.spectra(p4, DELAY, ZAPPED, req[0], req[1], req[2], 64, 8)
    i, q, u, v, w = R.stokes(on, non, off, noff, ZAPPED)
    return i, v


def _raw_pol(s, reqs, n=None, nrm=21):
    """pb_search_pol itself on sentinel-filled outputs -> (rc, message, outputs untouched?)"""
    q = np.ascontiguousarray(reqs, np.int32).reshape(-1, 3)
    n = q.shape[0] if n is None else n
    m = max(n, q.shape[0], 1)
    ints = [np.full(sh, -77, np.int32) for sh in ((m, 4, NCHAN), (m, NCHAN), (m, 4, NCHAN), (m, NCHAN), (m,))]
    dbl = [np.full(sh, -77.0) for sh in ((m, nrm, 2), (m, 6))]
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rc = s._L.pb_search_pol(s._s, q.ctypes.data_as(i32p), n, *[a.ctypes.data_as(i32p) for a in ints[:4]],
                            dbl[0].ctypes.data_as(f64p), ints[4].ctypes.data_as(i32p), dbl[1].ctypes.data_as(f64p))
    return rc, s._L.pb_search_last_error(s._s).decode(), all(np.all(a == -77) for a in ints + dbl)


def test_refusals_and_the_off_state():
    nsamp = 2500
    x = _noise_block(61, nsamp)
    p4, xt = R.planes(x)
    one = np.ascontiguousarray(xt.T)
    with search.Searcher(max_samples=nsamp, **KW) as s, search.Searcher(max_samples=nsamp, **KW) as fresh:
        want = fresh.run(one, want_series=True)
        rc, msg, clean = _raw_pol(s, [(0, 0, 1)])
        assert rc == EINVAL and "not switched on" in msg and clean                  # before set_pol
        with pytest.raises(libpb.PbError, match="set_pol"):
            s.pol(0, 0, 1)
        fill = C.c_int(-5)
        assert s._L.pb_search_pol_fetch(s._s, 0, one.ctypes.data_as(C.POINTER(C.c_uint8)), one.nbytes) == EINVAL
        # set_pol refuses values out of range and changes nothing
        for bad in (dict(off_len=0), dict(off_len=1025), dict(guard=-1), dict(guard=1025), dict(rm=(0.0, 1.0, 0)),
                    dict(rm=(0.0, 1.0, 8193)), dict(rm=(float("nan"), 1.0, 5)), dict(rm=(0.0, float("inf"), 5)), dict(max_cands=-1)):
            with pytest.raises(ValueError, match="pb_search_set_pol"):
                s.set_pol(**dict(dict(rm=(-10.0, 1.0, 21), max_cands=4), **bad))
            assert s._pol is None and _raw_pol(s, [(0, 0, 1)])[0] == EINVAL
        # not while streaming is on, and no streaming while it is on
        s.set_gulp(100)
        with pytest.raises(ValueError, match="streaming"):
            s.set_pol(rm=(-10.0, 1.0, 21), max_cands=4)
        s.set_gulp(0)
        s.set_pol(rm=(-10.0, 1.0, 21), max_cands=4)
        with pytest.raises(ValueError, match="polarisation"):
            s.set_gulp(100)
        for call in (lambda: s._L.pb_search_push(s._s, x.ctypes.data_as(C.c_void_p), 0, 10, 8, C.byref(fill)),
                     lambda: s._L.pb_search_push_f32(s._s, x.ctypes.data_as(C.c_void_p), 0, 10, C.c_float(1.0), C.byref(fill)),
                     lambda: s._L.pb_search_gulp_advance(s._s, 0),
                     lambda: s._L.pb_search_gulp_fetch(s._s, one.ctypes.data_as(C.POINTER(C.c_uint8)), one.nbytes, C.byref(fill))):
            assert call() == EINVAL and fill.value == -5 and "streaming is not switched on" in s._L.pb_search_last_error(s._s).decode()
        with pytest.raises(libpb.PbError):
            s.gulp_peaks(6.0)
        rc, msg, clean = _raw_pol(s, [(0, 0, 1)])
        assert rc == EINVAL and "no block searched" in msg and clean                # before any four-product run
        with pytest.raises(libpb.PbError, match="8-bit"):
            s.run(x[:1000], nbit=4)                                                 # nbit != 8 while the stage is on
        assert _raw_pol(s, [(0, 0, 1)])[0] == EINVAL                                # (nothing was searched)
        r = s.run(x, want_series=True)
        tout, ndm = r["tout"], s.ndm
        assert np.array_equal(r["series"], want["series"]) and r["snr"].tobytes() == want["snr"].tobytes()
        rc, msg, clean = _raw_pol(s, [(0, 5, 1)] * 5)
        assert rc == EINVAL and "max_cands" in msg and clean                        # n > max_cands
        for bad in ((0, 5, 0), (0, 5, 65), (0, 5, -4), (0, tout, 1), (0, -1, 1), (ndm, 5, 1), (-1, 5, 1)):
            rc, msg, clean = _raw_pol(s, [(1, 7, 2), bad])
            assert rc == EINVAL and "request 1 out of range" in msg and clean, bad
        rc, msg, clean = _raw_pol(s, [(1, 7, 2)], n=0)
        assert rc == 0 and clean                                                    # no request: nothing to do
        got = s.pol([1, 30], [7, tout - 1], [2, 64])                                # the next valid call works
        ref = R.pol(p4, DELAY, ZAPPED, LAM2, [(1, 7, 2), (30, tout - 1, 64)], 64, 8, -10.0, 1.0, 21)
        for k in SPEC:
            assert np.array_equal(got[k].astype(np.int64), ref[k]), k
        none = s._L.pb_search_pol(s._s, np.array([1, 7, 2], np.int32).ctypes.data_as(C.POINTER(C.c_int32)), 1, None, None, None, None,
                                  None, None, None)
        assert none == 0                                                            # any output may be NULL
        # off again: a 1-IF block runs and matches a fresh Searcher
        s.set_pol(max_cands=0)
        rc, msg, clean = _raw_pol(s, [(0, 0, 1)])
        assert rc == EINVAL and "not switched on" in msg and clean
        back = s.run(one, want_series=True)
        for k in ("snr", "width_log2", "series", "stats"):
            assert back[k].tobytes() == want[k].tobytes(), k
        assert np.array_equal(s.fetch_clean(), xt)
        s.set_gulp(100)                                                             # and streaming may be switched on again
        assert s.push(one[:50]) == 50


def test_gulps_carry_the_polarisation_of_their_candidates():
    """Three host gulps of 2500 samples; a pulse in the middle of the second (t 3700) and one whose on window [4996, 5004)
    straddles the boundary between the second and the third.  Each is compared with one search of the whole stream as a
    single block: trial DM, peak sample and width of the candidate, and every array of its "pol" entry -- the S/N itself is
    not, the statistics of a series being those of its block.  Both pulses are compared: a gulp's block starts
    max_delay + 63 = 667 samples before its first new sample, the off windows reach 72 samples before the peak and
    8 + 8 + 64 = 80 after it, and a candidate is only emitted by the gulp whose block holds every sample of its boxcars,
    so the gulped and the single-block requests sum the same samples."""
    gulp, n = 2500, 3
    pulses = [dict(t=3700, w=8, amp=2.5, p=0.8, rm=37.0, chi0=0.4), dict(t=4996, w=8, amp=2.5, p=0.6, rm=-20.0, chi0=1.0, v=0.3)]
    x = R.simulate(71, n * gulp, NCHAN, FCH1, FOFF, DELAY[15], pulses)
    rm = (-100.0, 1.0, 201)

    def strongest(cands, t):
        near = [c for c in cands if abs(c["peak_idx"] - t) <= 16 and "pol" in c]
        return max(near, key=lambda c: c["snr"]) if near else None

    with search.Searcher(max_samples=n * gulp, **KW) as s:
        s.set_pol(rm=rm, max_cands=8)
        s.set_cutouts(nsub=8, nt=16, ndmrow=4, max_cands=8)
        g = search.GulpSearch(s, threshold=10.0, pol=dict(thresh=12.0, max_per_gulp=8))
        whole = g.push(x.reshape(n * gulp, 4 * NCHAN)) + g.finish()
    with search.Searcher(max_samples=gulp + MAXD + 63 + 64, **KW) as s:
        s.set_pol(rm=rm, max_cands=8)
        s.set_cutouts(nsub=8, nt=16, ndmrow=4, max_cands=8)
        g = search.GulpSearch(s, threshold=10.0, pol=dict(thresh=12.0, max_per_gulp=8))
        with pytest.raises(ValueError):
            g.feed(x[:10])
        with pytest.raises(ValueError):
            g.feed_plane(np.zeros((10, NCHAN), np.float32))
        batches = [g.push(x[k * gulp:(k + 1) * gulp]) for k in range(n)] + [g.finish()]
    with pytest.raises(ValueError):
        with search.Searcher(max_samples=gulp + MAXD + 127, **KW) as s:
            s.set_pol(max_cands=2)
            search.GulpSearch(s, gulp=gulp, pol={})
    for t, where in ((3700, 1), (4996, 2)):
        a = strongest(whole, t)
        b = strongest(batches[where], t)
        assert a is not None and b is not None, t
        assert all(strongest(bt, t) is None for i, bt in enumerate(batches) if i != where), t      # emitted once
        assert (a["dmi"], a["peak_idx"], a["tfilt"]) == (b["dmi"], b["peak_idx"], b["tfilt"]), t
        for k in search.POL_KEYS + ("pft", "pft_hits"):
            assert np.array_equal(a["pol"][k], b["pol"][k], equal_nan=True), (t, k)
        assert a["pol"]["tscr"] == b["pol"]["tscr"] and a["pol"]["pft"].shape == (4, 8, 16)
    a = strongest(whole, 3700)
    assert abs(a["dmi"] - 15) <= 1 and abs(search.pol_numbers(a["pol"])[0] - 37.0) <= 2.0
    assert abs(search.pol_numbers(strongest(whole, 4996)["pol"])[0] + 20.0) <= 2.0
    assert all("pol" not in c for c in whole if c["snr"] < 12.0)


def test_cli_writes_pol_files(tmp_path, capsys):
    """search -pol on a nifs 4 file written here (not the filterbank host's: that seam is covered by
    test_the_self_test_pulse_of_a_coherence_file_goes_through_search_pol below): the candidate
    lines are those of the same file's total intensity searched without -pol, every gulp with polarised candidates gets a
    .pol file whose lines parse and a .pol.npz whose `on` sums equal the restatement applied to the file's bytes."""
    import os
    sig = importlib.import_module("vlite-fast_amd.sigproc")
    x = R.simulate(81, 7500, NCHAN, FCH1, FOFF, DELAY[15], [dict(t=3700, w=8, amp=2.5, p=0.8, rm=37.0, chi0=0.4)])
    p4, xt = R.planes(x)

    def fil(name, nifs, body):
        hdr = b"".join([sig.send_string("HEADER_START"), sig.send_int("data_type", 1), sig.send_double("fch1", FCH1),
                        sig.send_double("foff", FOFF), sig.send_int("nchans", NCHAN), sig.send_int("nbits", 8),
                        sig.send_double("tstart", 57570 + 3600 / 86400.), sig.send_double("tsamp", TSAMP),
                        sig.send_int("nifs", nifs), sig.send_string("HEADER_END")])
        (tmp_path / name).write_bytes(hdr + body.tobytes())
        return str(tmp_path / name)

    args = ["-dm", "0", "60", "-dm_step", "2", "-nsamps_gulp", "2500", "-boxcar_max", "64", "-zap_chans", "0", "3", "-zap_chans",
            "90", "96", "-detect_thresh", "10"]
    n1 = search.main(["-f", fil("one.fil", 1, np.ascontiguousarray(xt.T))] + args)
    plain = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    out = tmp_path / "cands"
    n4 = search.main(["-f", fil("four.fil", 4, x)] + args + ["-pol", "-pol_thresh", "12", "-pol_max", "4", "-rm", "-100", "100",
                                                             "-rm_step", "1", "-output_dir", str(out), "-cutouts"])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert n4 == n1 == len(lines) >= 1 and lines == plain                       # the search is the 1-IF one
    pols = sorted(p for p in os.listdir(out) if p.endswith(".pol"))
    assert pols and all(p[:-4] + ".cand" in os.listdir(out) and p + ".npz" in os.listdir(out) for p in pols)
    seen = 0
    for p in pols:
        rows = [l.split("\t") for l in open(out / p).read().splitlines()]
        z = np.load(out / (p + ".npz"))
        cand_lines = open(out / (p[:-4] + ".cand")).read().splitlines()
        assert len(rows) == z["on"].shape[0] <= 4 and z["F"].shape[1:] == (201, 2) and z["pft"].shape[1] == 4
        assert np.array_equal(z["rms"], -100.0 + np.arange(201))
        for i, cols in enumerate(rows):
            assert len(cols) == 13 and "\t".join(cols[:9]) in cand_lines and float(cols[0]) >= 12.0
            nums = [float(v) for v in cols[9:]]                                  # RM, L/I, V/I, angle in degrees
            assert nums[0] == z["summary"][i, 5] and -90.0 <= nums[3] <= 90.0
            peak, tfilt, dmi = int(z["cands"][i, 1]), int(z["cands"][i, 3]), int(z["cands"][i, 4])
            assert peak == int(cols[1]) and dmi == int(cols[4])
            on, non, off, noff = R.spectra(p4, DELAY, ZAPPED, dmi, peak, 1 << tfilt, 64, 8)
            if np.all(z["noff"][i][~ZAPPED] == 128):        # windows that the gulp's block did not cut hold what the file's do
                assert np.array_equal(z["on"][i], on) and np.array_equal(z["non"][i], non), (p, i)
                assert np.array_equal(z["off"][i], off) and np.array_equal(z["noff"][i], noff), (p, i)
                seen += 1
            if abs(peak - 3700) <= 8 and abs(dmi - 15) <= 1:
                assert abs(nums[0] - 37.0) <= 2.0 and 0.5 < nums[1] < 1.1
    assert seen >= 1


SEAM_R = 256                        # rows per segment of the seam test: 32 samples per segment, 320 per shortened second


def test_the_self_test_pulse_of_a_coherence_file_goes_through_search_pol(tmp_path, capsys, oracle):
    """The seam.  The Python host writes an 8-bit -P 2 --coherence file with its self-test pulse (-i: DM 80, 2 ms, x1.05,
    injected from the first row of the first second, which is second 3600 of the dump), search -pol reads it.
    The host's delays and width scale with the rows per segment (set_frb_delays: rate = R x 12500 x 10), so at 256 rows
    the sweep is 0.99 of a shortened second -- 317 of its 320 samples -- and at the header's tsamp it is DM 80 x 256 / 1024
    = 20; the pulse arrives in output channel 0 at set_frb_delays(80, 256)[2155] / 8 = 90.5 samples.  Two seconds are
    written (a third is read and dropped): 640 samples, searched as one block at DM 0, 1 .. 26.
    Expected S/N: the pulse is 5.1 rows of the 8 of a sample at 1.05^2 in power, +6.6 % of a sample whose relative rms is
    1 / 4 (16 exponentials: 8 rows, two hands) -- 0.26 sigma per channel, x sqrt(3710 channels) = 16.  As
    tests/test_gpu_chain.py does, the test asks for half of that, at the sweep's DM within one trial and within 4 samples
    of the arrival sample.  Observed on an MI355X: S/N 13.26 at sample 90, trial DM 20.  The sums in .pol.npz equal the restatement applied to the file's bytes for every candidate
    (one block: stream and block coordinates are the same) and the .pol lines parse.  Nothing is asserted about the RM of
    an unpolarised injection."""
    import os
    from test_gpu_pipeline import _dump
    sig = importlib.import_module("vlite-fast_amd.sigproc")
    pbmod = importlib.import_module("vlite-fast_amd.process_baseband")
    dump = str(tmp_path / "obs.uw")
    rng = np.random.default_rng(91)                 # Gaussian baseband: two seconds of 10 segments, two hands; the third
    n = SEAM_R * 12500                              # second, which the host drops, repeats the second
    two = np.clip(rng.standard_normal((20, 2, n), dtype=np.float32) * np.float32(16.9) + np.float32(128.5), 0, 255).astype(np.uint8)
    _dump(dump, np.concatenate([two, two[10:]]))
    d = tmp_path / "fb"
    os.makedirs(str(d))
    argv = ["-i", "-w", "2", "-r", "2", "-b", "8", "-P", "2", "--coherence", "--no-control", "--replay", dump, "--datadir", str(d),
            "--logdir", str(d / "logs"), "--rows-per-seg", str(SEAM_R)]
    assert pbmod.run(pbmod.build_parser().parse_args(argv)) == 0
    fil = [str(d / f) for f in sorted(os.listdir(str(d))) if f.endswith("_kur.fil")][0]
    raw = open(fil, "rb").read()
    hdr, off = sig.read_header(raw[:4096])
    assert hdr["nifs"] == 4 and hdr["nbits"] == 8 and hdr["nchans"] == 4096
    body = np.frombuffer(raw[off:], np.uint8).reshape(-1, 4, 4096)
    assert body.shape[0] == 640
    out = tmp_path / "cands"
    n = search.main(["-f", fil, "-dm", "0", "26", "-dm_step", "1", "-boxcar_max", "16", "-nsamps_gulp", "640", "-detect_thresh", "6",
                     "-zap_chans", "0", "190", "-zap_chans", "3900", "4096", "-pol", "-pol_max", "4", "-rm", "-50", "50", "-rm_step",
                     "1", "-pol_off", "16", "2", "-output_dir", str(out)])
    lines = [l.split("\t") for l in capsys.readouterr().out.splitlines() if l.strip()]
    arrival = float(oracle.set_frb_delays(80.0, SEAM_R)[2155]) / 8.0
    dm_sweep = 80.0 * SEAM_R / 1024.0
    with capsys.disabled():
        print("\nseam: %d candidates; strongest S/N %s at sample %s, DM %s; arrival %.2f, sweep DM %.2f"
              % (n, lines[0][0] if lines else None, lines[0][1] if lines else None, lines[0][5] if lines else None, arrival, dm_sweep))
    assert n >= 1 and abs(arrival - 90.5) < 0.5
    best = max(lines, key=lambda c: float(c[0]))
    assert float(best[0]) >= 8.0                                    # half of the expected 16
    assert abs(float(best[5]) - dm_sweep) <= 1.0 and abs(int(best[1]) - arrival) <= 4
    zapped = R.zap_mask(4096, search.HEIMDALL_ZAP)
    delay = R.delays(np.arange(0.0, 27.0), hdr["fch1"], hdr["foff"], 4096, hdr["tsamp"])
    p4, _ = R.planes(body)
    pols = sorted(p for p in os.listdir(out) if p.endswith(".pol"))
    assert pols
    found = 0
    for p in pols:
        rows = [l.split("\t") for l in open(out / p).read().splitlines()]
        z = np.load(out / (p + ".npz"))
        assert 1 <= len(rows) == z["on"].shape[0] <= 4 and z["F"].shape[1:] == (101, 2) and "pft" not in z
        for i, cols in enumerate(rows):
            assert len(cols) == 13 and all(np.isfinite(float(v)) for v in cols[9:])
            peak, tfilt, dmi = int(z["cands"][i, 1]), int(z["cands"][i, 3]), int(z["cands"][i, 4])
            on, non, off, noff = R.spectra(p4, delay, zapped, dmi, peak, 1 << tfilt, 16, 2)
            for k, v in zip(SPEC, (on, non, off, noff)):
                assert np.array_equal(z[k][i], v), (p, i, k)
            found += cols[:9] == best[:9]
    assert found == 1                                               # the pulse's candidate carries its polarisation


def test_more_polarised_candidates_than_cutouts_and_flags_without_pol():
    """GulpSearch(pol=...) analyses up to its own max_per_gulp; the images stop at the cutouts' max_cands"""
    x = R.simulate(71, 2500, NCHAN, FCH1, FOFF, DELAY[15], [dict(t=900, w=8, amp=2.5, p=0.8, rm=37.0, chi0=0.4)])
    with search.Searcher(max_samples=2500, **KW) as s:
        s.set_pol(rm=(-10.0, 1.0, 21), max_cands=8)
        s.set_cutouts(nsub=8, nt=16, ndmrow=4, max_cands=2)
        g = search.GulpSearch(s, threshold=8.0, pol=dict(thresh=8.0, max_per_gulp=8))
        cands = g.push(x.reshape(2500, 4 * NCHAN)) + g.finish()
    withpol = [c for c in cands if "pol" in c]
    assert len(withpol) >= 3 and [c["snr"] for c in withpol] == sorted((c["snr"] for c in cands), reverse=True)[:len(withpol)]
    assert ["pft" in c["pol"] for c in withpol] == [True, True] + [False] * (len(withpol) - 2)
    for bad in (["-rm", "1", "2"], ["-pol_max", "3"], ["-rm_step", "1"], ["-pol_thresh", "7"], ["-pol_off", "8", "1"]):
        with pytest.raises(SystemExit):
            search.parse_args(["-f", "x.fil"] + bad)
    with pytest.raises(SystemExit):
        search.parse_flags("-rm 1 2")


def test_planes_of_a_channel_count_that_is_no_multiple_of_four():
    """nchan 98: the rows are not dword multiples, so the block goes byte by byte, host block included"""
    nchan, nsamp = 98, 2501
    x = np.random.default_rng(12).integers(0, 256, (nsamp, 4, nchan)).astype(np.uint8)
    x[50:60] = 255
    p4, xt = R.planes(x)
    with search.Searcher(max_samples=nsamp, **dict(KW, nchan=nchan, zap=())) as s:
        s.set_pol(max_cands=1)
        s.run(x)
        for k in range(4):
            assert np.array_equal(s.pol_fetch(k), p4[k]), k
        assert np.array_equal(s.fetch_clean(), xt)


def test_set_pol_refuses_buffers_beyond_two_gib():
    """4096 channels x 140 000 samples: the four planes alone are 2.3 GB"""
    with search.Searcher(nchan=4096, max_samples=140000, dm_min=0.0, dm_max=2.0, dm_step=2.0, boxcar_max=4, zap=()) as s:
        with pytest.raises(ValueError, match="2 GiB"):
            s.set_pol(max_cands=1)
        assert s._pol is None
        with pytest.raises(libpb.PbError, match="set_pol"):
            s.pol(0, 0, 1)
        s.set_gulp(100)                                             # nothing was switched on: streaming is still allowed
