"""What the search's stages share (csrc/search_dev.h, search_internal.h), on the GPU: a saturated block through every
user of the packed-byte gather -- the 16-bit partial sums at their largest, both flush points and the tail loop --
against closed-form sums, and the stages' buffers across a switch off and on again with another geometry."""
import importlib

import numpy as np
import pytest

import search_cutout_ref as R
from test_gpu_search import _plane

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")
FCH1, FOFF = 361.94, -0.16


def test_saturated_block_through_every_user_of_the_gather():
    nchan, T, zap = 520, 1024, ((0, 5),)
    nact = 515                                          # = 2 * 240 + 35, and 515 % 4 == 3
    codes = np.full((T, nchan), 255, np.uint8)
    with search.Searcher(nchan=nchan, max_samples=T, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_min=0.0, dm_max=20.0,
                         dm_step=4.0, boxcar_max=4, zap=zap) as s:
        r = s.run(codes, want_series=True)
        tout = r["tout"]
        assert r["series"].shape == (s.ndm, tout) and np.all(r["series"] == 255 * nact)
        s.set_refine(nstep=3, half_window=16, wmax=4, max_cands=2)
        tpk = np.array([5, tout // 2])
        f = s.refine_raw(t=tpk, width=3, dm_lo=2.0, dm_step=4.0, want_series=True)
        t = tpk[:, None] - 18 + np.arange(36)[None, :]              # sample of each position of a fine series
        want = np.where((t >= 0) & (t < tout), 255 * nact, 0).astype(np.uint32)
        assert f["series"].shape == (2, 3, 36)
        assert np.array_equal(f["series"], np.broadcast_to(want[:, None, :], (2, 3, 36)))
        s.set_cutouts(nsub=4, nt=8, ndmrow=2, max_cands=3)
        reqs = [(1, 5, 1), (3, tout // 2, 2), (5, tout - 1, 8)]
        c = s.cutouts(*zip(*reqs))
        delay = R.delays(s.dms, FCH1, FOFF, nchan, search.TSAMP)
        ref = R.cutouts(codes.T, delay, R.zap_mask(nchan, zap), r["series"], 4, 8, 2, reqs)
    assert np.array_equal(c["ft_hits"], ref["ft_hits"]) and c["ft_hits"].any()
    assert np.array_equal(c["ft"], 255 * c["ft_hits"])


def _use_stages(s, cut, ref, gi, tout):
    """each stage once on the searcher's current block, with the given geometry: every array that comes back"""
    s.set_cutouts(**cut)
    s.set_refine(**ref)
    s.set_giants(**gi)
    out = {}
    c = s.cutouts([2, 9], [40, tout - 3], [1, 4])
    out.update({"cut_" + k: c[k] for k in ("ft", "ft_hits", "dt", "dt_hits")})
    f = s.refine_raw(t=[700, 30], width=[4, 1], dm_lo=30.0, dm_step=1.5, want_series=True)
    out.update({"rf_" + k: f[k] for k in ("status", "sn_dm", "kbest", "opt_sn", "opt_loc", "series")})
    g = s.giants(3.0, want_list=True)
    out.update({"gi_" + k: g[k] for k in ("snr", "peak", "tfilt", "dmi", "members", "npoints", "i0", "i1")})
    out.update({"gl_" + k: v for k, v in g["giant_list"].items()})
    out["gi_n"] = np.array([g["ngiants"], int(g["overflow"])])
    return out


def test_stages_switched_off_and_on_again_with_another_geometry():
    nchan, T = 64, 2048
    codes, _ = _plane(91, T, nchan, dm=40.0, t0=700, width=4, amp=0.8, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP)
    kw = dict(nchan=nchan, max_samples=T, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_min=0.0, dm_max=80.0, dm_step=4.0,
              boxcar_max=16, zap=())
    first = (dict(nsub=4, nt=16, ndmrow=4, max_cands=4), dict(nstep=8, half_window=64, wmax=8, max_cands=4),
             dict(sep_time=3, sep_dm=5, sep_filter=3, max_giants=1 << 14))
    second = (dict(nsub=8, nt=24, ndmrow=2, max_cands=2), dict(nstep=5, half_window=40, wmax=16, max_cands=3),
              dict(sep_time=8, sep_dm=2, sep_filter=1, max_giants=1 << 12))
    s = search.Searcher(**kw)
    tout = s.run(codes)["tout"]
    a = _use_stages(s, *first, tout)
    s.set_cutouts(max_cands=0)
    s.set_refine(max_cands=0)
    s.set_giants(max_giants=0)
    for call in (lambda: s.cutouts(0, 0, 1), lambda: s.refine_raw(0, 1, 0.0, 1.0), lambda: s.giants(3.0)):
        with pytest.raises(Exception, match="not switched on"):
            call()
    b = _use_stages(s, *second, tout)
    with search.Searcher(**kw) as fresh:
        assert fresh.run(codes)["tout"] == tout
        want = _use_stages(fresh, *second, tout)
    assert a["gi_n"][0] > 0 and b["gi_n"][0] > 0 and not b["gi_n"][1]
    assert a["cut_ft"].shape != b["cut_ft"].shape and a["rf_series"].shape != b["rf_series"].shape
    assert set(b) == set(want)
    for k in want:
        assert b[k].dtype == want[k].dtype and np.array_equal(b[k], want[k], equal_nan=b[k].dtype.kind == "f"), k
    s.close()                                           # destroyed with every stage on: the process goes on cleanly
