"""The refinement's definition (include/pb_hip.h under pb_search_set_refine) without a GPU: the NumPy restatement
(tests/search_refine_ref.py) against what the reference's own refine_dm / optimize_pulse / tophat_smooth / qn returned
(tests/golden/reference_refine.npz, made by tests/golden/make_refine_golden.py), against hand-made answers, on an
off-grid pulse, and over the GPU test's seeded inputs.  S/N tolerances are search_refine_ref.sn_bound: the rounding of
the float64 operands, nothing measured."""
import importlib
from fractions import Fraction

import numpy as np
import pytest

import make_refine_golden as G
import search_refine_cases as K
import search_refine_ref as R

search = importlib.import_module("vlite-fast_amd.search")


@pytest.fixture(scope="module")
def gold():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "reference_refine.npz"))


def _series(oracle, fb, dm):
    """the reference's dedispersed, masked sum (oracle.dedisperse and chan_mask restate it; tests/test_oracle_golden.py
    holds them to the reference): only the estimator is under test here"""
    work = fb.copy()
    oracle.dedisperse(work, dm, G.TSAMP, ref_freq=G.FREF)
    q = work[0][oracle.chan_mask() == 1].astype(np.int64).sum(axis=0)
    return q


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_reproduces_the_reference(oracle, gold, name):
    seed, ntime, dm, t0, plen, amp, t_pk, dm0, ddm, rng = G.CASES[name]
    fb = G.plane(seed, ntime, dm, t0, plen, amp)
    assert np.array_equal(gold[name + "_params"][[0, 1, 6]], [seed, ntime, t_pk])
    i0, i1 = R.window(t_pk, G.H, ntime)
    assert (i0, i1) == tuple(gold[name + "_params"][10:12].astype(int)) and (name != "edge" or i0 == 0)
    # optimize_pulse at the candidate DM: the width the reference went on with
    wp0 = R.width_pass(_series(oracle, fb, dm0), t_pk, G.H, 32)
    assert np.array_equal(wp0["opt_loc"], gold[name + "_opt0_locs"].astype(int))
    assert np.all(np.abs(wp0["opt_sn"] - gold[name + "_opt0_sns"]) <= wp0["err"])
    width = int(wp0["widths"][np.argmax(wp0["opt_sn"])])
    assert width == int(gold[name + "_width"])
    # refine_dm at that width
    dms = gold[name + "_dms"]
    q = np.stack([_series(oracle, fb, d) for d in dms])
    dp = R.dm_pass(q, np.ones(dms.size, bool), t_pk, width, G.H)
    print(name, "worst |sn - ref| / bound:", np.max(np.abs(dp["sn_dm"] - gold[name + "_sns"]) / dp["err"]))
    assert np.all(np.abs(dp["sn_dm"] - gold[name + "_sns"]) <= dp["err"])
    kb = int(np.argmax(gold[name + "_sns"]))
    assert dp["kbest"] == kb
    # qn and the smoothed series of the best trial, optimize_pulse at the refined DM
    qn = float(gold[name + "_qn_window"])
    assert abs(dp["qn"][kb] - qn) <= np.spacing(qn)
    sm, _, _ = R.smooth(q[kb], width)
    gs = gold[name + "_smooth"]
    assert np.all(np.abs(sm[i0:i1] - gs) <= 2 * np.spacing(gs))          # the reference multiplies by a rounded 1 / n
    if name == "edge":
        assert sm[0] == float(q[kb][0]) == gs[0]                         # the ramp: one sample at t = 0
    wp = R.width_pass(q[kb], t_pk, G.H, 32)
    assert np.array_equal(wp["widths"], gold[name + "_widths"])
    assert np.array_equal(wp["opt_loc"], gold[name + "_opt_locs"].astype(int))
    assert np.all(np.abs(wp["opt_sn"] - gold[name + "_opt_sns"]) <= wp["err"])


def test_the_pieces_by_hand():
    assert R.qn_quarters([1, 2, 4, 8]) == 9 and R.qn([1, 2, 4, 8]) == 2.2219 * 2.25      # differences 1 2 3 4 6 7 at 1.25
    assert R.qn_quarters([5, 5, 5, 9]) == 0 and R.qn_quarters([0, 10]) == 40
    assert R.med2([5, 1, 9, 3]) == 8 and R.med2([7, 1, 4]) == 8
    assert np.array_equal(R.smooth([3, 6, 9, 12, 0], 3)[0], [3, 6, 9, 7, 0])
    assert np.array_equal(R.smooth([3, 6, 9, 12, 0], 5)[0], [3, 6, 6, 7, 0])
    assert R.odd(4) == 5 and R.odd(5) == 5 and R.odd(1) == 1


def _slow(q, t_pk, width, H, wmax):
    """one evaluated trial by the header's words, in exact rationals, written apart from the restatement"""
    T = len(q)
    w = width + 1 if width % 2 == 0 else width
    i0, i1 = max(0, t_pk - H), min(T, t_pk + H)
    n = i1 - i0

    def med(v):
        v = sorted(v)
        return Fraction(v[(len(v) - 1) // 2] + v[len(v) // 2], 2)

    def qnf(v):
        d = sorted(abs(a - b) for i, a in enumerate(v) for b in v[i + 1:])
        pos = Fraction(len(d) - 1, 4)
        r = int(pos)
        return d[r] + (pos - r) * (d[min(r + 1, len(d) - 1)] - d[r])

    best = None
    for t in range(i0, i1):
        h = min(w // 2, t, T - 1 - t)
        v = Fraction(sum(q[t - h:t + h + 1]), 2 * h + 1)
        best = v if best is None or v > best else best
    num, sig = best - med(q[i0:i1]), qnf(q[i0:i1])
    sn = 0.0 if sig == 0 else float(num) / (2.2219 * float(sig) / np.sqrt(w))
    off = q[i0:i0 + n // 4] + q[i0 + 3 * n // 4:i1]
    m, s = med(off), qnf(off)
    opt = []
    for ww in range(1, wmax, 2):
        cand = [(sum(q[t - ww // 2:t + ww // 2 + 1]), -t) for t in range(i0 + ww, i1 - ww)]
        top, mt = max(cand)
        opt.append((-mt - i0, 0.0 if s == 0 else float(Fraction(top, ww) - m) / (2.2219 * float(s)) * np.sqrt(ww)))
    return sn, opt


def test_hand_made_requests():
    rng = np.random.default_rng(5)
    T, H, wmax = 40, 16, 4
    q = rng.integers(900, 1100, (3, T))
    q[1, 19:22] += 400
    q[2, 20:22] += 300
    # an even width (4 -> 5), a window clipped at both ends ([4, 36) would fit: take H = 24 -> [0, 40))
    for width, Hh in ((4, 16), (3, 24), (1, 16)):
        r = R.refine(q, [True, True, True], 20, width, Hh, wmax)
        assert r["status"] == 0 and r["kbest"] == 1
        for k in range(3):
            sn, opt = _slow(q[k].tolist(), 20, width, Hh, wmax)
            assert abs(r["sn_dm"][k] - sn) <= 4 * np.spacing(abs(sn)), (width, k)
            if k == 1:
                assert [o[0] for o in opt] == r["opt_loc"].tolist()
                assert np.all(np.abs(np.array([o[1] for o in opt]) - r["opt_sn"]) <= 4 * np.spacing(np.abs(r["opt_sn"])))
    assert R.window(20, 24, T) == (0, 40)
    even, odd5 = R.refine(q, [True] * 3, 20, 4, 16, wmax), R.refine(q, [True] * 3, 20, 5, 16, wmax)
    assert np.array_equal(even["sn_dm"], odd5["sn_dm"])
    # qn == 0: more than a quarter of the pair differences vanish -> S/N 0 in both passes, first trial wins
    flat = np.full((2, T), 1000)
    flat[:, 20] = 5000
    r = R.refine(flat, [True, True], 20, 1, 16, wmax)
    assert r["status"] == 0 and np.array_equal(r["sn_dm"], [0, 0]) and r["kbest"] == 0 and not r["opt_sn"].any()
    # the spike is found all the same: i0 = 4, so t = 20 is position 16; the first 3-sample mean that holds it is t = 19's
    assert r["opt_loc"].tolist() == [16, 15]
    # a window shorter than 4 wmax: status 1, nothing computed
    r = R.refine(q, [True] * 3, 2, 1, 8, wmax)                           # [0, 10): 10 < 16
    assert r["status"] == 1 and np.isnan(r["sn_dm"]).all() and r["kbest"] == -1 and (r["opt_loc"] == -1).all()
    assert np.isnan(r["opt_sn"]).all()
    # trials outside the grid: NaN, never the winner; none inside: kbest -1
    r = R.refine(q, [True, False, True], 20, 3, 16, wmax)
    assert np.isnan(r["sn_dm"][1]) and r["kbest"] == 2 and r["status"] == 0
    r = R.refine(q, [False] * 3, 20, 3, 16, wmax)
    assert r["status"] == 0 and r["kbest"] == -1 and np.isnan(r["sn_dm"]).all() and np.isnan(r["opt_sn"]).all()


def test_off_grid_pulse_is_refined_towards_its_dm():
    x, kw, dms, dm_true, t0, tout = K.offgrid_inputs()
    r, st1 = K.two_pass(x.T, np.arange(kw["nchan"]), tout, dms, kw["fch1"], kw["foff"], kw["nchan"], 4, t0, 1)
    print("refined DM %.4f (true %.1f, grid %.1f), pass-1 step %.4f, S/N %.1f, width %d, peak %d" % (
        r["dm"], dm_true, dms[4], st1, r["snr"], r["width"], r["peak"]))
    assert abs(r["dm"] - dm_true) <= 0.5 * st1 and abs(r["dm"] - dm_true) < abs(dms[4] - dm_true)
    assert r["snr"] > 20 and abs(r["peak"] - t0) <= 2 and r["width"] <= 5


def test_near_ties_of_the_gpu_inputs_stay_under_the_cap():
    n = ties = 0
    for case in range(len(K.CASES)):
        kw, dms, zapped, maxd = K.geometry(case)
        tout, T = K.length(case)
        x = K.codes(case, T)
        xt = x.T
        if K.CASES[case][6]:
            xt = K.cleaned_block(xt, zapped)            # the cleaning restated (tests/search_rfi_ref.py)
            assert not np.array_equal(xt, x.T)
        res = K.restate(case, xt, tout, dms)
        n += len(res)
        ties += sum(r["near_tie"] for r in res)
    print("near-ties of the DM pass: %d of %d requests" % (ties, n))
    assert ties <= K.NEAR_TIE_CAP * n


def test_cli_flags():
    a = search.parse_args(["-f", "x.fil", "-refine", "-refine_max", "4"])
    assert a.refine and a.refine_thresh == a.detect_thresh and a.refine_max == 4
    assert not search.parse_args(["-f", "x.fil"]).refine
    with pytest.raises(SystemExit):
        search.parse_args(["-f", "x.fil", "-refine", "-refine_max", "0"])
    c = dict(snr=9.5, peak_idx=1200, peak_time=0.9375, tfilt=2, dmi=7, dm=20.0, ngiant=3, i0=1198, i1=1204,
             refined=dict(dm=20.125, snr=12.25, width=5, peak=1201))
    t = search.refined_line(c).split()
    assert len(t) == 13 and t[:9] == search.candidate_line(c).split()
    assert (float(t[9]), float(t[10]), int(t[11]), int(t[12])) == (20.125, 12.25, 5, 1201)
