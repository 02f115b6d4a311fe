"""The 54 seeded coherence cases of tests/coherence_cases.py, without a GPU: (a) what they cover, as conditions on the
draw, and (b) tests/coherence_ref.py on exactly these inputs against the oracle -- its AA / BB planes and codes are
orc_segment's npol = 2 planes and codes (NaN where the oracle has NaN), the oracle's row weights of the two pols are
equal (k_detect_coh keeps one weight per row), and the inputs reach the edges at which CR and CI have branches of their
own: weight 0, 0 < w < 0.2, the 11x clip at non-zero weights, NaN in the raw stream."""
import numpy as np
import pytest

import coherence_cases as CC
import coherence_ref as CR
from helpers import compact_ave, oracle_run

NCO = 4096
SEEDS = range(CC.NCASES)


def test_cases_cover_what_they_are_for():
    cs = [CC.case(s, with_data=False) for s in SEEDS]
    assert {(c["T"], c["nbit"], c["rfi_mode"]) for c in cs} == {(T, b, m) for T in (32, 8) for b in (8, 4, 2) for m in (0, 1, 2)}
    for c in cs:
        assert c["T"] == (32 if c["R"] % 32 == 0 else 8) and c["lag"] < c["nsets"] and c["nseg"] <= c["max_seg"], c
    assert {c["nant"] for c in cs} == {1, 2}
    assert {c["nsets"] for c in cs} == {1, 2, 3}
    assert any(c["lag"] > 0 for c in cs)
    assert any(c["max_seg"] > c["nseg"] for c in cs)
    assert {c["inject"] for c in cs} == {False, True}
    assert {c["keep_ave"] for c in cs} == {False, True}
    for mode in (0, 1, 2):
        kinds = {k for c in cs if c["rfi_mode"] == mode for k in c["kinds"]}
        assert kinds == set(range(CC.NKINDS)), (mode, kinds)
    # the bandpass stays 0 through a first segment of code 0 and is initialised again at the second
    assert any(4 in c["kinds"] and c["nseg"] * c["nb"] >= 2 for c in cs)
    # two antennas under one, two and three buffer sets
    assert {c["nsets"] for c in cs if c["nant"] == 2} == {1, 2, 3}


_done = {}


def _evaluate(O, seed):
    """the reference over the whole stream of every antenna of case `seed` against the oracle -> dict of counts"""
    if seed in _done:
        return _done[seed]
    c = CC.case(seed)
    R, mode, nbit = c["R"], c["rfi_mode"], c["nbit"]
    nsegs = c["nseg"] * c["nb"]
    delays = O.set_frb_delays(80.0, R) if c["inject"] else None
    inj = 1 if c["inject"] else 0
    r = dict(plane_diff=0, nan_diff=0, code_diff=0, weight_diff=0, w0=0, wlow=0, clip=0, raw_nan=0, kur_nan=0)
    for d in c["datas"]:
        clips = {}
        ref = CR.run(O, d, R, mode, nbit, delays, inj, clip_out=clips)
        res, _, _ = oracle_run(O, d, R, rfi_mode=mode, npol=2, nbit=nbit, frb_delays=delays, inject_now=inj)
        w = np.stack([x.weights.reshape(2, R) for x in res])                      # [nsegs][2][R]
        if mode:
            r["weight_diff"] += int((w[:, 0].view(np.uint32) != w[:, 1].view(np.uint32)).sum())
            r["w0"] += int((w[:, 0] == 0).sum())
            r["wlow"] += int(((w[:, 0] > 0) & (w[:, 0] < np.float32(0.2))).sum())
            both = ((w[:, 0] != 0) & (w[:, 1] != 0))[:, :, None]                  # [nsegs][R][1]
            cl = np.stack(clips[1])                                               # [nsegs][2][R][4096]
            r["clip"] += int(((cl[:, 0] | cl[:, 1]) & both).sum())
        for st in CC.streams(mode):
            rc, rp = ref[st]
            orc = np.stack([compact_ave(x.ave_kur if st else x.ave_raw, R, 2).reshape(2, R // 8, NCO) for x in res])
            mine = rp[:, :2]
            nm, no = np.isnan(mine), np.isnan(orc)
            r["nan_diff"] += int((nm != no).sum())
            r["plane_diff"] += int(((mine.view(np.uint32) != orc.view(np.uint32)) & ~nm & ~no).sum())
            oc = np.concatenate([x.codes_kur if st else x.codes_raw for x in res])
            b = NCO * nbit // 8
            r["code_diff"] += int((rc.reshape(nsegs * R // 8, 4, b)[:, :2].ravel() != oc).sum())
            r["kur_nan" if st else "raw_nan"] += int(np.isnan(rp[:, 2]).sum())
    _done[seed] = r
    return r


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_aa_bb_are_the_oracles(oracle, seed):
    r = _evaluate(oracle, seed)
    what = CC.describe(CC.case(seed, with_data=False))
    assert r["nan_diff"] == 0, "case %s: NaN in %d places where the other has none" % (what, r["nan_diff"])
    assert r["plane_diff"] == 0, "case %s: %d AA / BB plane values differ" % (what, r["plane_diff"])
    assert r["code_diff"] == 0, "case %s: %d AA / BB code bytes differ" % (what, r["code_diff"])
    assert r["weight_diff"] == 0, "case %s: %d row weights differ between the pols" % (what, r["weight_diff"])
    assert r["kur_nan"] == 0, "case %s: %d NaN in the excised stream's CR" % (what, r["kur_nan"])


def test_inputs_reach_the_edges(oracle):
    tot = {}
    for s in SEEDS:
        for k, v in _evaluate(oracle, s).items():
            tot[k] = tot.get(k, 0) + v
    assert tot["w0"] > 0, "no row of weight 0"
    assert tot["wlow"] > 0, "no row with 0 < w < 0.2"
    assert tot["clip"] > 0, "no sample takes the 11x clip at non-zero weights"
    assert tot["raw_nan"] > 0, "no NaN in a raw-stream CR plane"
