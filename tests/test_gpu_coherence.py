"""Coherence output (AA, BB, CR, CI) on the GPU: AA and BB byte for byte what npol = 2 writes, CR and CI bit-exact
against the CPU reference of tests/coherence_ref.py, the pipelining modes, and properties that do not depend on the
formula's details."""
import numpy as np
import pytest

import coherence_ref as CR
from helpers import compact_ave, libpb, make_input, oracle_run

pytestmark = pytest.mark.gpu

NCO = 4096


def _run(lp, data, R, rfi_mode, nbit, coherence, inject=False, keep_ave=True, nsets=1, nbatch=1, nant=1):
    """data [nseg][2][n]; the segments go through in nbatch equal batches.  -> {stream: codes}, {stream: planes}"""
    nseg = data.shape[0]
    per = nseg // nbatch
    h = lp.PbHandle(nant=nant, nbit=nbit, npol=2, rfi_mode=rfi_mode, rows_per_seg=R, max_seg=per, keep_ave=keep_ave,
                    inject_frb=inject, nsets=nsets, coherence=coherence)
    codes = {0: [], 1: []}
    aves = {0: [], 1: []}
    pend = []

    def collect(b, s):
        h.select_set(s)
        for a in range(nant):
            o = h.fetch(a, 0, per, ave=keep_ave)
            if a == 0:
                codes[0].append(o["raw"]); codes[1].append(o["kur"])
                aves[0].append(o["ave_raw"]); aves[1].append(o["ave_kur"])
            else:
                assert np.array_equal(o["raw"], codes[0][-1]) and np.array_equal(o["kur"], codes[1][-1])

    for b in range(nbatch):
        s = b % nsets
        h.select_set(s)
        for a in range(nant):
            for i in range(per):
                h.submit_planar(a, i, data[b * per + i, 0], data[b * per + i, 1])
        h.process(per, inject_now=(1 + b * per) if inject else 0)
        pend.append((b, s))
        if len(pend) >= nsets:
            collect(*pend.pop(0))
    while pend:
        collect(*pend.pop(0))
    h.close()
    return ({k: np.concatenate(v) for k, v in codes.items()},
            {k: (np.concatenate(v) if keep_ave else None) for k, v in aves.items()})


def _streams(rfi_mode):
    return (0,) if rfi_mode == 0 else (1,) if rfi_mode == 1 else (0, 1)


def _aabb(codes, R, nbit, nseg):
    """coherence codes -> the AA, BB half of every time sample, as npol = 2 lays it out"""
    b = NCO * nbit // 8
    return codes.reshape(nseg * R // 8, 4, b)[:, :2].ravel()


@pytest.mark.parametrize("rfi_mode", [0, 1, 2])
@pytest.mark.parametrize("nbit", [8, 4, 2])
def test_aa_bb_are_the_npol2_bytes(rfi_mode, nbit):
    lp = libpb()
    R, nseg = 16, 3
    data = make_input(31 + rfi_mode, R, nseg)          # flagged, fully flagged and dropped-data rows
    for inject in (False, True):
        c2, _ = _run(lp, data, R, rfi_mode, nbit, False, inject=inject, keep_ave=False)
        c4, _ = _run(lp, data, R, rfi_mode, nbit, True, inject=inject, keep_ave=False)
        for st in _streams(rfi_mode):
            assert c4[st].size == 2 * c2[st].size
            assert np.array_equal(_aabb(c4[st], R, nbit, nseg), c2[st]), (st, inject)


@pytest.mark.parametrize("rfi_mode,nbit,R,nseg,inject", [
    (2, 8, 16, 3, False), (2, 4, 8, 3, True), (2, 2, 72, 2, False), (0, 8, 24, 3, True), (1, 8, 40, 2, False),
    (1, 2, 32, 3, True), (0, 4, 64, 2, False)])
def test_cr_ci_bit_exact_vs_cpu_reference(oracle, rfi_mode, nbit, R, nseg, inject):
    lp = libpb()
    data = make_input(7 + R, R, nseg)
    delays = oracle.set_frb_delays(80.0, R) if inject else None
    ref = CR.run(oracle, data, R, rfi_mode, nbit, delays, 1 if inject else 0)
    codes, aves = _run(lp, data, R, rfi_mode, nbit, True, inject=inject)
    # the restated recurrence is the oracle's: AA, BB planes = orc_segment's npol = 2 planes
    res, _, _ = oracle_run(oracle, data, R, rfi_mode=rfi_mode, npol=2, nbit=nbit, frb_delays=delays,
                           inject_now=1 if inject else 0)
    for st in _streams(rfi_mode):
        rc, rp = ref[st]
        orc = np.stack([compact_ave(r.ave_kur if st else r.ave_raw, R, 2).reshape(2, R // 8, NCO) for r in res])
        assert np.array_equal(rp[:, :2].view(np.uint32), orc.view(np.uint32)), st
        got = aves[st].reshape(nseg, 4, R // 8, NCO)
        assert np.array_equal(got.view(np.uint32), rp.view(np.uint32)), (st, np.argwhere(got != rp)[:5])
        assert np.array_equal(codes[st], rc), st


def test_cr_ci_one_full_second(oracle):
    """one second of one antenna: ten 1024-row segments in one batch, the bandpass carried across them"""
    lp = libpb()
    R, nseg = 1024, 10
    data = make_input(101, R, nseg)
    ref = CR.run(oracle, data, R, 2, 8)
    codes, aves = _run(lp, data, R, 2, 8, True)
    for st in (0, 1):
        assert np.array_equal(aves[st].reshape(nseg, 4, R // 8, NCO).view(np.uint32), ref[st][1].view(np.uint32)), st
        assert np.array_equal(codes[st], ref[st][0]), st


@pytest.mark.parametrize("nsets,nant", [(1, 1), (2, 1), (3, 1), (2, 2)])
def test_pipelining_gives_the_same_bytes(nsets, nant):
    lp = libpb()
    R, nseg = 32, 6
    data = make_input(55, R, nseg)
    base, _ = _run(lp, data, R, 2, 8, True, keep_ave=False, nbatch=nseg)
    got, _ = _run(lp, data, R, 2, 8, True, keep_ave=False, nsets=nsets, nbatch=nseg // 2 if nant > 1 else nseg,
                  nant=nant)
    if nant > 1:
        base, _ = _run(lp, data, R, 2, 8, True, keep_ave=False, nbatch=nseg // 2)
    for st in (0, 1):
        assert np.array_equal(got[st], base[st]), st


def _noise(seed, n, sigma=10.0):
    return np.random.default_rng(seed).normal(0, sigma, n)


def _u8(x):
    return np.clip(np.rint(x) + 128, 1, 255).astype(np.uint8)


def test_identical_pols_give_zero_ci():
    lp = libpb()
    R, nseg = 32, 2
    data = make_input(3, R, nseg, rfi=False, dropped=False)
    data[:, 1] = data[:, 0]
    _, aves = _run(lp, data, R, 2, 8, True)
    for st in (0, 1):
        p = aves[st].reshape(nseg, 4, R // 8, NCO)
        assert np.all(p[:, 3] == 0.0), st
        assert np.array_equal(p[:, 0], p[:, 1])


def test_swapping_pols_swaps_aa_bb_and_negates_ci():
    lp = libpb()
    R, nseg = 32, 3
    data = make_input(9, R, nseg)
    sw = np.ascontiguousarray(data[:, ::-1])
    _, a = _run(lp, data, R, 2, 8, True)
    _, b = _run(lp, sw, R, 2, 8, True)
    for st in (0, 1):
        p = a[st].reshape(nseg, 4, R // 8, NCO)
        q = b[st].reshape(nseg, 4, R // 8, NCO)
        assert np.array_equal(p[:, 0], q[:, 1]) and np.array_equal(p[:, 1], q[:, 0]), st
        assert np.array_equal(p[:, 2].view(np.uint32), q[:, 2].view(np.uint32)), st
        assert np.array_equal(p[:, 3], -q[:, 3]), st


def test_noise_statistics_full_size():
    lp = libpb()
    R, nseg = 1024, 2
    n = R * 12500
    data = np.empty((nseg, 2, n), np.uint8)
    for s in range(nseg):
        for p in range(2):
            data[s, p] = _u8(_noise(1000 + 2 * s + p, n))
    _, aves = _run(lp, data, R, 2, 8, True)
    for st in (0, 1):
        p = aves[st].reshape(nseg, 4, R // 8, NCO)[1:]         # past the bandpass initialisation
        sa = p[:, 0].std()
        for k in (2, 3):
            assert abs(p[:, k].mean()) < 0.02, (st, k, p[:, k].mean())
            assert abs(p[:, k].std() / sa - 1) < 0.05, (st, k, p[:, k].std(), sa)


def test_correlated_pols_give_positive_cr():
    lp = libpb()
    R, nseg = 64, 2
    n = R * 12500
    data = np.empty((nseg, 2, n), np.uint8)
    for s in range(nseg):
        a = _noise(500 + s, n)
        data[s, 0] = _u8(a)
        data[s, 1] = _u8(a + _noise(900 + s, n))
    _, aves = _run(lp, data, R, 2, 8, True)
    for st in (0, 1):
        p = aves[st].reshape(nseg, 4, R // 8, NCO)
        assert p[:, 2].mean() > 0.5, (st, p[:, 2].mean())
        assert abs(p[:, 3].mean()) < 0.05, (st, p[:, 3].mean())
