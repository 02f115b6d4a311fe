"""The seeded inputs of the refinement's GPU test (tests/test_gpu_search_refine.py), kept apart so that
tests/test_search_refine_cpu.py can run the restatement over the very same inputs without a GPU: it asserts there that
at most 1 % of the requests are near-ties of the DM pass (the only requests whose kbest the GPU test may leave out)."""
import numpy as np

import search_refine_ref as R
import search_rfi_ref as P
import search_stats_ref as S

F32 = np.float32
TSAMP = float(F32(12500.0 / 128e6 * 8))
FCH1 = float(F32(361.94))
NEAR_TIE_CAP = 0.01

# nbit, nchan, zap, DM list?, tout, (nstep, H, wmax), cleaned
CASES = [
    (8, 64, (), False, 1000, (8, 128, 32), False),
    (4, 64, ((0, 3), (60, 64)), True, 777, (8, 64, 32), False),        # windows at the block's ends are too short
    (2, 200, ((60, 64),), False, 901, (5, 40, 8), False),
    (8, 256, ((70, 75),), True, 1030, (32, 128, 32), False),
    (4, 1024, ((0, 50), (1000, 1024)), False, 650, (8, 128, 32), False),
    (8, 4096, ((0, 190), (3900, 4096)), True, 600, (8, 128, 32), False),
    (8, 256, ((0, 10),), False, 1203, (8, 128, 32), True),
    (8, 64, ((8, 16), (20, 22)), False, 130, (8, 128, 32), False),        # the block shorter than a full window
]
LINEAR = dict(dm_min=0.0, dm_max=40.0, dm_step=4.0)
DMLIST = np.array([1.0, 3.5, 7.25, 12.0, 20.0, 33.0], np.float32)


def delays(dms, fch1, foff, nchan, tsamp=TSAMP):
    """the search's delays for DMs given as float64 and a band given as the interface's binary32 numbers"""
    f = float(F32(fch1)) + float(F32(foff)) * np.arange(nchan)
    return np.stack([np.floor(4.148808e3 * dm * (f ** -2 - f.max() ** -2) / float(F32(tsamp)) + 0.5).astype(np.int64) for dm in dms])


def geometry(case):
    nbit, nchan, zap, use_list, tout, geo, clean = CASES[case]
    foff = float(F32(-40.0 / nchan))
    dms = DMLIST.astype(np.float64) if use_list else LINEAR["dm_min"] + LINEAR["dm_step"] * np.arange(11)
    zapped = np.zeros(nchan, bool)
    for lo, hi in zap:
        zapped[lo:hi] = True
    d = delays(dms, FCH1, foff, nchan)
    kw = dict(nchan=nchan, fch1=FCH1, foff=foff, tsamp=TSAMP, boxcar_max=16, zap=zap)
    kw.update(dict(dm_list=DMLIST) if use_list else LINEAR)
    return kw, dms, zapped, int(d[:, ~zapped].max())


def length(case):
    """(tout, T) of a case's block: T = tout + the largest delay, never a multiple of 64"""
    tout = CASES[case][4]
    maxd = geometry(case)[3]
    if (tout + maxd) % 64 == 0:
        tout += 1
    return tout, tout + maxd


def codes(case, T):
    """[T][nchan] codes: noise about mid-range and a dispersed 3-sample pulse at DM 9.3 near a third of the block"""
    nbit, nchan, zap, use_list, tout, geo, clean = CASES[case]
    top = (1 << nbit) - 1
    rng = np.random.default_rng(4100 + case)
    g = rng.standard_normal((T, nchan)) * (33.8 * top / 255.0) + top / 2.0
    foff = float(F32(-40.0 / nchan))
    d = delays([9.3], FCH1, foff, nchan)[0]
    t0 = tout // 3
    for c in range(nchan):
        g[t0 + d[c]:t0 + d[c] + 3, c] += 0.6 * top / 4.0
    if clean:
        g[tout // 2, :] += top                                           # a broadband impulse for the cleaning to remove
    return np.clip(np.floor(g + 0.5), 0, top).astype(np.uint8)


def requests(case, dms):
    """(t_pk, width, dm_lo, dm_step) per request: windows at both block edges, the pulse, even and odd widths, trials
    that leave the grid at either end.  dm_lo and dm_step are multiples of 2^-6 below 64, so every fine DM is a binary32
    number and a second Searcher can take the fine trials as its DM list."""
    nbit, nchan, zap, use_list, tout, (nstep, H, wmax), clean = CASES[case]
    rng = np.random.default_rng(4200 + case)
    last = float(dms[-1])
    step = 0.125 if nstep <= 8 else 0.03125
    pts = [(0, 1, 8.5), (tout - 1, 2, 8.0), (tout // 3 + 1, 3, 9.3 - step * nstep / 2), (H - 1, wmax, 2.0),
           (max(tout - H, 0), 4, last - step * (nstep // 2)),            # the upper trials are above the grid
           (tout // 2, 5, -step * (nstep // 2)),                         # the lower trials are below 0
           (tout // 3, 1, last + 1.0)]                                   # every trial above the grid
    pts += [(int(rng.integers(0, tout)), int(rng.integers(1, wmax + 1)), float(rng.integers(0, int(last * 0.9) * 64)) / 64.0)
            for _ in range(5)]
    return [(t, w, float(np.round(lo * 64) / 64), step) for t, w, lo in pts]


def restate(case, xt, tout, dms):
    """the restatement's answer for every request of a case from the block the search saw -> list of dicts (R.refine's,
    plus series: the ABI's [nstep][2 (H + M)] window)"""
    nbit, nchan, zap, use_list, _, (nstep, H, wmax), clean = CASES[case]
    kw, _, zapped, _ = geometry(case)
    chans = np.nonzero(~zapped)[0]
    out = []
    for t, w, lo, st in requests(case, dms):
        fine = R.trial_dms(lo, st, nstep)
        valid = (fine >= 0) & (fine <= float(dms[-1]))
        d = delays(np.where(valid, fine, 0.0), FCH1, kw["foff"], nchan)
        q = R.fine_series(xt, chans, d, tout)
        q[~valid] = 0
        r = R.refine(q, valid, t, w, H, wmax)
        r["series"] = R.series_window(q, t, H, wmax // 2) * (0 if r["status"] else 1)
        r["fine"], r["valid"] = fine, valid
        out.append(r)
    return out


def cleaned_block(xt, zapped, tol=5.0, boxcar_max=16):
    """the block after the search's default RFI cleaning (Searcher.set_rfi(True, True), no running baseline), by the
    restatements of tests/search_rfi_ref.py and tests/search_stats_ref.py: narrow pass, then the broad pass with the
    zero-DM series' level and rms rounded to binary32"""
    chans = np.nonzero(~zapped)[0]
    xa, _, meds = P.narrow(np.ascontiguousarray(xt), chans, tol)
    z = P.zero_dm(xa, chans)
    lvl, rms, _ = S.series_stats(z.astype(np.int64), 0)
    nbox = int(np.log2(boxcar_max)) + 1
    best, bw = P.zero_dm_snr(z, np.float32(lvl), np.float32(rms), nbox, 0)
    return P.apply_broad(xa, chans, meds, P.broad_flags(best, bw, tol))


def offgrid_inputs():
    """a reduced geometry with a strong 2-sample pulse at DM 35.0 between the grid's 32 and 40 (shared with the GPU test)"""
    nchan, tout, dm_true, t0 = 256, 1500, 35.0, 700
    foff = float(np.float32(-40.0 / nchan))
    dms = 8.0 * np.arange(11)
    maxd = int(delays(dms, FCH1, foff, nchan).max())
    rng = np.random.default_rng(77)
    g = rng.standard_normal((tout + maxd, nchan)) * 33.8 + 127.5
    d = delays([dm_true], FCH1, foff, nchan)[0]
    for c in range(nchan):
        g[t0 + d[c]:t0 + d[c] + 2, c] += 60.0
    x = np.clip(np.floor(g + 0.5), 0, 255).astype(np.uint8)
    kw = dict(nchan=nchan, fch1=FCH1, foff=foff, tsamp=TSAMP, boxcar_max=64, zap=(), dm_min=0.0, dm_max=80.0, dm_step=8.0)
    return x, kw, dms, dm_true, t0, tout


def two_pass(xt, chans, tout, dms, fch1, foff, nchan, dmi, t, width_log2, nstep=32, H=128, wmax=32, tsamp=TSAMP):
    """Searcher.refine's sequence on the restatement -> (dict like Searcher.refine's, with the S/N bounds: snr_err and a
    third array in each of trials; pass-1 step)"""
    gaps = [abs(dms[j] - dms[dmi]) for j in (dmi - 1, dmi + 1) if 0 <= j < len(dms)]
    span, width = max(gaps), min(1 << width_log2, wmax)
    lo, st = dms[dmi] - span, 2.0 * span / (nstep - 1)
    trials = []
    for p in range(2):
        fine = R.trial_dms(lo, st, nstep)
        valid = (fine >= 0) & (fine <= dms[-1])
        q = R.fine_series(xt, chans, delays(np.where(valid, fine, 0.0), fch1, foff, nchan, tsamp), tout,
                          t - H - wmax, t + H + wmax)
        q[~valid] = 0
        r = R.refine(q, valid, t, width, H, wmax)
        trials.append((fine, r["sn_dm"], r["err_dm"]))
        if p == 0:
            st1 = float(np.float32(st))
            lo, st = fine[r["kbest"]] - 2.0 * st1, 4.0 * st1 / (nstep - 1)
    iw = int(np.argmax(r["opt_sn"]))
    return dict(dm=float(fine[r["kbest"]]), snr=float(r["sn_dm"][r["kbest"]]), snr_err=float(r["err_dm"][r["kbest"]]), width=int(2 * iw + 1),
                peak=int(max(0, t - H) + r["opt_loc"][iw]), trials=trials, opt_sn=r["opt_sn"], opt_loc=r["opt_loc"]), st1
