"""What the polarisation stage costs the search at heimdall's production flags (tools/search_rfi_time.py's gulp: 30 720
samples of 4096 channels, the tolerance-spaced trial DMs 2-1000, boxcars up to 64, the edge zaps, a 2-s running baseline,
the peak list at S/N 6 from page-locked host memory).  In one process on one card, medians after discarded first gulps:
  * the 1-IF gulp with the stage never switched on, through the C ABI directly, for this tree's library and -- with
    --parent PATH -- for another libpb_hip.so (the parent commit's, built in a separate worktree), in alternating rounds:
    never switched on both launch the same kernels, and this tree's median is expected inside the parent's
    minimum .. maximum (recorded as never_on_within_parent_spread);
  * through Searcher.peaks, alternating: the 1-IF gulp on a Searcher without the stage and the four-product gulp
    [nsamp][4][nchan] on one with it -- wall ms of each, and the device ms of k_transpose_codes and of k_transpose_pol
    (the transpose stage of pb_search_timers);
  * on the Searcher with the stage on, 32 requests spread over the block with 2001 trial RMs: the device time of
    pb_search_pol's kernels, of the kernels with the copy to the host, and the wall time of the call.
Prints one JSON line.

    python tools/search_pol_time.py [--reps 20] [--parent /path/to/parent/libpb_hip.so] [--out profiles/search_pol_time.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import torch  # noqa: E402  (page-locked host memory)
import search_cutout_time as CT  # noqa: E402  (the gulp through a library bound by hand)

search = importlib.import_module("vlite-fast_amd.search")
libpb = importlib.import_module("vlite-fast_amd.libpb")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent", default=None, help="the parent commit's libpb_hip.so")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, nchan, nreq = search.HEIMDALL_GULP, 4096, 32
    rng = np.random.default_rng(3)
    pinned4 = torch.empty((T, 4, nchan), dtype=torch.uint8, pin_memory=True)
    codes4 = pinned4.numpy()
    for k in range(4):
        codes4[:, k] = np.clip(rng.normal(127.5, 1 / 0.02957, (T, nchan)), 0, 255).astype(np.uint8)
    pinned = torch.empty((T, nchan), dtype=torch.uint8, pin_memory=True)
    codes = pinned.numpy()
    codes[:] = (codes4[:, 0].astype(np.uint16) + codes4[:, 1] + 1) >> 1          # the block that the stage searches
    dml = search.dedisp_dm_list(2.0, 1000.0, search.TSAMP, search.FCH1, search.FOFF, nchan)
    per = max(1, a.reps // a.rounds)
    this, parent = [], []
    for _ in range(a.rounds):
        t, ndm, tout = CT.gulp_times_other(libpb.LIB_PATH, codes, dml, per)
        this += t
        if a.parent:
            parent += CT.gulp_times_other(a.parent, codes, dml, per)[0]
    res = dict(what="search gulp on a four-product block, and the polarisation of 32 candidates",
               gpu=torch.cuda.get_device_name(0), nchan=nchan, nsamp=T, tout=tout, ndm=ndm,
               boxcar_max=search.HEIMDALL_BOXCAR_MAX, zap=search.HEIMDALL_ZAP, baseline_samples=int(2.0 / search.TSAMP),
               reps=per * a.rounds, rounds=a.rounds, ms_per_gulp_never_on=CT.spread(this))
    if a.parent:
        res["parent_library"] = dict(ms_per_gulp=CT.spread(parent))
        res["never_on_median_minus_parent_median_ms"] = round(float(np.median(this) - np.median(parent)), 4)
        res["never_on_within_parent_spread"] = bool(min(parent) <= np.median(this) <= max(parent))
    with search.Searcher(max_samples=T, dm_list=dml) as s1, search.Searcher(max_samples=T, dm_list=dml) as s4:
        for s in (s1, s4):
            s.set_baseline(int(2.0 / search.TSAMP))
        s4.set_pol(max_cands=nreq)
        off_len, guard, (rm_lo, rm_step, nrm), _ = s4._pol
        w1, w4, tr1, tr4, h1, h4 = [], [], [], [], [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            p1 = s1.peaks(codes, 6.0)
            t1 = time.perf_counter()
            p4 = s4.peaks(codes4, 6.0)
            t2 = time.perf_counter()
            if rep >= 1:
                w1.append((t1 - t0) * 1e3)
                w4.append((t2 - t1) * 1e3)
                tr1.append(s1.timers()["transpose"])
                tr4.append(s4.timers()["transpose"])
                h1.append(s1.timers()["h2d"])
                h4.append(s4.timers()["h2d"])
        assert p1["total"] == p4["total"] and abs(s4.pol_timers()["transpose"] - tr4[-1]) < 1e-6
        res["gulp_through_searcher"] = dict(
            one_if=dict(wall_ms=CT.spread(w1), h2d_ms=CT.spread(h1), k_transpose_codes_ms=CT.spread(tr1), bytes_in=T * nchan,
                        bytes_out=T * nchan),
            four_products=dict(wall_ms=CT.spread(w4), h2d_ms=CT.spread(h4), k_transpose_pol_ms=CT.spread(tr4),
                               bytes_in=4 * T * nchan, bytes_out=5 * T * nchan))
        res["pol_gulp_minus_one_if_gulp_ms"] = round(float(np.median(w4) - np.median(w1)), 4)
        if a.parent:
            res["pol_gulp_minus_parent_gulp_ms"] = round(float(np.median(w4) - np.median(parent)), 4)
        dmi = np.linspace(40, ndm - 40, nreq).astype(int)
        tpk = np.linspace(2000, tout - 2000, nreq).astype(int)
        wid = 1 << (np.arange(nreq) % 7)
        dev, cp, wall = [], [], []
        for rep in range(a.reps + 1):
            t1 = time.perf_counter()
            r = s4.pol(dmi, tpk, wid)
            t2 = time.perf_counter()
            if rep >= 1:
                tm = s4.pol_timers()
                dev.append(tm["kernels"])
                cp.append(tm["with_copy"])
                wall.append((t2 - t1) * 1e3)
        assert (r["kbest"] >= 0).all() and (r["summary"][:, 0] == 4096 - 190 - 196).all()
        res["pol"] = dict(requests=nreq, nrm=nrm, rm_lo=rm_lo, rm_step=rm_step, off_len=off_len, guard=guard,
                          device_ms_kernels=CT.spread(dev), device_ms_with_copy=CT.spread(cp), wall_ms_call=CT.spread(wall))
        res["pol_share_of_gulp"] = round(float(np.median(dev)) / float(np.median(w4)), 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
