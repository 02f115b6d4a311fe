"""What refining candidates costs the search at heimdall's production flags (tools/search_rfi_time.py's gulp: 30 720
samples of 4096 channels, the tolerance-spaced trial DMs 2-1000, boxcars up to 64, the edge zaps, a 2-s running baseline,
the peak list at S/N 6 from page-locked host memory).  In one process on one card:
  * the gulp with refinement never switched on, through the C ABI directly, for this tree's library and -- with
    --parent PATH -- for another libpb_hip.so (the parent commit's, built in a separate worktree), in alternating rounds:
    median, minimum and maximum wall ms of each; never switched on both launch the same kernels, and this tree's median
    is expected inside the parent's minimum .. maximum (recorded as never_on_within_parent_spread);
  * on a Searcher with refinement on (default geometry: 32 fine trials, half window 128, widths below 32), 32 requests
    spread over the block: the device time of pb_search_refine's kernels, of the kernels with the copy to the host, and
    the wall time of the call.
Prints one JSON line.

    python tools/search_refine_time.py [--reps 20] [--parent /path/to/parent/libpb_hip.so] [--out profiles/search_refine_time.json]"""
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
    pinned = torch.empty((T, nchan), dtype=torch.uint8, pin_memory=True)
    codes = pinned.numpy()
    codes[:] = np.clip(rng.normal(127.5, 1 / 0.02957, (T, nchan)), 0, 255).astype(np.uint8)
    dml = search.dedisp_dm_list(2.0, 1000.0, search.TSAMP, search.FCH1, search.FOFF, nchan)
    per = max(1, a.reps // a.rounds)
    this, parent = [], []
    for _ in range(a.rounds):
        t, ndm, tout = CT.gulp_times_other(libpb.LIB_PATH, codes, dml, per)
        this += t
        if a.parent:
            parent += CT.gulp_times_other(a.parent, codes, dml, per)[0]
    res = dict(what="search gulp and refinement of 32 candidates", gpu=torch.cuda.get_device_name(0), nchan=nchan, nsamp=T,
               tout=tout, ndm=ndm, boxcar_max=search.HEIMDALL_BOXCAR_MAX, zap=search.HEIMDALL_ZAP,
               baseline_samples=int(2.0 / search.TSAMP), reps=per * a.rounds, rounds=a.rounds,
               ms_per_gulp_never_on=CT.spread(this))
    if a.parent:
        res["parent_library"] = dict(ms_per_gulp=CT.spread(parent))
        res["never_on_median_minus_parent_median_ms"] = round(float(np.median(this) - np.median(parent)), 4)
        res["never_on_within_parent_spread"] = bool(min(parent) <= np.median(this) <= max(parent))
    with search.Searcher(max_samples=T, dm_list=dml) as s:
        s.set_baseline(int(2.0 / search.TSAMP))
        s.set_refine(max_cands=nreq)
        nstep, H, wmax, _ = s._ref
        dmi = np.linspace(40, ndm - 40, nreq).astype(int)
        tpk = np.linspace(2000, tout - 2000, nreq).astype(int)
        plan = [s.refine_plan(int(d), 2) for d in dmi]
        width, lo, st = [np.array(v) for v in zip(*plan)]
        dev, cp, wall = [], [], []
        for rep in range(a.reps + 2):
            s.peaks(codes, 6.0)
            t1 = time.perf_counter()
            r = s.refine_raw(tpk, width, lo, st)
            t2 = time.perf_counter()
            if rep >= 2:
                tm = s.refine_timers()
                dev.append(tm["kernels"])
                cp.append(tm["with_copy"])
                wall.append((t2 - t1) * 1e3)
        assert not r["status"].any() and (r["kbest"] >= 0).all()
        nact = nchan - sum(hi - lo_ for lo_, hi in search.HEIMDALL_ZAP)
        byt = nreq * nstep * nact * 2 * (H + wmax // 2)
        res["refine"] = dict(requests=nreq, nstep=nstep, half_window=H, wmax=wmax, bytes_summed=byt,
                             device_ms_kernels=CT.spread(dev), device_ms_with_copy=CT.spread(cp), wall_ms_call=CT.spread(wall))
        res["refine_share_of_gulp"] = round(float(np.median(dev)) / float(np.median(this)), 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
