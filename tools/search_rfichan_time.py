"""What the cleaning's channel stage costs at heimdall's production flags (tools/search_rfi_time.py's gulp: 30 720 samples
of 4096 channels, the tolerance-spaced trial DMs 2-1000, boxcars up to 64, the edge zaps, a 2-s running baseline, the peak
list at S/N 6 from page-locked host memory).  The block is noise with one channel in sixteen at four times the spread, so
the stage has 232 channels to find and fill.  In one process on one card:
  * the gulp with the stage never switched on, through the C ABI directly, for this tree's library and -- with --parent
    PATH -- for another libpb_hip.so (the parent commit's, built in a separate worktree), in alternating rounds: never
    switched on both launch the same kernels, and this tree's median is expected inside the parent's minimum .. maximum
    (recorded as never_on_within_parent_spread);
  * on one Searcher, the stage off and on in alternation: median wall ms per gulp each way, the stage's device ms
    (pb_search_rfi_chan_info) and its share of the gulp;
  * the same with the narrow and broad passes on as well, and their device ms (pb_search_rfi_info) beside the stage's.
Prints one JSON line.

    python tools/search_rfichan_time.py [--reps 20] [--parent /path/to/parent/libpb_hip.so] [--out profiles/search_rfichan_time.json]"""
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="the parent commit's libpb_hip.so")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, nchan = search.HEIMDALL_GULP, 4096
    rng = np.random.default_rng(3)
    pinned = torch.empty((T, nchan), dtype=torch.uint8, pin_memory=True)
    codes = pinned.numpy()
    sig = np.full(nchan, 1 / 0.02957 / 4)
    sig[8::16] *= 4
    for t in range(0, T, 1024):                            # (in slices: the doubles of a whole gulp are 1 GB)
        codes[t:t + 1024] = np.clip(rng.standard_normal((min(1024, T - t), nchan)) * sig + 127.5, 0, 255).astype(np.uint8)
    dml = search.dedisp_dm_list(2.0, 1000.0, search.TSAMP, search.FCH1, search.FOFF, nchan)
    per = max(2, -(-6 // a.rounds))
    this, parent = [], []
    for _ in range(a.rounds):
        t, ndm, tout = CT.gulp_times_other(libpb.LIB_PATH, codes, dml, per)
        this += t
        if a.parent:
            parent += CT.gulp_times_other(a.parent, codes, dml, per)[0]
    res = dict(what="search gulp with and without the cleaning's channel stage", gpu=torch.cuda.get_device_name(0), nchan=nchan,
               nsamp=T, tout=tout, ndm=ndm, boxcar_max=search.HEIMDALL_BOXCAR_MAX, zap=search.HEIMDALL_ZAP,
               baseline_samples=int(2.0 / search.TSAMP), reps=a.reps, ms_per_gulp_never_on=CT.spread(this))
    if a.parent:
        res["parent_library"] = dict(ms_per_gulp=CT.spread(parent))
        res["never_on_median_minus_parent_median_ms"] = round(float(np.median(this) - np.median(parent)), 4)
        res["never_on_within_parent_spread"] = bool(min(parent) <= np.median(this) <= max(parent))
    with search.Searcher(max_samples=T, dm_list=dml) as s:
        s.set_baseline(int(2.0 / search.TSAMP))
        for name, rfi in (("stage_alone", False), ("with_narrow_and_broad", True)):
            s.set_rfi(rfi, rfi)
            wall = {"off": [], "on": []}
            stages, chan_ms, rfi_ms, info = [], [], [], None
            for rep in range(a.reps + 2):                   # the first two rounds warm up
                for mode in ("off", "on"):
                    s.set_rfi_chan(tol=4.0 if mode == "on" else 0.0)
                    t0 = time.perf_counter()
                    s.peaks(codes, 6.0)
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep < 2:
                        continue
                    wall[mode].append(dt)
                    if mode == "on":
                        info = s.rfi_chan_info()
                        chan_ms.append(info["ms"])
                        rfi_ms.append(s.rfi_info()["ms"])
                        stages.append(s.timers())
            off, on = float(np.median(wall["off"])), float(np.median(wall["on"]))
            res[name] = dict(ms_per_gulp_off=CT.spread(wall["off"]), ms_per_gulp_on=CT.spread(wall["on"]),
                             chan_device_ms=CT.spread(chan_ms), chan_share_of_gulp=round(float(np.median(chan_ms)) / off, 5),
                             wall_increase=round(on / off - 1.0, 5), nflag=info["nflag"],
                             narrow_broad_device_ms=CT.spread(rfi_ms) if rfi else None,
                             stage_ms_on={k: round(float(np.median([d[k] for d in stages])), 4) for k in stages[0]})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
