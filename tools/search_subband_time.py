"""What the sub-band search costs at heimdall's production flags (tools/search_rfi_time.py's gulp: 30 720 samples of 4096
channels, the tolerance-spaced trial DMs 2-1000, boxcars up to 64, the edge zaps, a 2-s running baseline, the peak list at
S/N 6 from page-locked host memory), with 8 base sub-bands and the 18 bands of search.subband_list(8).  In one process on one
card, medians after a discarded first gulp, with the spread:
  * the gulp with the stage never switched on, through the C ABI directly, for this tree's library and -- with --parent
    PATH -- for another libpb_hip.so (the parent commit's, built in a separate worktree), in alternating rounds: never
    switched on both launch the same kernels, and this tree's median is expected inside the parent's minimum .. maximum
    (recorded as never_on_within_parent_spread);
  * on a Searcher with the stage on: the wall time of the gulp (Searcher.peaks), of the stage (Searcher.subbands at S/N 7
    over the whole block) and the stage's four device times (pb_search_subband_timers), with each kernel group's share;
  * gulp plus stage against the 24 s that a gulp spans.
Prints one JSON line.

    python tools/search_subband_time.py [--reps 6] [--parent /path/to/parent/libpb_hip.so] [--out profiles/search_subband_time.json]"""
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
    ap.add_argument("--reps", type=int, default=6, help="timed gulps (at least 5), after one that is left out")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nsb", type=int, default=8)
    ap.add_argument("--dm-chunk", type=int, default=0)
    ap.add_argument("--parent", default=None, help="the parent commit's libpb_hip.so")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.reps = max(a.reps, 5)
    T, nchan = search.HEIMDALL_GULP, 4096
    rng = np.random.default_rng(3)
    pinned = torch.empty((T, nchan), dtype=torch.uint8, pin_memory=True)
    codes = pinned.numpy()
    codes[:] = np.clip(rng.normal(127.5, 1 / 0.02957, (T, nchan)), 0, 255).astype(np.uint8)
    dml = search.dedisp_dm_list(2.0, 1000.0, search.TSAMP, search.FCH1, search.FOFF, nchan)
    per = max(2, -(-a.reps // a.rounds))
    this, parent = [], []
    for _ in range(a.rounds):
        t, ndm, tout = CT.gulp_times_other(libpb.LIB_PATH, codes, dml, per)
        this += t
        if a.parent:
            parent += CT.gulp_times_other(a.parent, codes, dml, per)[0]
    bands = search.subband_list(a.nsb)
    res = dict(what="search gulp, and the sub-band search of the same block", gpu=torch.cuda.get_device_name(0), nchan=nchan,
               nsamp=T, tout=tout, ndm=ndm, boxcar_max=search.HEIMDALL_BOXCAR_MAX, zap=search.HEIMDALL_ZAP,
               baseline_samples=int(2.0 / search.TSAMP), nsb=a.nsb, nbands=len(bands), reps=per * a.rounds, rounds=a.rounds,
               ms_per_gulp_never_on=CT.spread(this))
    if a.parent:
        res["parent_library"] = dict(ms_per_gulp=CT.spread(parent))
        res["never_on_median_minus_parent_median_ms"] = round(float(np.median(this) - np.median(parent)), 4)
        res["never_on_within_parent_spread"] = bool(min(parent) <= np.median(this) <= max(parent))
    with search.Searcher(max_samples=T, dm_list=dml) as s:
        s.set_baseline(int(2.0 / search.TSAMP))
        s.set_subbands(a.nsb, dm_chunk=a.dm_chunk)
        wg, ws, dev = [], [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            pk = s.peaks(codes, 6.0)
            t1 = time.perf_counter()
            sb = s.subbands(7.0)
            t2 = time.perf_counter()
            if rep >= 1:
                wg.append((t1 - t0) * 1e3)
                ws.append((t2 - t1) * 1e3)
                dev.append(s.subband_timers())
            main_dd = s.timers()["dedisperse"]
        assert pk["tout"] == tout and not sb["overflow"]
        keys = ("dedisperse", "stats", "boxcar", "with_copy")
        d = {k: CT.spread([x[k] for x in dev]) for k in keys}
        kern = sum(d[k]["median"] for k in keys[:3])
        res["stage"] = dict(points_at_7=sb["npoints"], wall_ms_gulp=CT.spread(wg), wall_ms_stage=CT.spread(ws),
                            device_ms=dict(k_dedisperse_sub=d["dedisperse"], band_sums_prefix_statistics=d["stats"],
                                           boxcars_best_band=d["boxcar"], with_copy=d["with_copy"]),
                            share_of_kernels={k: round(d[k]["median"] / kern, 4) for k in keys[:3]},
                            main_dedispersion_ms=round(main_dd, 4))
        total = float(np.median(wg) + np.median(ws))
        span = T * search.TSAMP * 1e3
        res["gulp_plus_stage_ms"] = round(total, 4)
        res["gulp_span_ms"] = round(span, 1)
        res["gulp_plus_stage_over_span"] = round(total / span, 6)
        res["keeps_up_with_the_stream"] = bool(total < span)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
