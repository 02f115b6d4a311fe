"""What the periodicity search costs at heimdall's production flags, on noise: 4096 channels, a gulp of 30 720 new samples
searched with the max_delay + 63 samples before it (the block that search.py makes for -nsamps_gulp 30720), the
tolerance-spaced trial DMs 2-1000, boxcars up to 64, the edge zaps, a 2-s running baseline, and -periodic 0.05 3.2
-periodic_bins 64 (octaves 0 .. 6).  In one process on one card, after a discarded first gulp: the device times of the gulp's
search (pb_search_timers) and of the stage (pb_search_periodic_timers: folding, last stage + evaluation, everything with the
copy), the stage's wall time, and all of it against the 24 s that a gulp spans.  Prints one JSON line.

    python tools/search_periodic_time.py [--reps 3] [--bins 64] [--periods 0.05 3.2] [--dm-chunk 0] [--out profiles/periodic_steptime.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import torch  # noqa: E402  (page-locked host memory, the card's name)

search = importlib.import_module("vlite-fast_amd.search")


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(min(v)), 4), max=round(float(max(v)), 4), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed gulps, after one that is left out")
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--periods", nargs=2, type=float, default=[0.05, 3.2])
    ap.add_argument("--dm-chunk", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gulp, nchan = search.HEIMDALL_GULP, 4096
    dml = search.dedisp_dm_list(2.0, 1000.0, search.TSAMP, search.FCH1, search.FOFF, nchan)
    k_lo, k_hi = search.periodic_octaves(a.periods[0], a.periods[1], a.bins, search.TSAMP)
    with search.Searcher(max_samples=gulp + 20000, dm_list=dml) as s:
        T = gulp + s.max_delay + 63
        rng = np.random.default_rng(3)
        pinned = torch.empty((T, nchan), dtype=torch.uint8, pin_memory=True)
        codes = pinned.numpy()
        for t0 in range(0, T, 4096):
            g = rng.standard_normal((min(4096, T - t0), nchan), dtype=np.float32)
            codes[t0:t0 + g.shape[0]] = np.clip(127.5 + g / 0.02957, 0, 255).astype(np.uint8)
        s.set_baseline(int(2.0 / search.TSAMP))
        s.set_periodic(a.bins, k_lo, k_hi, dm_chunk=a.dm_chunk)
        wg, ws, dev, core = [], [], [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            pk = s.peaks(codes, 6.0)
            t1 = time.perf_counter()
            tab = s.periodic()
            t2 = time.perf_counter()
            if rep >= 1:
                wg.append((t1 - t0) * 1e3)
                ws.append((t2 - t1) * 1e3)
                dev.append(s.periodic_timers())
                core.append(s.timers())
        span = gulp * search.TSAMP * 1e3
        d = {k: spread([x[k] for x in dev]) for k in ("fold", "eval", "with_copy")}
        c = {k: spread([x[k] for x in core]) for k in core[0]}
        res = dict(what="search gulp, and the periodicity search of the same block's series, on noise",
                   gpu=torch.cuda.get_device_name(0), nchan=nchan, nact=s.nact, nsamp=T, tout=pk["tout"], ndm=s.ndm,
                   boxcar_max=search.HEIMDALL_BOXCAR_MAX, zap=search.HEIMDALL_ZAP, baseline_samples=int(2.0 / search.TSAMP),
                   bins=a.bins, periods_s=a.periods, octaves=[k_lo, k_hi], dm_chunk=a.dm_chunk, stages="one launch per stage",
                   reps=a.reps, entries=int(tab["snr"].size), skipped=int((tab["i"] < 0).sum()),
                   trials=int(tab["M"].astype(np.int64).sum()), largest_snr_on_noise=round(float(tab["snr"].max()), 4),
                   search_device_ms=c, search_wall_ms=spread(wg), periodic_device_ms=d, periodic_wall_ms=spread(ws),
                   gulp_span_ms=round(span, 1), periodic_over_span=round(d["with_copy"]["median"] / span, 6),
                   gulp_plus_stage_over_span=round(float(np.median(wg) + np.median(ws)) / span, 6))
        res["keeps_up_with_the_stream"] = bool(res["gulp_plus_stage_over_span"] < 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
