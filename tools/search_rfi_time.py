"""What RFI cleaning costs the search at heimdall's production flags: one 30 720-sample gulp of 4096 channels, the
tolerance-spaced trial DMs 2-1000, boxcars up to 64, the edge zaps, a 2-s running baseline, the peak list at S/N 6 from
page-locked host memory (tools/bench_search.py's case (b)).  Cleaning off and on alternate in one process on one
Searcher; prints one JSON line: median wall ms per gulp each way, the cleaning's device ms (pb_search_rfi_info), the
stage times, and the cleaning's share of the gulp.  The block is noise with a few broadband bursts and a noisy channel,
so both passes have something to do.

    python tools/search_rfi_time.py [--reps 20] [--out profiles/search_rfi_time.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402  (page-locked host memory)

search = importlib.import_module("vlite-fast_amd.search")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, nchan = search.HEIMDALL_GULP, 4096
    rng = np.random.default_rng(3)
    pinned = torch.empty((T, nchan), dtype=torch.uint8, pin_memory=True)
    codes = pinned.numpy()
    codes[:] = np.clip(rng.normal(127.5, 1 / 0.02957, (T, nchan)), 0, 255).astype(np.uint8)
    for t, w in ((5000, 2), (12000, 8), (20000, 1)):
        codes[t:t + w] = np.clip(codes[t:t + w].astype(np.int32) + 40, 0, 255).astype(np.uint8)
    codes[::7, 1000] = 255
    dml = search.dedisp_dm_list(2.0, 1000.0, search.TSAMP, search.FCH1, search.FOFF, nchan)
    wall = {"off": [], "on": []}
    stages = {"off": [], "on": []}
    rfi_ms, info = [], None
    with search.Searcher(max_samples=T, dm_list=dml) as s:
        s.set_baseline(int(2.0 / search.TSAMP))
        for rep in range(a.reps + 2):                       # the first two rounds warm up
            for mode in ("off", "on"):
                if mode == "on":
                    s.set_rfi()
                else:
                    s.set_rfi(False, False)
                t0 = time.perf_counter()
                s.peaks(codes, 6.0)
                dt = (time.perf_counter() - t0) * 1e3
                if rep < 2:
                    continue
                wall[mode].append(dt)
                stages[mode].append(s.timers())
                if mode == "on":
                    info = s.rfi_info()
                    rfi_ms.append(info["ms"])
        ndm, tout = s.ndm, T - s.max_delay
    med = {m: float(np.median(v)) for m, v in wall.items()}
    st = {m: {k: round(float(np.median([d[k] for d in v])), 4) for k in v[0]} for m, v in stages.items()}
    res = dict(what="search gulp with and without RFI cleaning", gpu=torch.cuda.get_device_name(0), nchan=nchan,
               nsamp=T, tout=tout, ndm=ndm, boxcar_max=search.HEIMDALL_BOXCAR_MAX, zap=search.HEIMDALL_ZAP,
               baseline_samples=int(2.0 / search.TSAMP), reps=a.reps,
               ms_per_gulp_off=round(med["off"], 3), ms_per_gulp_on=round(med["on"], 3),
               rfi_device_ms=round(float(np.median(rfi_ms)), 4), rfi_device_ms_min=round(float(np.min(rfi_ms)), 4),
               rfi_device_ms_max=round(float(np.max(rfi_ms)), 4),
               rfi_share_of_gulp=round(float(np.median(rfi_ms)) / med["off"], 4),
               wall_increase=round(med["on"] / med["off"] - 1.0, 4),
               last_flags=dict(n_narrow=info["n_narrow"], n_broad_samples=info["n_broad_samples"]),
               stage_ms_off=st["off"], stage_ms_on=st["on"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
