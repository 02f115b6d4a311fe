"""What finding giants and clustering them on the device costs the search at heimdall's production flags
(tools/search_rfi_time.py's gulp: 30 720 samples of 4096 channels, the tolerance-spaced trial DMs 2-1000, boxcars up to 64,
the edge zaps, a 2-s running baseline).  In one process on one card:
  * the gulp with the stage never switched on, through the C ABI directly, for this tree's library and -- with
    --parent PATH -- for another libpb_hip.so (the parent commit's, built in a separate worktree), in alternating rounds:
    median, minimum and maximum wall ms of each; never switched on both launch the same kernels, and this tree's median
    is expected inside the parent's minimum .. maximum (recorded as never_on_within_parent_spread);
  * on noise with a few planted pulses, at threshold 6 and at a threshold low enough that the point list passes 2^20:
    the giants, the clusters, the device time of the giant pass and of the labelling and merge, the sweeps, the wall time
    of Searcher.giants + candidates_from_giants, and beside it the wall time of the host path on the same gulp,
    Searcher.peaks + candidates_from_peaks, given up and reported as "> 60 s" when it runs longer (it runs in a child
    process that is ended).
Prints one JSON line.

    python tools/search_giants_time.py [--reps 10] [--parent /path/to/parent/libpb_hip.so] [--out profiles/search_giants_time.json]"""
import argparse
import importlib
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import search_cutout_time as CT  # noqa: E402  (the gulp through a library bound by hand)

search = importlib.import_module("vlite-fast_amd.search")
libpb = importlib.import_module("vlite-fast_amd.libpb")

HOST_LIMIT_S = 60.0


def make_gulp(T, nchan):
    rng = np.random.default_rng(3)
    codes = np.empty((T, nchan), np.uint8)
    for i in range(0, T, 3072):
        codes[i:i + 3072] = np.clip(rng.normal(127.5, 1 / 0.02957, (min(3072, T - i), nchan)), 0, 255).astype(np.uint8)
    tsamp, fch1, foff = search.TSAMP, search.FCH1, search.FOFF
    f = fch1 + foff * np.arange(nchan)
    for dm, t0, amp in ((60.0, 3000, 14), (300.0, 9000, 12), (500.0, 15000, 12)):
        d = np.floor(4.148808e3 * dm * (f ** -2 - f[0] ** -2) / tsamp + 0.5).astype(int)
        for w in range(4):
            codes[t0 + w + d, np.arange(nchan)] = np.clip(codes[t0 + w + d, np.arange(nchan)].astype(int) + amp, 0, 255)
    return codes


def host_path(q, codes, dml, thresh):
    """child process: the point list and the host's grouping, timed"""
    with search.Searcher(max_samples=codes.shape[0], dm_list=dml) as s:
        s.set_baseline(int(2.0 / search.TSAMP))
        s.peaks(codes, 1e30)                                            # (first call: the context, the allocations)
        t0 = time.perf_counter()
        pk = s.peaks(codes, thresh, max_out=1 << 20)
        t1 = time.perf_counter()
        q.put(dict(points=int(pk["total"]), peaks_wall_ms=round((t1 - t0) * 1e3, 3)))
        c = search.candidates_from_peaks(pk, s.dms, s.tsamp)
        q.put(dict(candidates=len(c), grouping_wall_ms=round((time.perf_counter() - t1) * 1e3, 3)))


def host_time(codes, dml, thresh):
    ctx = mp.get_context("spawn")                                       # a fresh process: nothing of this one's GPU state
    q = ctx.Queue()
    p = ctx.Process(target=host_path, args=(q, codes, dml, thresh))
    p.start()
    out, t0 = {}, time.perf_counter()
    while time.perf_counter() - t0 < HOST_LIMIT_S + 5 and len(out) < 4:
        try:
            out.update(q.get(timeout=1.0))
        except Exception:
            if not p.is_alive():
                break
    if "grouping_wall_ms" not in out:
        out["grouping_wall_ms"] = "> %d s" % HOST_LIMIT_S
    if p.is_alive():
        p.terminate()
    p.join()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent", default=None, help="the parent commit's libpb_hip.so")
    ap.add_argument("--low", type=float, default=3.0, help="the low threshold")
    ap.add_argument("--no-host", action="store_true", help="leave the host path out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    T, nchan = search.HEIMDALL_GULP, 4096
    pinned = torch.empty((T, nchan), dtype=torch.uint8, pin_memory=True)
    codes = pinned.numpy()
    codes[:] = make_gulp(T, nchan)
    dml = search.dedisp_dm_list(2.0, 1000.0, search.TSAMP, search.FCH1, search.FOFF, nchan)
    per = max(1, a.reps // a.rounds)
    this, parent = [], []
    for _ in range(a.rounds):
        t, ndm, tout = CT.gulp_times_other(libpb.LIB_PATH, codes, dml, per)
        this += t
        if a.parent:
            parent += CT.gulp_times_other(a.parent, codes, dml, per)[0]
    res = dict(what="search gulp; giants and clusters on the device", gpu=torch.cuda.get_device_name(0), nchan=nchan, nsamp=T,
               tout=tout, ndm=ndm, boxcar_max=search.HEIMDALL_BOXCAR_MAX, zap=search.HEIMDALL_ZAP,
               baseline_samples=int(2.0 / search.TSAMP), reps=per * a.rounds, rounds=a.rounds,
               ms_per_gulp_never_on=CT.spread(this))
    if a.parent:
        res["parent_library"] = dict(ms_per_gulp=CT.spread(parent))
        res["never_on_median_minus_parent_median_ms"] = round(float(np.median(this) - np.median(parent)), 4)
        res["never_on_within_parent_spread"] = bool(min(parent) <= np.median(this) <= max(parent))
    with search.Searcher(max_samples=T, dm_list=dml) as s:
        s.set_baseline(int(2.0 / search.TSAMP))
        pk = s.peaks(codes, 1e30, max_out=1)
        for name, thresh, cap in (("threshold_6", 6.0, 1 << 18), ("threshold_low", a.low, 1 << 22)):
            s.set_giants(max_giants=cap)
            gi, lab, cp, wall = [], [], [], []
            for rep in range(a.reps + 1):
                t1 = time.perf_counter()
                r = s.giants(thresh)
                c = search.candidates_from_giants(r, s.dms, s.tsamp)
                t2 = time.perf_counter()
                if rep >= 1:
                    tm = s.giant_timers()
                    gi.append(tm["giants"])
                    lab.append(tm["label"])
                    cp.append(tm["with_copy"])
                    wall.append((t2 - t1) * 1e3)
            res[name] = dict(thresh=thresh, max_giants=cap, giants=r["ngiants"], overflow=r["overflow"], clusters=len(c),
                             points_in_giants=int(r["npoints"].sum()), sweeps=tm["sweeps"], device_ms_giant_pass=CT.spread(gi),
                             device_ms_label_and_merge=CT.spread(lab), device_ms_with_copy=CT.spread(cp),
                             wall_ms_giants_and_candidates=CT.spread(wall),
                             strongest=search.candidate_line(c[0]) if c else None)
    if not a.no_host:
        for name, thresh in (("threshold_6", 6.0), ("threshold_low", a.low)):
            res[name]["host_path"] = host_time(np.array(codes), dml, thresh)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
