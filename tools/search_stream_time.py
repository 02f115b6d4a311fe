"""What gathering the gulp on the device saves the search at heimdall's production flags (tools/search_rfi_time.py's gulp:
30 720 new samples of 4096 channels, the tolerance-spaced trial DMs 2-1000, boxcars up to 64, the edge zaps, a 2-s running
baseline; every gulp but the first is searched with the max_delay + 63 samples before it).  In one process on one card:
  * today's path: GulpSearch.push of a whole gulp of 8-bit samples from page-locked memory -- wall ms per gulp, and the
    device ms of its stages (H2D, transpose, dedisperse, statistics, boxcar, D2H);
  * the fed path, the same samples in 24 pieces of 1280 from device memory (8 bits, and the production's 2 bits): wall and
    device ms per push, wall and device ms of the advance, and wall ms from the last push's return to the candidates
    (pb_search_gulp_peaks and the host's grouping) with the device ms of its stages;
  * the same with host pieces (page-locked);
  * the block path with the stage never switched on, through the C ABI directly, for this tree's library and -- with
    --parent PATH -- for another libpb_hip.so (the parent commit's, built in a separate worktree), in alternating rounds:
    both launch the same kernels, and this tree's median is expected inside the parent's minimum .. maximum.
The candidates of the three paths are compared; candidates_equal must be true.  Prints one JSON line.

    python tools/search_stream_time.py [--gulps 4] [--parent /path/to/parent/libpb_hip.so] [--out profiles/search_stream_time.json]"""
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
import search_cutout_time as CT  # noqa: E402  (the gulp through a library bound by hand; spread)
import search_giants_time as GT  # noqa: E402  (the gulp's samples: noise and three planted pulses)

search = importlib.import_module("vlite-fast_amd.search")
libpb = importlib.import_module("vlite-fast_amd.libpb")

PIECE = 1280
THRESH = 6.0


def pack(x, nbit):
    """u8 [nsamp][nchan] -> SIGPROC codes, low bits first (values taken modulo 2^nbit)"""
    v = np.asarray(x, np.uint8).ravel() & np.uint8((1 << nbit) - 1)
    if nbit == 8:
        return v
    per = 8 // nbit
    v = v.reshape(-1, per)
    out = np.zeros(v.shape[0], np.uint8)
    for i in range(per):
        out |= v[:, i] << np.uint8(nbit * i)
    return out


def make_searcher(maxs, dml):
    s = search.Searcher(max_samples=maxs, dm_list=dml)
    s.set_baseline(int(2.0 / search.TSAMP))
    return s


def lines(cands):
    return [search.candidate_line(c) for c in cands]


def whole_gulps(codes, ngulp, maxs, dml):
    """today's path: the same gulp pushed ngulp times from page-locked memory; the first (no tail yet) is left out"""
    wall, dev, out = [], [], []
    with make_searcher(maxs, dml) as s:
        g = search.GulpSearch(s, threshold=THRESH)
        for k in range(ngulp + 1):
            t0 = time.perf_counter()
            c = g.push(codes)
            t1 = time.perf_counter()
            out += lines(c)
            if k >= 1:
                wall.append((t1 - t0) * 1e3)
                dev.append(s.timers())
        out += lines(g.finish())
    stages = {k: CT.spread([d[k] for d in dev]) for k in dev[0]}
    return dict(wall_ms_per_gulp=CT.spread(wall), device_ms_stages=stages,
                device_ms_per_gulp=CT.spread([sum(d.values()) for d in dev])), out


def fed_gulps(piece_args, nbit, ngulp, maxs, dml, T):
    """the fed path by hand, step by step as GulpSearch.feed does it (no cutouts, no refinement): piece_args(i) gives
    Searcher.push's arguments for piece i of the gulp"""
    push_wall, push_dev, copy_dev, adv_wall, adv_dev, tail_wall, tail_dev, out = [], [], [], [], [], [], [], []
    with make_searcher(maxs, dml) as s:
        ov = (1 << (s.nbox - 1)) - 1
        s.set_gulp(s.max_delay + ov)
        done = 0
        for k in range(ngulp + 1):
            for i in range(T // PIECE):
                t0 = time.perf_counter()
                fill = s.push(nbit=nbit, **piece_args(i))
                t1 = time.perf_counter()
                if k >= 1:
                    tm = s.gulp_timers()
                    push_wall.append((t1 - t0) * 1e3)
                    push_dev.append(tm["append"])
                    copy_dev.append(tm["copy"])
            t1 = time.perf_counter()
            pk = s.gulp_peaks(THRESH)
            nout = pk["tout"] - ov
            full = pk["t"] < nout
            c = search.candidates_from_peaks(search.GulpSearch._subset(pk, full), s.dms, s.tsamp, sample0=done)
            t2 = time.perf_counter()
            pending = (search.GulpSearch._subset(pk, ~full), done)
            done += nout
            dv = s.timers()
            s.gulp_advance(min(s.max_delay + ov, fill))
            t3 = time.perf_counter()
            out += lines(c)
            if k >= 1:
                tail_wall.append((t2 - t1) * 1e3)
                tail_dev.append(sum(dv.values()))
                adv_wall.append((t3 - t2) * 1e3)
                adv_dev.append(s.gulp_timers()["advance"])
        out += lines(search.candidates_from_peaks(pending[0], s.dms, s.tsamp, sample0=pending[1]))
    return dict(nbit=nbit, pieces_per_gulp=T // PIECE, wall_ms_per_push=CT.spread(push_wall),
                device_ms_copy_per_push=CT.spread(copy_dev), device_ms_append_per_push=CT.spread(push_dev),
                wall_ms_last_push_to_candidates=CT.spread(tail_wall), device_ms_search=CT.spread(tail_dev),
                wall_ms_advance=CT.spread(adv_wall), device_ms_advance=CT.spread(adv_dev),
                wall_ms_per_gulp_all_pushes=round(float(np.sum(push_wall)) / ngulp, 4)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gulps", type=int, default=4, help="gulps timed per path (one more is run first and left out)")
    ap.add_argument("--reps", type=int, default=8, help="never-switched-on gulps per library")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent", default=None, help="the parent commit's libpb_hip.so")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    T, nchan = search.HEIMDALL_GULP, 4096
    pinned = torch.empty((T, nchan), dtype=torch.uint8, pin_memory=True)
    codes = pinned.numpy()
    codes[:] = GT.make_gulp(T, nchan)
    dml = search.dedisp_dm_list(2.0, 1000.0, search.TSAMP, search.FCH1, search.FOFF, nchan)
    maxs = T + int(4.148808e3 * 1000.0 * abs((search.FCH1 + (nchan - 1) * search.FOFF) ** -2 - search.FCH1 ** -2) / search.TSAMP) + 64
    res = dict(what="search gulp gathered on the device from pieces", gpu=torch.cuda.get_device_name(0), nchan=nchan,
               new_samples_per_gulp=T, piece=PIECE, ndm=int(dml.size), boxcar_max=search.HEIMDALL_BOXCAR_MAX,
               zap=search.HEIMDALL_ZAP, baseline_samples=int(2.0 / search.TSAMP), max_samples=maxs, gulps=a.gulps, threshold=THRESH)
    res["whole_gulp_from_pinned_host"], ref = whole_gulps(codes, a.gulps, maxs, dml)
    dev = torch.from_numpy(codes).cuda()
    torch.cuda.synchronize()
    res["fed_from_device"], got_dev = fed_gulps(lambda i: dict(device_ptr=dev.data_ptr() + i * PIECE * nchan, nsamp=PIECE), 8,
                                                a.gulps, maxs, dml, T)
    res["fed_from_pinned_host"], got_host = fed_gulps(lambda i: dict(codes=codes[i * PIECE:(i + 1) * PIECE]), 8, a.gulps, maxs, dml, T)
    res["candidates"] = len(ref)
    res["candidates_equal"] = bool(got_dev == ref and got_host == ref)
    # the production's 2 bits (other samples: the low two bits of the same codes; timing only)
    dev2 = torch.from_numpy(pack(codes, 2)).cuda()
    torch.cuda.synchronize()
    res["fed_from_device_2bit"], _ = fed_gulps(lambda i: dict(device_ptr=dev2.data_ptr() + i * PIECE * nchan // 4, nsamp=PIECE), 2,
                                               a.gulps, maxs, dml, T)
    del dev, dev2
    per = max(1, a.reps // a.rounds)
    this, parent = [], []
    for _ in range(a.rounds):
        this += CT.gulp_times_other(libpb.LIB_PATH, codes, dml, per)[0]
        if a.parent:
            parent += CT.gulp_times_other(a.parent, codes, dml, per)[0]
    res["block_path_never_on"] = dict(reps=per * a.rounds, rounds=a.rounds, ms_per_gulp=CT.spread(this))
    if a.parent:
        res["block_path_never_on"]["parent_library_ms_per_gulp"] = CT.spread(parent)
        res["block_path_never_on"]["median_minus_parent_median_ms"] = round(float(np.median(this) - np.median(parent)), 4)
        res["block_path_never_on"]["within_parent_spread"] = bool(min(parent) <= np.median(this) <= max(parent))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
