"""What per-candidate cutouts cost the search at heimdall's production flags: one 30 720-sample gulp of 4096 channels,
the tolerance-spaced trial DMs 2-1000, boxcars up to 64, the edge zaps, a 2-s running baseline, the peak list at S/N 6
from page-locked host memory (tools/search_rfi_time.py's gulp).  In one process on one card: the gulp with cutouts never
switched on (median, minimum and maximum wall ms over the repetitions; through the C ABI directly, and through
Searcher.peaks never switched on and switched on), then on a Searcher with cutouts on the device time of
pb_search_cutouts (its kernels alone, and with the copy to the host) and its wall time for 32 requests at tscr 1 and at
tscr 32, spread over the DM and time range of the block.  Prints one JSON line.

With PB_LIBPATH pointing at another libpb_hip.so -- e.g. the parent commit's, built in a separate worktree -- only the
gulp is timed (that library may have no cutouts); --merge FILE adds those figures to the record of an earlier run under
"other_library", so that one file holds both: with cutouts never switched on both libraries launch the same kernels,
and the two gulp times are expected to agree within the spread the tool reports.

    python tools/search_cutout_time.py [--reps 20] [--out profiles/search_cutout_time.json]
    PB_LIBPATH=/path/to/parent/libpb_hip.so python tools/search_cutout_time.py --gulp-only --merge profiles/search_cutout_time.json"""
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


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))


def gulp_times_other(path, codes, dml, reps):
    """the never-switched-on gulp through another libpb_hip.so, bound here by hand: the package's loader insists on every
    function of THIS tree's ABI, which an older library does not have"""
    import ctypes as C
    L = C.CDLL(path)
    vp, fp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.pb_search_create_list.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, fp, C.c_int, C.c_int, ip,
                                        C.c_int, C.POINTER(vp)]
    L.pb_search_set_baseline.argtypes = [vp, C.c_int]
    L.pb_search_peaks.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int32), C.c_int, ip, ip]
    L.pb_search_info.argtypes = [vp, ip, ip, ip]
    L.pb_search_destroy.argtypes = [vp]
    L.pb_search_destroy.restype = None
    T, nchan = codes.shape
    zap = [v for pair in search.HEIMDALL_ZAP for v in pair]
    s = vp()
    dl = np.ascontiguousarray(dml, np.float32)
    rc = L.pb_search_create_list(0, nchan, T, search.FCH1, search.FOFF, search.TSAMP, dl.ctypes.data_as(fp), dl.size,
                                 search.HEIMDALL_BOXCAR_MAX, (C.c_int * len(zap))(*zap), len(zap) // 2, C.byref(s))
    assert rc == 0, rc
    L.pb_search_set_baseline(s, int(2.0 / search.TSAMP))
    md = C.c_int()
    L.pb_search_info(s, None, None, C.byref(md))
    buf = np.empty((1 << 18, 4), np.int32)
    n, t, out = C.c_int(), C.c_int(), []
    for rep in range(reps + 2):
        t0 = time.perf_counter()
        rc = L.pb_search_peaks(s, codes.ctypes.data_as(vp), 0, T, 8, C.c_float(6.0), buf.ctypes.data_as(C.POINTER(C.c_int32)),
                               1 << 18, C.byref(n), C.byref(t))
        assert rc == 0, rc
        if rep >= 2:
            out.append((time.perf_counter() - t0) * 1e3)
    L.pb_search_destroy(s)
    return out, dl.size, T - md.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gulp-only", action="store_true", help="time the gulp alone (a library without cutouts)")
    ap.add_argument("--merge", default=None, help="add this run's gulp figures to that JSON file as other_library")
    ap.add_argument("--label", default="library of PB_LIBPATH", help="with --merge: what the other library is")
    a = ap.parse_args()
    T, nchan, ncut = search.HEIMDALL_GULP, 4096, 32
    rng = np.random.default_rng(3)
    pinned = torch.empty((T, nchan), dtype=torch.uint8, pin_memory=True)
    codes = pinned.numpy()
    codes[:] = np.clip(rng.normal(127.5, 1 / 0.02957, (T, nchan)), 0, 255).astype(np.uint8)
    dml = search.dedisp_dm_list(2.0, 1000.0, search.TSAMP, search.FCH1, search.FOFF, nchan)
    # cutouts never switched on
    gulp, ndm, tout = gulp_times_other(os.environ.get("PB_LIBPATH") or importlib.import_module("vlite-fast_amd.libpb").LIB_PATH,
                                       codes, dml, a.reps)
    res = dict(what="search gulp and per-candidate cutouts", gpu=torch.cuda.get_device_name(0), nchan=nchan, nsamp=T, tout=tout,
               ndm=ndm, boxcar_max=search.HEIMDALL_BOXCAR_MAX, zap=search.HEIMDALL_ZAP, baseline_samples=int(2.0 / search.TSAMP),
               reps=a.reps, library=a.label if os.environ.get("PB_LIBPATH") else "this tree's", ms_per_gulp_never_on=spread(gulp))
    if not a.gulp_only:
        # the same gulp through Searcher.peaks (which adds Python's share), for the comparison with the switched-on one
        with search.Searcher(max_samples=T, dm_list=dml) as s:
            s.set_baseline(int(2.0 / search.TSAMP))
            off = []
            for rep in range(a.reps + 2):
                t0 = time.perf_counter()
                s.peaks(codes, 6.0)
                if rep >= 2:
                    off.append((time.perf_counter() - t0) * 1e3)
        res["ms_per_gulp_searcher_never_on"] = spread(off)
        with search.Searcher(max_samples=T, dm_list=dml) as s:
            s.set_baseline(int(2.0 / search.TSAMP))
            s.set_cutouts(max_cands=ncut)
            nsub, nt, nrow, _ = s._cut
            nact = nchan - sum(hi - lo for lo, hi in search.HEIMDALL_ZAP)
            dmi = np.linspace(40, ndm - 40, ncut).astype(int)
            tpk = np.linspace(9000, tout - 9000, ncut).astype(int)
            on = []
            for tscr in (1, 32):
                dev, cp, wall = [], [], []
                for rep in range(a.reps + 2):
                    t0 = time.perf_counter()
                    s.peaks(codes, 6.0)
                    t1 = time.perf_counter()
                    s.cutouts(dmi, tpk, tscr)
                    t2 = time.perf_counter()
                    if rep >= 2:
                        tm = s.cutout_timers()
                        dev.append(tm["kernels"])
                        cp.append(tm["with_copy"])
                        wall.append((t2 - t1) * 1e3)
                        if tscr == 1:
                            on.append((t1 - t0) * 1e3)
                byt = ncut * (nact * nt * tscr + nrow * nt * tscr * 4)
                res["cutouts_tscr%d" % tscr] = dict(requests=ncut, bytes_read=byt, device_ms_kernels=spread(dev),
                                                    device_ms_with_copy=spread(cp), wall_ms_call=spread(wall),
                                                    gb_per_s=round(byt / (float(np.median(dev)) * 1e-3) / 1e9, 1))
            res["geometry"] = dict(nsub=nsub, nt=nt, ndmrow=nrow)
            res["ms_per_gulp_searcher_switched_on"] = spread(on)
            res["cutouts_share_of_gulp_tscr1"] = round(res["cutouts_tscr1"]["device_ms_kernels"]["median"] / float(np.median(gulp)), 4)
            res["cutouts_share_of_gulp_tscr32"] = round(res["cutouts_tscr32"]["device_ms_kernels"]["median"] / float(np.median(gulp)), 4)
    if a.merge:
        with open(a.merge) as f:
            base = json.loads(f.read())
        base["other_library"] = dict(library=res["library"], reps=a.reps, ms_per_gulp_never_on=res["ms_per_gulp_never_on"])
        d = base["other_library"]["ms_per_gulp_never_on"]["median"] - base["ms_per_gulp_never_on"]["median"]
        base["other_library"]["median_minus_this_ms"] = round(d, 4)
        res = base
        a.out = a.out or a.merge
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
