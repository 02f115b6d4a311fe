"""What searching the fp32 plane in-process costs and buys (pb_search_push_f32, process_baseband --search).  In one
process on one card:
  * push: device ms of pb_search_push_f32 for 1280 x 4096 samples from device memory, beside pb_search_push of the same
    number of samples at 8 and at 2 bits (pb_search_gulp_timers' append);
  * block_path_never_on: the production gulp through the block path with the streaming stage never switched on, through
    the C ABI directly, for this tree's library and -- with --parent PATH -- for another libpb_hip.so (the parent
    commit's, built in a separate worktree), in alternating rounds of one run each, as tools/search_stream_time.py does;
  * step: wall ms of pb_process of one full-size second (10 segments of 1024 rows, 2 bits) with keep_ave off and on;
  * replay: a dump of --seconds full-size seconds (the same noise every second) through process_baseband.py -b 2 without
    --search, with --search-input codes and with --search-input plane: wall seconds of run() (a first run, then
    three), seconds of data per wall second, and how many candidate lines the run printed.  The search flags are
    SEARCH_FLAGS below (a short gulp and DM range, so that a dump of a few seconds fires gulps at all; not the
    production flags, whose gulp alone is 24 s of data);
  * snr: the reference's self-test pulse (DM 14, 2 ms, x1.05, 512 samples, the noise of tests/test_gpu_chain.py) at trial
    DM 14: best S/N from the plane of a 2-bit handle, from an 8-bit handle's codes and from the 2-bit codes;
  * nan_segment: an all-zero first segment (every frame dropped) through an 8-bit handle with keep_ave: NaNs in its plane, and
    whether the plane pushed through pb_search_push_f32 gives the block of the handle's own codes.
Prints one JSON line.

    python tools/search_plane_time.py [--parent /path/to/parent/libpb_hip.so] [--out profiles/search_plane_time.json]"""
import argparse
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import search_cutout_time as CT  # noqa: E402  (the gulp through a library bound by hand; spread)
import search_giants_time as GT  # noqa: E402  (the gulp's samples: noise and three planted pulses)

search = importlib.import_module("vlite-fast_amd.search")
libpb = importlib.import_module("vlite-fast_amd.libpb")
vdif = importlib.import_module("vlite-fast_amd.vdif")
pbmod = importlib.import_module("vlite-fast_amd.process_baseband")

PIECE, NCHAN = 1280, 4096
SEARCH_FLAGS = "-dm 2 100 -boxcar_max 64 -nsamps_gulp 2560 -zap_chans 0 190 -zap_chans 3900 4096 -detect_thresh 6"
R, SEG, NFFT = 1024, 10, 12500


def push_times(reps):
    import torch
    rng = np.random.default_rng(1)
    plane = torch.from_numpy(rng.normal(0, 1, (PIECE, NCHAN)).astype(np.float32)).cuda()
    codes8 = torch.from_numpy(rng.integers(0, 256, PIECE * NCHAN, dtype=np.uint8)).cuda()
    codes2 = torch.from_numpy(rng.integers(0, 256, PIECE * NCHAN // 4, dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    out = {}
    with search.Searcher(nchan=NCHAN, max_samples=2 * PIECE, dm_min=0, dm_max=10, dm_step=2, boxcar_max=4) as s:
        s.set_gulp(16)
        for name, call in (("plane_f32", lambda: s.push_plane(device_ptr=plane.data_ptr(), nsamp=PIECE)),
                           ("codes_8bit", lambda: s.push(nbit=8, device_ptr=codes8.data_ptr(), nsamp=PIECE)),
                           ("codes_2bit", lambda: s.push(nbit=2, device_ptr=codes2.data_ptr(), nsamp=PIECE))):
            ms = []
            for rep in range(reps + 3):
                call()
                if rep >= 3:
                    ms.append(s.gulp_timers()["append"])
                s.gulp_advance(0)
            out[name] = CT.spread(ms)
    return dict(samples=PIECE, nchan=NCHAN, reps=reps, device_ms_append=out)


def never_on(parent, rounds):
    T = search.HEIMDALL_GULP
    codes = GT.make_gulp(T, NCHAN)
    dml = search.dedisp_dm_list(2.0, 1000.0, search.TSAMP, search.FCH1, search.FOFF, NCHAN)
    this, par = [], []
    for _ in range(rounds):
        this += CT.gulp_times_other(libpb.LIB_PATH, codes, dml, 1)[0]
        if parent:
            par += CT.gulp_times_other(parent, codes, dml, 1)[0]
    res = dict(rounds=rounds, runs_per_round=1, ms_per_gulp=CT.spread(this))
    if parent:
        res["parent_library_ms_per_gulp"] = CT.spread(par)
        res["median_minus_parent_median_ms"] = round(float(np.median(this) - np.median(par)), 4)
        res["within_parent_spread"] = bool(min(par) <= np.median(this) <= max(par))
    return res


def one_second(seed):
    """u8 [2][10 x 1024 x 12500]: one full-size second of genbase-style noise"""
    rng = np.random.default_rng(seed)
    return np.clip(rng.standard_normal((2, SEG * R * NFFT), dtype=np.float32) * np.float32(16.9) + np.float32(128.5),
                   0, 255).astype(np.uint8)


def step_times(sec, reps):
    out = {}
    for keep in (False, True):
        with libpb.PbHandle(nbit=2, rfi_mode=2, rows_per_seg=R, max_seg=SEG, keep_ave=keep) as h:
            n = R * NFFT
            for sg in range(SEG):
                h.submit_planar(0, sg, sec[0, sg * n:(sg + 1) * n], sec[1, sg * n:(sg + 1) * n])
            ms = []
            for rep in range(reps + 2):
                h.sync()
                t0 = time.perf_counter()
                h.process(SEG)
                h.sync()
                if rep >= 2:
                    ms.append((time.perf_counter() - t0) * 1e3)
            out["keep_ave_on" if keep else "keep_ave_off"] = CT.spread(ms)
    return dict(reps=reps, wall_ms_per_second_of_data=out)


def replay(sec, seconds, tmp):
    dump = os.path.join(tmp, "obs.uw")
    with open(dump, "wb") as f:
        f.write(vdif.ascii_header_format(vdif.writer_header(7, 0.8718, -0.72452, "B0833-45", 58000.0, "19A-331", 33, 3600)))
        for k in range(seconds):
            f.write(vdif.frame_block(sec[0], sec[1], 3600 + k, 33, 7).tobytes())
    out = dict(seconds_in_dump=seconds, seconds_kept=seconds - 1, search_flags=SEARCH_FLAGS)
    for name, more in (("no_search", []), ("search_codes", ["--search", SEARCH_FLAGS, "--search-input", "codes"]),
                       ("search_plane", ["--search", SEARCH_FLAGS, "--search-input", "plane"])):
        d = os.path.join(tmp, name)
        os.makedirs(d)
        argv = ["-w", "0", "-r", "2", "-b", "2", "--no-control", "--replay", dump, "--datadir", d, "--logdir", os.path.join(d, "logs")] + more
        walls, ncand = [], 0
        for rep in range(4):                        # the first run pays the page cache and the runtime's start-up
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                t0 = time.perf_counter()
                rc = pbmod.run(pbmod.build_parser().parse_args(argv))
                walls.append(time.perf_counter() - t0)
            assert rc == 0
            ncand = sum(1 for l in buf.getvalue().splitlines() if l.count("\t") == 8)
        out[name] = dict(wall_s_first_run=round(walls[0], 4), wall_s=CT.spread(walls[1:]), candidate_lines=ncand,
                         seconds_of_data_per_wall_second=round((seconds - 1) / float(np.median(walls[1:])), 2))
    return out


def pulse_snr():
    rng = np.random.default_rng(20261018)
    R2, S2, T2 = 1024, 4, 512
    data = np.empty((S2, 2, R2 * NFFT), np.uint8)
    for sg in range(S2):
        data[sg] = np.clip(rng.standard_normal((2, R2 * NFFT), dtype=np.float32) * np.float32(16.9) + np.float32(128.5),
                           0, 255).astype(np.uint8)
    best = {}
    with search.Searcher(nchan=NCHAN, max_samples=T2, boxcar_max=16, zap=search.HEIMDALL_ZAP, dm_min=0, dm_max=28, dm_step=2) as s:
        s.set_gulp(1)
        for nbit in (2, 8):
            with libpb.PbHandle(nbit=nbit, rfi_mode=1, rows_per_seg=R2, max_seg=S2, inject_frb=True, keep_ave=nbit == 2) as h:
                h.set_frb_params(dm=14.0, width_rows=-1, amp=1.05)
                for sg in range(S2):
                    h.submit_planar(0, sg, data[sg, 0], data[sg, 1])
                h.process(S2, inject_now=1)
                h.sync()
                codes, ave = h.output_dev(0, 1)
                s.push(nbit=nbit, device_ptr=codes, nsamp=T2)
                best["codes_%dbit" % nbit] = float(s.gulp_run()["snr"][7].max())
                s.gulp_advance(0)
                if nbit == 2:
                    s.push_plane(device_ptr=ave, nsamp=T2)
                    best["plane_of_2bit_handle"] = float(s.gulp_run()["snr"][7].max())
                    s.gulp_advance(0)
    best["plane_over_2bit_codes"] = round(best["plane_of_2bit_handle"] / best["codes_2bit"], 4)
    return dict(trial_dm=14.0, best_snr=best)


def nan_segment():
    rows, nseg = 64, 4
    T = rows * nseg // 8
    rng = np.random.default_rng(3)
    data = np.clip(rng.standard_normal((nseg, 2, rows * NFFT), dtype=np.float32) * np.float32(16.9) + np.float32(128.5),
                   0, 255).astype(np.uint8)
    data[0] = 0                                     # every frame of the first segment dropped (tools/nan_codes_check.py)
    with libpb.PbHandle(nbit=8, rfi_mode=2, rows_per_seg=rows, max_seg=nseg, keep_ave=True) as h:
        for sg in range(nseg):
            h.submit_planar(0, sg, data[sg, 0], data[sg, 1])
        h.process(nseg)
        h.sync()
        out = h.fetch(0, 0, nseg, ave=True)
        codes, ave = h.output_dev(0, 1)
        with search.Searcher(nchan=NCHAN, max_samples=64, dm_min=0, dm_max=2, dm_step=2, boxcar_max=1) as s:
            s.set_gulp(1)
            s.push_plane(device_ptr=ave, nsamp=T)
            from_plane = s.gulp_fetch()
            s.gulp_advance(0)
            s.push(nbit=8, device_ptr=codes, nsamp=T)
            from_codes = s.gulp_fetch()
    plane = out["ave_kur"].reshape(T, NCHAN)
    nan = np.isnan(plane)
    return dict(samples=T, nan_values_in_plane=int(nan.sum()), nan_time_samples=int(nan.any(axis=1).sum()),
                codes_of_nan_values=sorted(set(out["kur"].reshape(T, NCHAN)[nan].tolist())),
                plane_block_equals_8bit_codes_block=bool(np.array_equal(from_plane, from_codes)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--seconds", type=int, default=9, help="seconds in the replayed dump (the last one is dropped)")
    ap.add_argument("--parent", default=None, help="the parent commit's libpb_hip.so")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    res = dict(what="the search fed the fp32 plane at 8-bit depth", gpu=torch.cuda.get_device_name(0))
    res["push"] = push_times(a.reps)
    res["snr"] = pulse_snr()
    res["nan_segment"] = nan_segment()
    res["block_path_never_on"] = never_on(a.parent, a.rounds)
    sec = one_second(7)
    res["step"] = step_times(sec, a.reps)
    with tempfile.TemporaryDirectory() as tmp:
        res["replay"] = replay(sec, a.seconds, tmp)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
