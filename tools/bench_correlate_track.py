"""Time of the fringe-stopping correlator (pb_correlate_tracked) beside pb_correlate of the same build, in one process on
one card: tools/bench_correlate.py's shape -- one second of data, R = 1024 x 10 segments, raw stream, 1024-row gates, 2
and 4 antennas --, device times from the two calls' timers, warm-up, then REPEATS calls, median and min / max.  The
model has every column non-zero (the kernel's work does not depend on its values).  One JSON line on stdout (and in the
file given as the first argument): both kernel times, their ratio, the bytes read and the implied TB/s.

    python tools/bench_correlate_track.py profiles/correlate_track_steptime.json"""
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

lp = importlib.import_module("vlite-fast_amd.libpb")
R, S, INT_ROWS, WARMUP, REPEATS = 1024, 10, 1024, 3, 15
NCO = 4096


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def time_both(nant):
    dev = torch.device("cuda", 0)
    model = np.random.default_rng(nant).uniform(-1, 1, (nant, 4)) * np.array([200.0, 1e-4, 1.0, 3e-4])
    with lp.PbHandle(device=0, nant=nant, nbit=8, npol=2, rfi_mode=0, rows_per_seg=R, max_seg=S, coherence=True) as h:
        n = h.seg_samples
        for a in range(nant):
            sec = bench.synth_second(torch, dev, 42 + a, n, S)
            torch.cuda.synchronize()
            for s in range(S):
                h.submit_planar_dev(a, s, sec[s][0].data_ptr(), sec[s][1].data_ptr(), n)
            h.sync()
        h.process(S)
        h.sync()
        plain, tracked, upload, copy = [], [], [], []
        for k in range(WARMUP + REPEATS):                      # the two calls alternate: the same card state for both
            vis, used = h.correlate(lp.CORR_RAW, S, INT_ROWS)
            p = h.correlate_timers()
            tvis, tused = h.correlate_tracked(lp.CORR_RAW, S, model, row_base=k * S * R, nrows=INT_ROWS)
            t = h.correlate_tracked_timers()
            if k >= WARMUP:
                plain.append(p[0])
                upload.append(t[0])
                tracked.append(t[1])
                copy.append(t[2])
        assert tvis.shape == vis.shape == (S * R // INT_ROWS, nant * (nant + 1) // 2, 4, NCO)
        assert int(used.min()) == INT_ROWS and int(tused.min()) == INT_ROWS
    return plain, tracked, upload, copy


def main():
    res = {"config": "R=1024 x 10 segments (1 s), raw stream, 1024-row gates, 8 bit; device ms per call: median, min, max "
                     "of %d calls after %d warm-up calls, pb_correlate and pb_correlate_tracked alternating" % (REPEATS, WARMUP),
           "cases": {}}
    for nant in (2, 4):
        plain, tracked, upload, copy = time_both(nant)
        nbytes = nant * 2 * S * R * NCO * 8
        p, t = stats(plain), stats(tracked)
        res["cases"]["A=%d" % nant] = {
            "pb_correlate_kernel_ms": p, "pb_correlate_tracked_kernel_ms": t,
            "pb_correlate_tracked_upload_ms": stats(upload), "pb_correlate_tracked_copy_out_ms": stats(copy),
            "tracked_over_plain": t["median"] / p["median"], "bytes_read": nbytes,
            "plain_TB_per_s": nbytes / (p["median"] * 1e-3) / 1e12, "tracked_TB_per_s": nbytes / (t["median"] * 1e-3) / 1e12}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
