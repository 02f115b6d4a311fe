"""Time of the correlator's X step (pb_correlate, int_rows = 1024) on one second of data -- R = 1024 x 10 segments -- of
2 and of 4 antennas, raw stream, beside the same arithmetic in plain torch on complex64 tensors of the same shape on
the same card: the baseline a user would otherwise write.  Device times: pb_correlate_timers for the library, events
for torch; warm-up, then REPEATS calls, median and min / max.  One JSON line on stdout (and in the file given as the
first argument): both figures, the bytes the kernel reads and the implied TB/s.

    python tools/bench_correlate.py profiles/correlate_steptime.json"""
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

lp = importlib.import_module("vlite-fast_amd.libpb")
R, S, INT_ROWS, WARMUP, REPEATS = 1024, 10, 1024, 3, 15
NCO = 4096


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def time_library(nant):
    dev = torch.device("cuda", 0)
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
        kern, copy = [], []
        for k in range(WARMUP + REPEATS):
            vis, used = h.correlate(lp.CORR_RAW, S, INT_ROWS)
            if k >= WARMUP:
                ms = h.correlate_timers()
                kern.append(ms[0])
                copy.append(ms[1])
        assert vis.shape == (S * R // INT_ROWS, nant * (nant + 1) // 2, 4, NCO) and int(used.min()) == INT_ROWS
    return kern, copy


def torch_loop(X, ngate):
    """per baseline i <= j: the four pol products, summed over each gate's rows"""
    A = X.shape[0]
    out = []
    for i in range(A):
        xi = X[i].view(2, 1, ngate, INT_ROWS, NCO)
        for j in range(i, A):
            xj = X[j].view(1, 2, ngate, INT_ROWS, NCO)
            out.append((xi * xj.conj()).sum(dim=3))            # [2][2][ngate][4096]
    return torch.stack(out)


def torch_einsum(X, ngate):
    Xg = X.view(X.shape[0], 2, ngate, INT_ROWS, NCO)
    return torch.einsum("apgtc,bqgtc->gabpqc", Xg, Xg.conj())  # every ordered pair, the lower triangle included


def time_torch(nant, fn):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    X = torch.view_as_complex(torch.randn(nant, 2, S * R, NCO, 2, device=dev, generator=g))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for k in range(WARMUP + REPEATS):
        a.record()
        out = fn(X, S * R // INT_ROWS)
        b.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            ms.append(a.elapsed_time(b))
        del out
    return ms


def main():
    res = {"config": "R=1024 x 10 segments (1 s), raw stream, int_rows 1024, 8 bit; device ms per call: "
                     "median, min, max of %d calls after %d warm-up calls" % (REPEATS, WARMUP), "cases": {}}
    for nant in (2, 4):
        kern, copy = time_library(nant)
        torch.cuda.empty_cache()
        loop = time_torch(nant, torch_loop)
        torch.cuda.empty_cache()
        ein = time_torch(nant, torch_einsum)
        torch.cuda.empty_cache()
        nbytes = nant * 2 * S * R * NCO * 8
        k = stats(kern)
        res["cases"]["A=%d" % nant] = {
            "pb_correlate_kernel_ms": k, "pb_correlate_copy_out_ms": stats(copy),
            "torch_loop_ms": stats(loop), "torch_einsum_ms": stats(ein),
            "bytes_read": nbytes, "kernel_TB_per_s": nbytes / (k["median"] * 1e-3) / 1e12,
            "torch_best_over_kernel": min(stats(loop)["median"], stats(ein)["median"]) / k["median"]}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
