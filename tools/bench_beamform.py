"""Time of the beamformer (pb_beamform, tscr = 8) on one second of data -- R = 1024 x 10 segments, raw stream -- of 4
antennas with 4 beams and of 8 antennas with 4 and 16 beams, beside the same arithmetic in plain torch on complex64
tensors of the same shape on the same card: the baseline a user would otherwise write.  Device times:
pb_beamform_timers for the library, events for torch; warm-up, then REPEATS calls, median and min / max.  One JSON line
on stdout (and in the file given as the first argument): both figures, the bytes of spectra the kernel reads per call
(every beam tile of four reads them once) and the implied TB/s.

    python tools/bench_beamform.py profiles/beamform_steptime.json"""
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
R, S, TSCR, WARMUP, REPEATS = 1024, 10, 8, 3, 15
NCO, CHANMIN, TILE = 4096, 2155, 4
CASES = ((4, 4), (8, 4), (8, 16))


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def time_library(nant, cases):
    """{nbeam: (weights ms, kernel ms, copy ms)} for one handle of nant antennas"""
    dev = torch.device("cuda", 0)
    out = {}
    with lp.PbHandle(device=0, nant=nant, nbit=8, npol=2, rfi_mode=0, rows_per_seg=R, max_seg=S, coherence=True) as h:
        n = h.seg_samples
        for a in range(nant):
            sec = bench.synth_second(torch, dev, 42 + a, n, S)
            torch.cuda.synchronize()
            for s in range(S):
                h.submit_planar_dev(a, s, sec[s][0].data_ptr(), sec[s][1].data_ptr(), n)
            h.sync()
            del sec
        torch.cuda.empty_cache()
        h.process(S)
        h.sync()
        for nbeam in cases:
            delay = np.random.default_rng(nbeam).uniform(-200.0, 200.0, (nbeam, nant))
            ms = [[], [], []]
            for k in range(WARMUP + REPEATS):
                beams, used = h.beamform(lp.CORR_RAW, S, delay, tscr=TSCR)
                if k >= WARMUP:
                    for i, v in enumerate(h.beamform_timers()):
                        ms[i].append(v)
            assert beams.shape == (nbeam, S * R // TSCR, 4, NCO) and int(used.min()) == TSCR
            out[nbeam] = ms
    return out


def torch_beams(X, W):
    """X complex64 [A][2][T][4096], W complex64 [nbeam][A][4096] -> float32 [nbeam][T / TSCR][4][4096]"""
    out = []
    for b in range(W.shape[0]):
        Y = (X * W[b][:, None, None, :]).sum(dim=0)                   # [2][T][4096]
        A, B = Y[0], Y[1]
        C = A * B.conj()
        P = torch.stack([A.real * A.real + A.imag * A.imag, B.real * B.real + B.imag * B.imag, C.real, C.imag], dim=1)
        out.append(P.view(-1, TSCR, 4, NCO).sum(dim=1))
    return torch.stack(out)


def time_torch(nant, nbeam):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    X = torch.view_as_complex(torch.randn(nant, 2, S * R, NCO, 2, device=dev, generator=g))
    W = torch.view_as_complex(torch.randn(nbeam, nant, NCO, 2, device=dev, generator=g))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for k in range(WARMUP + REPEATS):
        a.record()
        out = torch_beams(X, W)
        b.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            ms.append(a.elapsed_time(b))
        del out
    return ms


def main():
    res = {"config": "R=1024 x 10 segments (1 s), raw stream, tscr 8, 8 bit; device ms per call: "
                     "median, min, max of %d calls after %d warm-up calls" % (REPEATS, WARMUP), "cases": {}}
    for nant in sorted(set(c[0] for c in CASES)):
        lib = time_library(nant, [c[1] for c in CASES if c[0] == nant])
        torch.cuda.empty_cache()
        for nbeam, ms in lib.items():
            tor = time_torch(nant, nbeam)
            torch.cuda.empty_cache()
            once = nant * 2 * S * R * NCO * 8
            nbytes = once * ((nbeam + TILE - 1) // TILE)
            k = stats(ms[1])
            res["cases"]["A=%d beams=%d" % (nant, nbeam)] = {
                "pb_beamform_weights_ms": stats(ms[0]), "pb_beamform_kernel_ms": k, "pb_beamform_copy_out_ms": stats(ms[2]),
                "torch_ms": stats(tor), "spectra_bytes": once, "bytes_read": nbytes,
                "kernel_TB_per_s": nbytes / (k["median"] * 1e-3) / 1e12,
                "spectra_once_TB_per_s": once / (k["median"] * 1e-3) / 1e12,
                "torch_over_kernel": stats(tor)["median"] / k["median"]}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
