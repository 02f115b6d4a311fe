"""Time of the beamformer (pb_beamform, tscr = 8) on one second of data -- R = 1024 x 10 segments, raw stream -- of 4
antennas with 4 beams and of 8 antennas with 4 and 16 beams, beside the same arithmetic in plain torch on complex64
tensors of the same shape on the same card: the baseline a user would otherwise write.  Device times:
pb_beamform_timers for the library, events for torch; warm-up, then REPEATS calls, median and min / max.  One JSON line
on stdout (and in the file given as the first argument): both figures, the bytes of spectra the kernel reads per call
(every beam tile of four reads them once) and the implied TB/s.

    python tools/bench_beamform.py profiles/beamform_steptime.json

--planes OUT.json [--parent-tree DIR]: pb_beam_planes (the beams as unit-variance planes that stay on the device) on the
same three cases with to_host=False, with and without a level handed in -- its four timers (uploads + weights + row
counts, beam kernel, level and plane kernels, copies to the host) -- beside pb_beamform's three timers for the same
arguments; with --parent-tree also those of the parent commit, measured by a child process that runs this tool as it
stands in DIR, a built checkout of that commit, before and after this library's calls, in the same session.  Per case the bytes that the level and plane
kernels must read (AA, BB and the row count of every value, once) and write, and the implied TB/s of stage 3 -- for
the call without a level also with the reads counted twice, which is what reaches memory if the second pass misses the
caches.

    python tools/bench_beamform.py --planes profiles/beam_planes_steptime.json --parent-tree /path/to/parent/checkout"""
import contextlib
import importlib
import json
import os
import statistics
import subprocess
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


@contextlib.contextmanager
def loaded_handle(nant):
    """a handle of nant antennas whose set holds one processed second"""
    dev = torch.device("cuda", 0)
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
        yield h


def time_library(nant, cases):
    """{nbeam: (weights ms, kernel ms, copy ms)} for one handle of nant antennas"""
    out = {}
    with loaded_handle(nant) as h:
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


def time_planes(nant, cases):
    """{nbeam: {"pb_beamform": 3 lists, "planes_level_in": 4 lists, "planes_own_level": 4 lists}}, the three calls taken in
    turn so that whatever else the card does meets all of them"""
    out = {}
    with loaded_handle(nant) as h:
        for nbeam in cases:
            delay = np.random.default_rng(nbeam).uniform(-200.0, 200.0, (nbeam, nant))
            ms = {"pb_beamform": [[], [], []], "planes_level_in": [[], [], [], []], "planes_own_level": [[], [], [], []]}
            level = None
            for k in range(WARMUP + REPEATS):
                h.beamform(lp.CORR_RAW, S, delay, tscr=TSCR)
                t = {"pb_beamform": h.beamform_timers()}
                none, ptr, level_out = h.beam_planes(lp.CORR_RAW, S, delay, tscr=TSCR, to_host=False)
                t["planes_own_level"] = h.beam_planes_timers()
                level = level_out if level is None else level
                h.beam_planes(lp.CORR_RAW, S, delay, tscr=TSCR, level=level, to_host=False)
                t["planes_level_in"] = h.beam_planes_timers()
                assert none is None and ptr and float(level_out.min()) > 0
                if k >= WARMUP:
                    for name, v in t.items():
                        for i, x in enumerate(v):
                            ms[name][i].append(x)
            out[nbeam] = ms
    return out


def parent_beamform(tree):
    """pb_beamform's timers per case from a child process that runs the tool of another checkout: {case: 3 stats}"""
    env = {k: v for k, v in os.environ.items() if k != "PB_LIBPATH"}
    r = subprocess.run([sys.executable, os.path.join(tree, "tools", "bench_beamform.py")], cwd=tree, env=env,
                       stdout=subprocess.PIPE, timeout=900)
    if r.returncode != 0:
        raise SystemExit("bench_beamform: the child in %s failed" % tree)
    cases = json.loads(r.stdout.decode().strip().splitlines()[-1])["cases"]
    return {name: [c["pb_beamform_weights_ms"], c["pb_beamform_kernel_ms"], c["pb_beamform_copy_out_ms"]] for name, c in cases.items()}


def total(parts):
    return sum(p["median"] for p in parts)


def main_planes(out_path, parent_tree):
    res = {"config": "R=1024 x 10 segments (1 s), raw stream, tscr 8, 8 bit; device ms per call: median, min, max of %d calls "
                     "after %d warm-up calls; pb_beam_planes with to_host=False (no plane is copied; its stage 4 is level_out "
                     "alone); parent: pb_beamform of the parent commit's library in a child process, before and after"
                     % (REPEATS, WARMUP), "cases": {}}
    before = parent_beamform(parent_tree) if parent_tree else None
    mine = {}
    for nant in sorted(set(c[0] for c in CASES)):
        for nbeam, ms in time_planes(nant, [c[1] for c in CASES if c[0] == nant]).items():
            mine[nant, nbeam] = ms
        torch.cuda.empty_cache()
    after = parent_beamform(parent_tree) if parent_tree else None
    for (nant, nbeam), ms in mine.items():
        name = "A=%d beams=%d" % (nant, nbeam)
        nval = nbeam * (S * R // TSCR) * NCO
        read_once, written = nval * 12, nval * 4
        c = {k: [stats(v) for v in lists] for k, lists in ms.items()}
        c["pb_beamform_total_ms"] = total(c["pb_beamform"])
        for k in ("planes_level_in", "planes_own_level"):
            c[k + "_total_ms"] = total(c[k])
        c["plane_bytes_read_once"], c["plane_bytes_written"] = read_once, written
        t_in, t_own = c["planes_level_in"][2]["median"] * 1e-3, c["planes_own_level"][2]["median"] * 1e-3
        c["level_in_read_TB_per_s"] = read_once / t_in / 1e12
        c["level_in_read_and_write_TB_per_s"] = (read_once + written) / t_in / 1e12
        c["own_level_read_once_TB_per_s"] = read_once / t_own / 1e12
        c["own_level_read_twice_TB_per_s"] = 2 * read_once / t_own / 1e12
        c["own_level_over_level_in"] = t_own / t_in
        if before:
            c["parent_pb_beamform_before"], c["parent_pb_beamform_after"] = before[name], after[name]
            c["parent_pb_beamform_total_ms"] = [total(before[name]), total(after[name])]
            c["device_resident_below_parent_total"] = bool(max(c["planes_level_in_total_ms"], c["planes_own_level_total_ms"])
                                                           < min(c["parent_pb_beamform_total_ms"]))
        res["cases"][name] = c
    line = json.dumps(res)
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--planes":
        return main_planes(sys.argv[2], sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "--parent-tree" else None)
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
