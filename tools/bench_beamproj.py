"""Time of the projecting beamformer (pb_beamform_proj, tscr = 8) on one second of data -- R = 1024 x 10 segments, raw
stream -- at the shapes of tools/bench_beamform.py: 4 antennas with 4 beams, 8 antennas with 4 and 16 beams, with
pb_beamform on the same handle in the same run as the yardstick.  The matrices are projectors of random Hermitian
matrices (nulling.projectors, one null per pol and channel); their values do not change the kernel's work.  Device
times: the calls' own timers; warm-up, then REPEATS calls alternating between the two, median and min / max.  Every
antenna count is a step of its own, a child process under a time limit, and a step that fails ends the run: nothing
more is started on the card.  A call's outputs stay under the library's 2 GiB.  One JSON line on stdout (and in the
file given as the first argument).

    python tools/bench_beamproj.py profiles/beamproj_steptime.json"""
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, S, TSCR, WARMUP, REPEATS = 1024, 10, 8, 3, 15
NCO, TILE = 4096, 4                # (the beams of a workgroup of either kernel)
CASES = ((4, 4), (8, 4), (8, 16))
STEP_LIMIT_S = 300


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def step(nant):
    """one handle of nant antennas: {case: figures} for its beam counts"""
    import numpy as np
    import torch

    import bench
    lp = importlib.import_module("vlite-fast_amd.libpb")
    nulling = importlib.import_module("vlite-fast_amd.nulling")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(nant)
    x = rng.standard_normal((2, NCO, nant, 2 * nant)) + 1j * rng.standard_normal((2, NCO, nant, 2 * nant))
    proj, _ = nulling.projectors(np.einsum("pcir,pcjr->pcij", x, np.conj(x)), 1)
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
        for nbeam in [c[1] for c in CASES if c[0] == nant]:
            nout = S * R // TSCR
            assert nbeam * nout * 4 * NCO * 4 <= 2 << 30                  # the library's limit on a call's outputs
            delay = np.random.default_rng(nbeam).uniform(-200.0, 200.0, (nbeam, nant))
            plain, nulled = [[], [], []], [[], [], []]
            for k in range(WARMUP + REPEATS):
                beams, used = h.beamform(lp.CORR_RAW, S, delay, tscr=TSCR)
                t0 = h.beamform_timers()
                pbeams, pused = h.beamform_proj(lp.CORR_RAW, S, delay, proj, tscr=TSCR)
                t1 = h.beamform_proj_timers()
                if k >= WARMUP:
                    for i in range(3):
                        plain[i].append(t0[i])
                        nulled[i].append(t1[i])
            assert beams.shape == pbeams.shape == (nbeam, nout, 4, NCO) and int(pused.min()) == TSCR
            once = nant * 2 * S * R * NCO * 8
            kp, kn = stats(plain[1]), stats(nulled[1])
            out["A=%d beams=%d" % (nant, nbeam)] = {
                "pb_beamform_proj_weights_ms": stats(nulled[0]), "pb_beamform_proj_kernel_ms": kn,
                "pb_beamform_proj_copy_out_ms": stats(nulled[2]), "pb_beamform_weights_ms": stats(plain[0]),
                "pb_beamform_kernel_ms": kp, "spectra_bytes": once,
                "bytes_read": once * (-(-nbeam // TILE)),
                "kernel_TB_per_s": once * (-(-nbeam // TILE)) / (kn["median"] * 1e-3) / 1e12,
                "pb_beamform_kernel_TB_per_s": once * (-(-nbeam // TILE)) / (kp["median"] * 1e-3) / 1e12,
                "proj_over_plain": kn["median"] / kp["median"]}
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        print(json.dumps(step(int(sys.argv[2]))))
        return 0
    res = {"config": "R=1024 x 10 segments (1 s), raw stream, tscr 8, 8 bit; device ms per call: median, min, max of %d "
                     "calls after %d warm-up calls; pb_beamform on the same handle, the calls alternating" % (REPEATS, WARMUP),
           "cases": {}}
    for nant in sorted(set(c[0] for c in CASES)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(nant)], cwd=ROOT, stdout=subprocess.PIPE,
                           timeout=STEP_LIMIT_S)
        if r.returncode != 0:
            print("bench_beamproj: the step of %d antennas ended with %d; stopping" % (nant, r.returncode), file=sys.stderr)
            return 1
        res["cases"].update(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
