"""Step time of coherence output against -P 2 on the same box: full size (1024 rows x 10 segments = one second of one
antenna per step), rfi_mode 2, 8 bit, two buffer sets, the two modes alternated in rounds.  One JSON line on stdout
(and in the file given as the first argument): the median ms per step of each mode.

    python tools/coherence_steptime.py profiles/coherence_steptime.json"""
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

lp = importlib.import_module("vlite-fast_amd.libpb")
S, STEPS, ROUNDS = 10, 40, 3


def measure(coherence):
    h = lp.PbHandle(device=0, nant=1, nbit=8, npol=2, rfi_mode=2, rows_per_seg=1024, max_seg=S, nsets=2,
                    coherence=coherence)
    n = h.seg_samples
    dev = torch.device("cuda", 0)
    sec = bench.synth_second(torch, dev, 42, n, S, rfi_frac=0.0)
    torch.cuda.synchronize()
    for st in range(2):
        h.select_set(st)
        for s in range(S):
            h.submit_planar_dev(0, s, sec[s][0].data_ptr(), sec[s][1].data_ptr(), n)
    h.sync()
    for k in range(4):                     # warm-up
        h.select_set(k % 2)
        h.process(S)
    h.sync()
    t0 = time.perf_counter()
    for k in range(STEPS):
        h.select_set(k % 2)
        h.process(S)
        if k >= 1:
            h.select_set((k - 1) % 2)
            for st in (0, 1):
                v = h.fetch_view(0, st, S)
                int(v[0]) + int(v[-1])
    h.sync()
    ms = (time.perf_counter() - t0) * 1e3 / STEPS
    h.close()
    return ms


def main():
    res = {"P2": [], "P2_coherence": []}
    for _ in range(ROUNDS):
        res["P2"].append(measure(False))
        res["P2_coherence"].append(measure(True))
    out = {"config": "R=1024 x 10 segments per step (1 s of one antenna), rfi_mode 2, 8 bit, nsets 2",
           "ms_per_step": {k: statistics.median(v) for k, v in res.items()},
           "rounds": res}
    out["ratio"] = out["ms_per_step"]["P2_coherence"] / out["ms_per_step"]["P2"]
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
