#!/usr/bin/env python3
"""Timing experiment: per-wave work / barrier-wait cycles of one k_detect2 workgroup (excised stream).
Needs a variant library built with -DD2_STAMP (tools/build_variants.sh) selected by PB_LIBPATH."""
import ctypes as C
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bench import synth_second

lp = importlib.import_module("vlite-fast_amd.libpb")
L = lp.load()
dev = torch.device("cuda", 0)
S = 10
PIPE = os.environ.get("D2_PIPE") == "1"      # as benchmarked: three buffer sets, detect beside the next channeliser
NSETS = 3 if PIPE else 1
h = lp.PbHandle(device=0, nant=1, nbit=8, npol=1, rfi_mode=2, rows_per_seg=1024, max_seg=S, nsets=NSETS,
                taps=int(os.environ.get("D2_TAPS", "1")))
sec = synth_second(torch, dev, 42, h.seg_samples, S)
torch.cuda.synchronize()
for st in range(NSETS):
    h.select_set(st)
    for s in range(S):
        h.submit_planar_dev(0, s, sec[s][0].data_ptr(), sec[s][1].data_ptr(), h.seg_samples)
h.sync()
def stamps():
    o = (C.c_ulonglong * 32)()
    rc = L.pb_internal_d2_stamps(o)
    assert rc == 0
    return list(o)


def run(nb):
    for k in range(nb):
        h.select_set(k % NSETS)
        h.process(S)
        if not PIPE:
            h.sync()
        elif k >= 2:
            h.select_set((k - 2) % NSETS)
            h.fetch_view(0, 1, S)
    h.sync()


run(12)
before = stamps()
run(42 if PIPE else 5)     # pipelined: 40 of the 42 detects run beside the next batch's channeliser
after = stamps()
out = [a - b for a, b in zip(after, before)]
rc = 0
nl = max(1, out[3])
names = {0: "A", int(os.environ.get("D2_WAVE_L", "5")): "L", 1: "B0", 2: "B1", 3: "B2", 9 - int(os.environ.get("D2_WAVE_L", "5")): "B3",
         6: "C0", 7: "C1"}          # C: the conversion waves (taps 1, RFI mode 2)
nstep = 10 * 1024 // 32 + 2
print("rc", rc, "steps", nstep, "launches", nl, "pipelined" if PIPE else "alone")
for w in range(8):
    if not out[w * 4 + 3]:
        continue
    work, wait, extra = out[w * 4] / nl, out[w * 4 + 1] / nl, out[w * 4 + 2] / nl
    print("wave %d %-3s work %8d (%6.0f/step)  barrier wait %8d (%6.0f/step)  dma wait %8d (%6.0f/step)"
          % (w, names.get(w, "?"), work, work / nstep, wait, wait / nstep, extra, extra / nstep))
h.close()

# when every workgroup of a launch started and ended (last 64 launches)
if hasattr(L, "pb_internal_d2_wg") or True:
    import numpy as np
    buf = (C.c_ulonglong * (64 * 256 * 4))()
    if L.pb_internal_d2_wg(buf) == 0:
        a = np.frombuffer(buf, dtype=np.uint64).reshape(64, 256, 4).astype(np.int64)
        n = a[:, 0, 3]
        order = np.argsort(n)
        # where and when the two workgroups of a channel group ran.  D2_PAIR_APART: blocks between partners -- 128 with
        # d2_block_map.h (the excised one first) and for a library from before it (grid (128, 2): the raw one first),
        # 8 for the paired order of profiles/r09_notes.md section 2
        apart = int(os.environ.get("D2_PAIR_APART", "128"))
        first = np.array([b for b in range(256) if (b % (2 * apart)) < apart])
        for i in order[-8:-2]:
            xcc = a[i, :, 2] & 0xff
            d0 = (a[i, first + apart, 0] - a[i, first, 0]) / 100.0      # us, second of the pair minus first
            d1 = (a[i, first + apart, 1] - a[i, first, 1]) / 100.0
            print("launch %3d: pairs %d apart on the same XCC %d of %d (workgroups per XCC %s) | second starts after first (us) "
                  "median %.1f p10 %.1f p90 %.1f | ends after median %.1f p10 %.1f p90 %.1f"
                  % (n[i], apart, int((xcc[first] == xcc[first + apart]).sum()), first.size,
                     np.bincount(xcc, minlength=8).tolist(), np.median(d0), np.percentile(d0, 10), np.percentile(d0, 90),
                     np.median(d1), np.percentile(d1, 10), np.percentile(d1, 90)))
        for i in order[-8:-2]:
            t0 = a[i, :, 0].min()
            st = (a[i, :, 0] - t0) / 100.0          # us
            en = (a[i, :, 1] - t0) / 100.0
            print("launch %3d: workgroup starts (us) min %.1f median %.1f p90 %.1f max %.1f | life median %.1f max %.1f | last end %.1f"
                  % (n[i], st.min(), np.median(st), np.percentile(st, 90), st.max(), np.median(en - st), (en - st).max(), en.max()))
