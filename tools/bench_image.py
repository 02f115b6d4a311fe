"""Time of the imager (pb_imager_run, DELAY mode, image only) on a 201 x 201 grid at 28 and at 153 baselines, beside the
same arithmetic in plain torch (binary64 phase, complex64 rotation and sums, pixels in chunks) on the same card and in
numpy on the host (a 21 x 21 grid, scaled by the pixel count).  Device times: pb_imager_timers for the library, events
for torch; warm-up, then REPEATS calls, median and min / max (torch: TORCH_REPEATS after one).  One JSON line on stdout
(and in the file given as the first argument): the times and the rotations per second (pixels x baselines x 2 slots x
4096 channels per call).

    python tools/bench_image.py profiles/image_steptime.json"""
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

lp = importlib.import_module("vlite-fast_amd.libpb")
N, N_HOST, WARMUP, REPEATS, TORCH_REPEATS, TORCH_CHUNK = 201, 21, 3, 15, 5, 64
NCO, CHANMIN = 4096, 2155


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def inputs(nbl, npix, seed=1):
    rng = np.random.default_rng(seed)
    u = (rng.standard_normal((nbl, 2, NCO)) + 1j * rng.standard_normal((nbl, 2, NCO))).astype(np.complex64)
    dd = rng.uniform(-4000, 4000, (npix, nbl))
    return u, dd


def time_library(u, dd):
    up, kern, back = [], [], []
    with lp.PbImager(u.shape[0], dd.shape[0]) as im:
        im.set_vis(u)
        for k in range(WARMUP + REPEATS):
            img = im.run(dd)
            if k >= WARMUP:
                ms = im.timers()
                up.append(ms[0])
                kern.append(ms[1])
                back.append(ms[2])
    return up, kern, back, img


def torch_image(u, dd, bins):
    out = []
    for p0 in range(0, dd.shape[0], TORCH_CHUNK):
        t = bins * (dd[p0:p0 + TORCH_CHUNK] / 12500.0)[:, :, None]          # [P][nbl][4096] binary64
        r = (t - torch.round(t)).to(torch.float32)
        rot = torch.polar(torch.ones_like(r), -2 * np.pi * r)
        z = torch.einsum("pbc,bsc->pbs", rot, u)
        out.append(z.abs().sum(dim=(1, 2)))
    return torch.cat(out)


def time_torch(u, dd):
    dev = torch.device("cuda", 0)
    tu, tdd = torch.from_numpy(u).to(dev), torch.from_numpy(dd).to(dev)
    bins = torch.arange(CHANMIN, CHANMIN + NCO, device=dev, dtype=torch.float64)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for k in range(1 + TORCH_REPEATS):
        a.record()
        img = torch_image(tu, tdd, bins)
        b.record()
        torch.cuda.synchronize()
        if k >= 1:
            ms.append(a.elapsed_time(b))
    return ms, img.cpu().numpy()


def numpy_image(u, dd):
    bins = (CHANMIN + np.arange(NCO)).astype(np.float64)
    out = np.empty(dd.shape[0], np.float32)
    for p in range(dd.shape[0]):
        t = bins * (dd[p] / 12500.0)[:, None]
        rot = np.exp(-2j * np.pi * (t - np.rint(t))).astype(np.complex64)
        out[p] = np.abs((u * rot[:, None, :]).sum(axis=-1)).sum()
    return out


def main():
    res = {"config": "%d x %d pixels, DELAY mode, image only; device ms per call: median, min, max of %d calls after %d "
                     "(torch: %d after 1, pixels in chunks of %d); numpy: one call of %d x %d pixels on the host, scaled "
                     "by the pixel count" % (N, N, REPEATS, WARMUP, TORCH_REPEATS, TORCH_CHUNK, N_HOST, N_HOST), "cases": {}}
    for nbl in (28, 153):
        u, dd = inputs(nbl, N * N)
        up, kern, back, img = time_library(u, dd)
        tms, timg = time_torch(u, dd)
        torch.cuda.empty_cache()
        t0 = time.time()
        nimg = numpy_image(u, dd[:N_HOST * N_HOST])
        host_s = (time.time() - t0) * (N * N) / float(N_HOST * N_HOST)
        rot = N * N * nbl * 2 * NCO
        k = stats(kern)
        res["cases"]["nbl=%d" % nbl] = {
            "upload_ms": stats(up), "kernel_ms": k, "copy_back_ms": stats(back), "torch_ms": stats(tms),
            "numpy_host_s_scaled": host_s, "rotations": rot, "rotations_per_s": rot / (k["median"] * 1e-3),
            "torch_over_kernel": stats(tms)["median"] / k["median"], "numpy_over_kernel": host_s * 1e3 / k["median"],
            "max_rel_diff_vs_torch": float(np.abs(img - timg).max() / np.abs(timg).max()),
            "max_rel_diff_vs_numpy": float(np.abs(img[:nimg.size] - nimg).max() / np.abs(nimg).max())}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
