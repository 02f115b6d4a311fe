"""Byte-equality of every output of the search between this tree's libpb_hip.so and another build of the same ABI
(--parent PATH: the parent commit's library), both loaded into this one process: the same inputs go through both and
each output array must agree byte for byte.  Cases: a saturated block (every code 255, 515 active channels), a noise
block with a pulse and the stages switched off and on again with another geometry, and a random geometry with RFI
cleaning and a running baseline on.  Outputs: S/N and width planes, statistics, series, the cleaned block, the four
cutout arrays, the six refinement outputs, the giant list and the candidates.  Prints one JSON line; exit status 1 on
any difference.  The third case is made in the style of tests/test_gpu_search.py's random geometries but is not one of
their seeded draws (its own seed, 96 channels, a fixed band), and the second draws its own noise.

    python tools/search_equal.py --parent /path/to/parent/libpb_hip.so --out profiles/search_refactor_equal.json
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
libpb = importlib.import_module("vlite-fast_amd.libpb")
search = importlib.import_module("vlite-fast_amd.search")
FCH1, FOFF = 361.94, -0.16


def bind(path):
    """make the package's loader bind `path` (None: this tree's library); the searchers made from now on use it"""
    libpb.LIB_PATH = path or os.path.join(HERE, "..", "vlite-fast_amd", "csrc", "libpb_hip.so")
    libpb._lib = None
    return libpb.load()


def stages(s, out, tag, cut, ref, gi, reqs_cut, reqs_ref, thresh):
    s.set_cutouts(**cut)
    s.set_refine(**ref)
    s.set_giants(**gi)
    c = s.cutouts(*zip(*reqs_cut))
    out.update({"%s.cut.%s" % (tag, k): c[k] for k in ("ft", "ft_hits", "dt", "dt_hits")})
    f = s.refine_raw(*zip(*reqs_ref), want_series=True)
    out.update({"%s.rf.%s" % (tag, k): f[k] for k in ("status", "sn_dm", "kbest", "opt_sn", "opt_loc", "series")})
    g = s.giants(thresh, want_list=True)
    out.update({"%s.gi.%s" % (tag, k): np.asarray(v) for k, v in g.items() if k != "giant_list"})
    out.update({"%s.gl.%s" % (tag, k): v for k, v in g["giant_list"].items()})


def run_block(s, out, tag, codes):
    r = s.run(codes, want_series=True)
    out.update({"%s.%s" % (tag, k): r[k] for k in ("snr", "width_log2", "stats", "series")})
    out[tag + ".clean"] = s.fetch_clean()
    return r["tout"]


def outputs():
    """every case through the library that is bound now: {name: array}"""
    out = {}
    # the saturated block
    with search.Searcher(nchan=520, max_samples=1024, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_min=0.0, dm_max=20.0,
                         dm_step=4.0, boxcar_max=4, zap=((0, 5),)) as s:
        tout = run_block(s, out, "sat", np.full((1024, 520), 255, np.uint8))
        stages(s, out, "sat", dict(nsub=4, nt=8, ndmrow=2, max_cands=3), dict(nstep=3, half_window=16, wmax=4, max_cands=2),
               dict(sep_time=3, sep_dm=2, sep_filter=3, max_giants=1 << 12),
               [(1, 5, 1), (3, tout // 2, 2), (5, tout - 1, 8)], [(5, 3, 2.0, 4.0), (tout // 2, 3, 2.0, 4.0)], 0.0)
    # noise and a pulse; the stages off and on again with another geometry
    rng = np.random.default_rng(91)
    codes = np.clip(np.floor(rng.normal(127.5, 33.8, (2048, 64))), 0, 255).astype(np.uint8)
    delay = np.round(4.148808e3 * 40.0 * ((FCH1 + FOFF * np.arange(64)) ** -2 - FCH1 ** -2) / search.TSAMP).astype(int)
    for c in range(64):
        codes[700 + delay[c]:704 + delay[c], c] = np.minimum(codes[700 + delay[c]:704 + delay[c], c].astype(int) + 27, 255)
    with search.Searcher(nchan=64, max_samples=2048, fch1=FCH1, foff=FOFF, tsamp=search.TSAMP, dm_min=0.0, dm_max=80.0,
                         dm_step=4.0, boxcar_max=16, zap=()) as s:
        tout = run_block(s, out, "cyc", codes)
        rc, rr = [(2, 40, 1), (9, tout - 3, 4)], [(700, 4, 30.0, 1.5), (30, 1, 30.0, 1.5)]
        stages(s, out, "cyc1", dict(nsub=4, nt=16, ndmrow=4, max_cands=4), dict(nstep=8, half_window=64, wmax=8, max_cands=4),
               dict(sep_time=3, sep_dm=5, sep_filter=3, max_giants=1 << 14), rc, rr, 3.0)
        s.set_cutouts(max_cands=0)
        s.set_refine(max_cands=0)
        s.set_giants(max_giants=0)
        stages(s, out, "cyc2", dict(nsub=8, nt=24, ndmrow=2, max_cands=2), dict(nstep=5, half_window=40, wmax=16, max_cands=3),
               dict(sep_time=8, sep_dm=2, sep_filter=1, max_giants=1 << 12), rc, rr, 3.0)
    # a random geometry (odd block length, a zapped notch), RFI cleaning and a running baseline on
    rng = np.random.default_rng(4003)
    nchan, fch1, foff = 96, float(np.float32(355.3)), float(np.float32(-48.0 / 96))
    kw = dict(nchan=nchan, fch1=fch1, foff=foff, tsamp=float(np.float32(search.TSAMP)), dm_min=0.0, dm_max=60.0, dm_step=5.0,
              boxcar_max=16, zap=((32, 41),))
    with search.Searcher(max_samples=8192, **kw) as s0:
        T = s0.max_delay + 2049
    codes = rng.integers(0, 256, (T, nchan)).astype(np.uint8)
    codes[1000:1003] = 250                                          # a broad-band impulse for the broad pass
    codes[::97, 7] = 255                                            # outliers for the narrow pass
    with search.Searcher(max_samples=T, **kw) as s:
        s.set_baseline(500)
        s.set_rfi(True, True, 4.0, 8)
        tout = run_block(s, out, "rnd", codes)
        info = s.rfi_info()
        out["rnd.rfi"] = np.array([info["n_narrow"], info["n_broad_samples"]])
        stages(s, out, "rnd", dict(nsub=6, nt=32, ndmrow=6, max_cands=3), dict(nstep=16, half_window=100, wmax=32, max_cands=2),
               dict(sep_time=3, sep_dm=200, sep_filter=3, max_giants=1 << 14),
               [(0, 0, 64), (6, tout // 3, 16), (12, tout - 1, 2)], [(100, 7, 10.0, 0.5), (tout - 2, 32, 55.0, 1.0)], 3.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's libpb_hip.so")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bind(None)
    mine = outputs()
    bind(os.path.abspath(a.parent))
    theirs = outputs()
    differ = sorted(k for k in set(mine) | set(theirs)
                    if k not in mine or k not in theirs or mine[k].dtype != theirs[k].dtype or mine[k].shape != theirs[k].shape
                    or mine[k].tobytes() != theirs[k].tobytes())
    res = dict(tool="search_equal", arrays=len(mine), bytes=int(sum(v.nbytes for v in mine.values())), differ=differ,
               equal=not differ, rnd_rfi=[int(v) for v in mine["rnd.rfi"]], giants={t: int(mine[t + ".gi.ngiants"]) for t in
                                                                                   ("sat", "cyc1", "cyc2", "rnd")})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if not differ else 1


if __name__ == "__main__":
    sys.exit(main())
