#!/usr/bin/env python3
"""Generate tests/golden/reference_refine.npz by IMPORTING the reference's own refinement code.

Run in the build container only (needs /root/reference):   python tests/golden/make_refine_golden.py

What is pinned: analysis/loc_step0.py refine_dm and optimize_pulse, analysis/utils.py tophat_smooth and qn, run the way
loc_step0.py's script part chains them (optimize_pulse at the candidate DM, refine_dm at the width it finds,
optimize_pulse at the refined DM) on integer-valued seeded planes of the reference's own geometry (6251 channels,
320-384 MHz, chan_mask, 781.25 us): one with the pulse in the middle of the series and one with the pulse in the
series' first samples, where the window is clipped at 0 and tophat_smooth's edge ramp carries the maximum.

Only the inputs' seeds and parameters and the reference's OUTPUTS are stored; no reference source text is copied.  The
import goes the way make_golden.py's does: loc_step0.py is a script over private data paths, so only its function
definitions are compiled, into a namespace that also holds its module-level `fref`."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth  # noqa: E402

REF = "/root/reference/analysis"
NCHAN, TSAMP, FREF = 6251, 12500 * 8 / 128e6, 361.9414488190918
H = 128

# name: seed, ntime, dm, first pulse sample t0, pulse length, amplitude (codes per channel), t_pk handed to the
# refinement, dm0 it starts from, delta_dm, dm_range
CASES = {
    "mid": (31, 1536, 56.77, 700, 5, 6.0, 702, 56.70, 0.02, 0.2),
    "edge": (32, 1280, 56.77, 1, 6, 8.0, 3, 56.83, 0.02, 0.2),
}


def mask_channels():
    """the channels chan_mask() keeps (its complement is in reference_python.npz: s1_chan_mask_idx)"""
    m = np.zeros(NCHAN, bool)
    m[2350:6200] = True
    m[3123:3128] = False
    m[4297] = False
    m[4988:4992] = False
    return m


def plane(seed, ntime, dm, t0, plen, amp):
    """[1][6251][ntime] float32 of integer codes 0..255: noise about 100 with sigma 20 and a dispersed top-hat pulse in
    the channels chan_mask keeps; channel c at get_vlite_chan_freqs(6251)[c] MHz, delays as loc_step0.dedisperse rounds
    them, relative to FREF"""
    g = synth.gauss(seed, NCHAN * ntime).reshape(NCHAN, ntime) * 20.0 + 100.0
    freqs = ((np.arange(NCHAN)) * 64. / NCHAN + 320)[::-1]
    delays = np.round(dm * 4.15e-3 * ((freqs * 1e-3) ** -2 - (FREF * 1e-3) ** -2) / TSAMP).astype(int)
    for c in np.nonzero(mask_channels())[0]:
        g[c, t0 + delays[c]:t0 + delays[c] + plen] += amp
    return np.clip(np.floor(g + 0.5), 0, 255).astype(np.float32)[None]


def import_reference():
    sys.path.insert(0, REF)
    import utils
    tree = ast.parse(open(os.path.join(REF, "loc_step0.py")).read())
    wanted = {"get_vlite_chan_freqs", "dedisperse", "chan_mask", "optimize_pulse", "refine_dm"}
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    ns = {"np": np, "utils": utils, "inplace_roll": utils.inplace_roll, "fref": FREF}
    exec(compile(ast.Module(body=body, type_ignores=[]), "loc_step0_functions", "exec"), ns)
    return utils, ns


def main():
    utils, loc0 = import_reference()
    out = {}
    assert np.array_equal(loc0["chan_mask"]() == 1, mask_channels())
    for name, (seed, ntime, dm, t0, plen, amp, t_pk, dm0, ddm, rng) in CASES.items():
        fb = plane(seed, ntime, dm, t0, plen, amp)
        i0, i1 = max(0, t_pk - H), min(ntime, t_pk + H)

        def series(d):
            work = fb.copy()
            loc0["dedisperse"](work, d, TSAMP, ref_freq=FREF)
            return (work[0] * loc0["chan_mask"]()[:, None]).sum(axis=0)

        widths, sns0, locs0 = loc0["optimize_pulse"](series(dm0), i0, i1)
        width = int(widths[np.argmax(sns0)])
        dms, sns = loc0["refine_dm"](fb, TSAMP, dm0, i0, i1, delta_dm=ddm, dm_range=rng, width=width)
        best = dms[np.argmax(sns)]
        q = series(best)
        widths1, sns1, locs1 = loc0["optimize_pulse"](q, i0, i1)
        out[name + "_params"] = np.array([seed, ntime, dm, t0, plen, amp, t_pk, dm0, ddm, rng, i0, i1])
        out[name + "_width"] = np.int64(width)
        out[name + "_opt0_sns"], out[name + "_opt0_locs"] = sns0, locs0
        out[name + "_dms"], out[name + "_sns"] = dms, sns
        out[name + "_widths"], out[name + "_opt_sns"], out[name + "_opt_locs"] = widths1, sns1, locs1
        out[name + "_qn_window"] = utils.qn(q[i0:i1])
        out[name + "_smooth"] = utils.tophat_smooth(q.copy(), width)[i0:i1]
        print(name, "width", width, "best dm", best, "sn", sns.max(), "argmax", np.argmax(sns), "loc", locs1[np.argmax(sns1)])
    path = os.path.join(HERE, "reference_refine.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
