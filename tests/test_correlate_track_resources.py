"""The fringe-stopping correlator's kernels' compiled resource usage (no GPU: hipcc cross-compiles gfx950): the tile
kernels and no others, no scratch memory, no LDS, two waves per SIMD, 8-byte loads of the spectra and stores of the
visibilities, the rows' table entries through scalar loads where a workgroup's first rows are equal, no atomics, no
inline assembly."""
import os
import re

import pytest

from kernel_resources import CSRC, HIPCC, compile_usage, kernel_text

# k_correlate_track<NI, NJ, DIAG>: k_correlate's tiles
KERNELS = ("k_correlate_trackILi1ELi1ELb1EE", "k_correlate_trackILi2ELi2ELb1EE", "k_correlate_trackILi3ELi3ELb1EE",
           "k_correlate_trackILi4ELi4ELb1EE", "k_correlate_trackILi4ELi1ELb0EE", "k_correlate_trackILi4ELi2ELb0EE")
# rows in flight x antennas read (csrc/pb_correlate_track.hip: track_rows_in_flight)
TABLE_LOADS = dict(zip(KERNELS, (16 * 1, 8 * 2, 5 * 3, 3 * 4, 2 * 5, 2 * 6)))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_tracked_kernels_use_no_scratch_and_no_lds():
    use, asm = compile_usage("pb_correlate_track.hip")
    assert len(use) == len(KERNELS), sorted(use)                    # every kernel of the file is on the list
    for name in KERNELS:
        k = [(sym, v) for sym, v in use.items() if name in sym]
        assert len(k) == 1, name
        sym, v = k[0]
        print(name, v)
        assert v["ScratchSize"] == 0, (name, v)
        assert v["LDSByteSize"] == 0, (name, v)
        assert v["NumVgprs"] + v["NumAgprs"] <= 256 and v["Occupancy"] >= 2, (name, v)      # two waves per SIMD
        text = kernel_text(asm, sym)
        assert "global_load_dwordx2" in text and "global_store_dwordx2" in text and "atomic" not in text
        assert "v_rndne_f64" in text                                 # the turn's rint, in binary64
        # a row's (s, p) per antenna of the tile is 16 bytes: vector loads in the loop of a workgroup whose first rows
        # differ, one per (row in flight, antenna) and row by row; scalar loads in the loop of one whose first rows are equal
        assert len(re.findall(r"global_load_dwordx4 ", text)) == TABLE_LOADS[name], name
        assert len(re.findall(r"s_load_dwordx(?:4|8|16) ", text)) >= 2 + 1, name      # (the arguments take two)
    src = open(os.path.join(CSRC, "pb_correlate_track.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)                    # no inline assembly
    assert "atomic" not in re.sub(r"//.*", "", src)
