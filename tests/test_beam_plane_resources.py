"""The beam-plane kernels' compiled resource usage (no GPU: hipcc cross-compiles gfx950): the three instantiations of
k_beam_plane and k_beam_level and no others, each with its resource lines, no scratch memory, no atomics, no inline
assembly, dword loads and stores per lane."""
import os
import re

import pytest

from kernel_resources import CSRC, HIPCC, LINES, compile_usage

KERNELS = ("k_beam_planeILb1ELb1EE", "k_beam_planeILb1ELb0EE", "k_beam_planeILb0ELb1EE", "k_beam_level")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_beam_plane_kernels_use_no_scratch_and_no_atomics():
    use, asm = compile_usage("pb_beam_plane.hip")
    assert len(use) == len(KERNELS), sorted(use)
    for name in KERNELS:
        k = [(sym, v) for sym, v in use.items() if name in sym]
        assert len(k) == 1, name
        sym, v = k[0]
        print(name, "NumVgprs %d  Occupancy %d  %s" % (v["NumVgprs"], v["Occupancy"], v))
        assert sorted(v) == sorted(LINES), (name, v)
        assert v["ScratchSize"] == 0, (name, v)
        assert v["LDSByteSize"] == 0, (name, v)
        assert v["Occupancy"] >= 4, (name, v)              # 256 lanes, 40 registers: latency hidden by waves
    assert "atomic" not in asm
    assert "global_load_dword" in asm and "global_store_dword" in asm
    src = open(os.path.join(CSRC, "pb_beam_plane.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)            # no inline assembly
