"""The projecting beamformer's kernels' compiled resource usage (no GPU: hipcc cross-compiles gfx950): the weights kernel
and the beam kernel (one instantiation each per antenna count 1..8), the row-count prefix and no others, each with its
resource lines, no scratch memory, no LDS, no atomics, no inline assembly; the beam kernel at two waves per SIMD or
more."""
import os
import re

import pytest

from kernel_resources import CSRC, HIPCC, LINES, compile_usage

KERNELS = (("k_beamproj_prefix",) + tuple("k_beamproj_weightsILi%dEE" % n for n in range(1, 9))
           + tuple("k_beamform_projILi%dEE" % n for n in range(1, 9)))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_beamproj_kernels_use_no_scratch():
    use, asm = compile_usage("pb_beamproj.hip")
    assert len(use) == len(KERNELS), sorted(use)                    # every kernel of the file is on the list
    for name in KERNELS:
        k = [v for sym, v in use.items() if name in sym]
        assert len(k) == 1, name
        print(name, k[0])
        assert sorted(k[0]) == sorted(LINES), (name, k[0])
        assert k[0]["ScratchSize"] == 0, (name, k[0])
        assert k[0]["LDSByteSize"] == 0, (name, k[0])
        assert k[0]["Occupancy"] >= 2, (name, k[0])
    assert "global_load_dwordx2" in asm and "atomic" not in asm
    assert "v_pk_mul_f32" in asm and "v_pk_add_f32" in asm          # the pairs of beams stay packed
    src = open(os.path.join(CSRC, "pb_beamproj.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)                    # no inline assembly
