"""The correlator's kernels' compiled resource usage (no GPU: hipcc cross-compiles gfx950): the tile kernels and the
prefix kernel and no others, no scratch memory, no LDS, no AGPRs, 8-byte loads of the spectra, no inline assembly."""
import os
import re

import pytest

from kernel_resources import CSRC, HIPCC, compile_usage

# k_correlate<NI, NJ, DIAG>: a group of 1..4 antennas against itself, and group 0 against 1 or 2 antennas of group 1
KERNELS = ("k_corr_prefix", "k_correlateILi1ELi1ELb1EE", "k_correlateILi2ELi2ELb1EE", "k_correlateILi3ELi3ELb1EE",
           "k_correlateILi4ELi4ELb1EE", "k_correlateILi4ELi1ELb0EE", "k_correlateILi4ELi2ELb0EE")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_correlate_kernels_use_no_scratch_and_no_lds():
    use, asm = compile_usage("pb_correlate.hip")
    assert len(use) == len(KERNELS), sorted(use)                    # every kernel of the file is on the list
    for name in KERNELS:
        k = [v for sym, v in use.items() if name in sym]
        assert len(k) == 1, name
        print(name, k[0])
        assert k[0]["ScratchSize"] == 0, (name, k[0])
        assert k[0]["LDSByteSize"] == 0, (name, k[0])
        assert k[0]["NumAgprs"] == 0, (name, k[0])                   # the accumulators are in VGPRs, none moved to an AGPR
    assert "global_load_dwordx2" in asm and "global_store_dwordx2" in asm and "atomic" not in asm
    src = open(os.path.join(CSRC, "pb_correlate.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)                    # no inline assembly
