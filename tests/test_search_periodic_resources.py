"""The periodicity search's kernels' compiled resource usage (no GPU: hipcc cross-compiles gfx950): the three kernels and no
others, each with its resource lines, no scratch memory, LDS within what the source declares, no atomics, no inline
assembly."""
import os
import re

import pytest

from kernel_resources import CSRC, HIPCC, LINES, compile_usage

# what the source declares: k_ffa_eval's window rows win[4][2][FFA_MAXP] of 8 bytes and the four waves' bests wbest[4][4]
FFA_MAXP = 256
LDS = {"k_ffa_down": 0, "k_ffa_stage": 0, "k_ffa_eval": 4 * 2 * FFA_MAXP * 8 + 4 * 4 * 4}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_periodic_kernels_use_no_scratch_and_little_lds():
    use, asm = compile_usage("search_periodic.hip")
    assert len(use) == len(LDS), sorted(use)
    src = open(os.path.join(CSRC, "search_periodic.hip")).read()
    assert re.search(r"#define FFA_MAXP %d\b" % FFA_MAXP, src)
    assert re.search(r"__shared__ uint64_t win\[4\]\[2\]\[FFA_MAXP\];", src) and re.search(r"__shared__ int32_t wbest\[4\]\[4\];", src)
    assert len(re.findall(r"__shared__", src)) == 2
    for name, lds in LDS.items():
        k = [(sym, v) for sym, v in use.items() if name in sym]
        assert len(k) == 1, name
        sym, v = k[0]
        print(name, "NumVgprs %d  Occupancy %d  %s" % (v["NumVgprs"], v["Occupancy"], v))
        assert sorted(v) == sorted(LINES), (name, v)
        assert v["ScratchSize"] == 0, (name, v)
        assert v["LDSByteSize"] <= lds <= 163840, (name, v)
        assert v["Occupancy"] >= 4, (name, v)              # memory-bound passes of 256 lanes: latency hidden by waves
    assert "atomic" not in asm
    assert "asm" not in re.sub(r"//.*", "", src)            # no inline assembly
