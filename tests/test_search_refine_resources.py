"""The refinement kernels' compiled resource usage (no GPU: hipcc cross-compiles gfx950): no scratch memory, LDS within
what lets several workgroups share a CU, and no inline assembly in their source."""
import os

import pytest

from kernel_resources import CSRC, HIPCC, compile_usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_refinement_kernels_use_no_scratch():
    use, _ = compile_usage("search_refine.hip")
    for name in ("k_refine_series", "k_refine_dm", "k_refine_width"):
        k = [v for sym, v in use.items() if name in sym]
        assert len(k) == 1, name
        assert k[0]["ScratchSize"] == 0 and k[0]["LDSByteSize"] <= 32 * 1024 and k[0]["Occupancy"] >= 4, (name, k[0])
    sec = open(os.path.join(CSRC, "search_refine.hip")).read()
    assert "k_refine_series" in sec and "k_refine_width" in sec and "asm" not in sec
