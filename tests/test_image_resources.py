"""The imager's kernels' compiled resource usage (no GPU: hipcc cross-compiles gfx950): the two kernels and no others,
each with its resource lines, and no scratch memory."""
import os

import pytest

from kernel_resources import HIPCC, LINES, compile_usage

KERNELS = ("k_image_z", "k_image_sum")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_image_kernels_use_no_scratch():
    use, _ = compile_usage("pb_image.hip")
    assert len(use) == len(KERNELS), sorted(use)                    # every kernel of the file is on the list
    for name in KERNELS:
        k = [v for sym, v in use.items() if name in sym]
        assert len(k) == 1, name
        print(name, k[0])
        assert sorted(k[0]) == sorted(LINES), (name, k[0])
        assert k[0]["ScratchSize"] == 0, (name, k[0])
