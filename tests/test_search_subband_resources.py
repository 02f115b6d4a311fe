"""The sub-band search kernels' compiled resource usage (no GPU: hipcc cross-compiles gfx950): no scratch memory, LDS within
64 KiB per workgroup so that two workgroups fit a CU, no inline assembly."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vlite-fast_amd", "csrc")
FLAGS = ("-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt "
         "-fno-gpu-flush-denormals-to-zero -I../../include -I. -w --cuda-device-only -S -o -").split()
KERNELS = ("k_dedisperse_sub", "k_band_sum", "k_band_best")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_subband_kernels_use_no_scratch_and_little_lds():
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["search_subband.hip"], cwd=CSRC, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    use, cur = {}, None
    for line in r.stdout.decode().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", line)
        if m and cur:
            use.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    assert len(use) == len(KERNELS), sorted(use)                    # every kernel of the file is on the list
    for name in KERNELS:
        k = [v for sym, v in use.items() if name in sym]
        assert len(k) == 1, name
        assert k[0]["ScratchSize"] == 0 and k[0]["LDSByteSize"] <= 64 * 1024, (name, k[0])
    src = open(os.path.join(CSRC, "search_subband.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)                    # no inline assembly
