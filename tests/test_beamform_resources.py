"""The beamformer's kernels' compiled resource usage (no GPU: hipcc cross-compiles gfx950): the weight, prefix and beam
kernels (one instantiation per antenna count 1..8) and no others, each with its resource lines, no scratch memory, no
LDS, no atomics, no inline assembly."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vlite-fast_amd", "csrc")
FLAGS = ("-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt "
         "-fno-gpu-flush-denormals-to-zero -I../../include -I. -w --cuda-device-only -S -o -").split()
KERNELS = ("k_beam_weights", "k_beam_prefix") + tuple("k_beamformILi%dEE" % n for n in range(1, 9))
LINES = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_beamform_kernels_use_no_scratch():
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["pb_beamform.hip"], cwd=CSRC, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    asm = r.stdout.decode()
    use, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"^; (%s): (\d+)" % "|".join(LINES), line)
        if m and cur:
            use.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    assert len(use) == len(KERNELS), sorted(use)                    # every kernel of the file is on the list
    for name in KERNELS:
        k = [v for sym, v in use.items() if name in sym]
        assert len(k) == 1, name
        print(name, k[0])
        assert sorted(k[0]) == sorted(LINES), (name, k[0])
        assert k[0]["ScratchSize"] == 0, (name, k[0])
        assert k[0]["LDSByteSize"] == 0, (name, k[0])
    assert "global_load_dwordx2" in asm and "atomic" not in asm
    src = open(os.path.join(CSRC, "pb_beamform.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)                    # no inline assembly
