"""The channel stage's kernels' compiled resource usage (no GPU: hipcc cross-compiles gfx950): the four kernels and no
others, no scratch memory, LDS within 16 KiB for all but the sort (whose LDS is dynamic: 8 bytes per padded channel), no
inline assembly."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vlite-fast_amd", "csrc")
FLAGS = ("-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt "
         "-fno-gpu-flush-denormals-to-zero -I../../include -I. -w --cuda-device-only -S -o -").split()
KERNELS = ("k_rfichan_moments", "k_rfichan_lag", "k_rfichan_vote", "k_rfichan_fill")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_rfichan_kernels_use_no_scratch_and_little_lds():
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["search_rfichan.hip"], cwd=CSRC, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    asm = r.stdout.decode()
    use, cur = {}, None
    for line in asm.splitlines():
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
        assert k[0]["ScratchSize"] == 0, (name, k[0])
        if name != "k_rfichan_lag":
            assert k[0]["LDSByteSize"] <= 16 * 1024, (name, k[0])
    # the moments are summed with the packed byte instructions, on 16-byte loads; the fill stores 16 bytes
    assert "v_sad_u8" in asm and "v_dot4_u32_u8" in asm and "global_load_dwordx4" in asm and "global_store_dwordx4" in asm
    src = open(os.path.join(CSRC, "search_rfichan.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)                    # no inline assembly
