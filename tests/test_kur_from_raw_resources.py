"""What leaving the unflagged rows out of the excised plane may not cost (no GPU: hipcc cross-compiles gfx950): the power
channelisers keep no scratch and three workgroups per CU, and detect's excised-stream kernels -- with the loader's
source select, and for the rectangular window two more waves that convert in LDS -- keep no scratch and an LDS
footprint that still lets a detect workgroup sit beside two channeliser workgroups."""
import os
import re

import pytest

from test_kernel_resources import _usage

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

D2 = re.compile(r"^_Z9k_detect2ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEv")       # T, NPOL, NBIT, MODE, DEPTH, CONV


def test_power_channelisers_keep_three_workgroups_per_cu():
    u = _usage("k_channelize.hip")
    u.update(_usage("k_channelize_pfb.hip"))
    names = ("_Z12k_channelize8", "k_channelize_kur", "k_inject_chan8", "k_inject_chan_kur", "k_channelize_pfb7", "k_inject_pfb7")
    for name in names:
        k = next(v for sym, v in u.items() if name in sym)
        assert k["ScratchSize"] == 0 and k["NumVgprs"] <= 168 and k["Occupancy"] >= 3, (name, k)
        assert k["LDSByteSize"] <= 163840 // 3, (name, k)


def test_detect_excised_kernels():
    u = {D2.match(sym).groups(): v for sym, v in _usage("k_detect2.hip").items() if D2.match(sym)}
    assert u
    kinds = set()
    for (T, npol, nbit, mode, depth, conv), v in u.items():
        if mode == "0":
            continue
        assert v["ScratchSize"] == 0, ((T, npol, nbit, mode, depth, conv), v)
        assert v["LDSByteSize"] <= 66 * 1024, ((T, npol, nbit, mode, depth, conv), v)
        kinds.add((mode, conv))
    # mode 1 has no raw plane to take rows from; mode 2 always does: as they are (taps 4) or converted (taps 1)
    assert kinds == {("1", "0"), ("2", "1"), ("2", "2")}
    # the headline kernel: chunks of 32 rows, three requested ahead, conversion waves: beside two 50 000-byte
    # channeliser workgroups in the CU's 160 KB
    head = u[("32", "1", "8", "2", "3", "2")]
    assert head["LDSByteSize"] + 2 * 50000 <= 163840, head
