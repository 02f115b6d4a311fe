"""Compiled resource usage of the channelisers after the injection split (no GPU: hipcc cross-compiles gfx950).  The
power-plane kernels exist twice -- k_channelize / k_channelize_kur / k_channelize_pfb without any FRB injection code,
k_inject_chan / k_inject_chan_kur / k_inject_pfb with it -- and all six keep what the design counts on: no scratch
memory, at most 168 VGPRs, three workgroups per CU, the LDS of one FFT buffer.  The coherence twins stay two, with no
scratch and two workgroups per CU."""
import functools
import os

import pytest

from test_kernel_resources import _usage

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

LDS_FFT = 50000          # one 6250 x float2 buffer
LDS_KUR = LDS_FFT + 8    # + the row's mask and weight words (k_channelize_kur)
LDS_PFB = 4 * 12528      # four staged rows, reused as the FFT buffer


@functools.lru_cache(maxsize=None)
def _u(src):
    return _usage(src)


def _one(u, pred, what):
    hits = [(sym, v) for sym, v in u.items() if pred(sym)]
    assert len(hits) == 1, (what, [s for s, _ in hits])
    return hits[0][1]


def _hot(name, k, lds):
    assert k["ScratchSize"] == 0, (name, k)
    assert k["NumVgprs"] <= 168 and k["Occupancy"] >= 3, (name, k)
    assert k["LDSByteSize"] == lds, (name, k)


def test_power_plane_kernels_and_their_injecting_twins():
    u = _u("k_channelize.hip")
    _hot("k_channelize", _one(u, lambda s: s == "_Z12k_channelize8ChanArgs", "k_channelize"), LDS_FFT)
    _hot("k_channelize_kur", _one(u, lambda s: "k_channelize_kur" in s, "k_channelize_kur"), LDS_KUR)
    _hot("k_inject_chan", _one(u, lambda s: s == "_Z13k_inject_chan8ChanArgs", "k_inject_chan"), LDS_FFT)
    _hot("k_inject_chan_kur", _one(u, lambda s: "k_inject_chan_kur" in s, "k_inject_chan_kur"), LDS_KUR)


def test_coherence_twins_are_two_and_as_before():
    u = _u("k_channelize.hip")
    coh = {s: v for s, v in u.items() if "k_coh_chan" in s}
    assert len(coh) == 2, sorted(coh)
    for s, k in coh.items():
        assert k["ScratchSize"] == 0 and k["Occupancy"] >= 2, (s, k)
        assert k["LDSByteSize"] in (LDS_FFT, LDS_KUR), (s, k)


def test_pfb_kernel_and_its_injecting_twin():
    u = _u("k_channelize_pfb.hip")
    assert not any("k_channelize_pfb_kur" in s for s in u)
    _hot("k_channelize_pfb", _one(u, lambda s: "k_channelize_pfb7" in s, "k_channelize_pfb"), LDS_PFB)
    _hot("k_inject_pfb", _one(u, lambda s: "k_inject_pfb" in s, "k_inject_pfb"), LDS_PFB)
