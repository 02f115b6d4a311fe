"""The beamformer's kernels' compiled resource usage (no GPU: hipcc cross-compiles gfx950), one compilation for both
tests: the two weights kernels, the row-count prefix and the two beam kernels (one instantiation per antenna count 1..8
of each templated kernel) and no others, each with its resource lines, no scratch memory, no LDS, no atomics, no inline
assembly; every beam kernel's pairs of beams packed; the projecting call's kernels at two waves per SIMD or more."""
import os
import re

import pytest

from kernel_resources import CSRC, HIPCC, LINES, compile_usage, kernel_text

PLAIN = tuple("k_beamformILi%dEE" % n for n in range(1, 9))
# what the projecting call runs: the prefix serves both calls
PROJ = (("k_beam_prefix",) + tuple("k_beamproj_weightsILi%dEE" % n for n in range(1, 9))
        + tuple("k_beamform_projILi%dEE" % n for n in range(1, 9)))
KERNELS = ("k_beam_weights",) + PLAIN + PROJ

_compiled = []


def _checked(names):
    """the file compiled once; per name (symbol, resource lines), each with all its lines, no scratch and no LDS"""
    if not _compiled:
        _compiled.append(compile_usage("pb_beamform.hip"))
    use, asm = _compiled[0]
    assert len(use) == len(KERNELS) == 26, sorted(use)              # every kernel of the file is on the list
    out = {}
    for name in names:
        k = [(sym, v) for sym, v in use.items() if name in sym]
        assert len(k) == 1, name
        sym, v = out[name] = k[0]
        print(name, v)
        assert sorted(v) == sorted(LINES), (name, v)
        assert v["ScratchSize"] == 0, (name, v)
        assert v["LDSByteSize"] == 0, (name, v)
        if "k_beamform" in name:                                    # the pairs of beams stay packed, in each beam kernel
            text = kernel_text(asm, sym)
            assert "v_pk_mul_f32" in text and "v_pk_add_f32" in text, name
    assert "global_load_dwordx2" in asm and "atomic" not in asm
    src = open(os.path.join(CSRC, "pb_beamform.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)                    # no inline assembly
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_beamform_kernels_use_no_scratch():
    assert len(_checked(KERNELS)) == 26


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_beamproj_kernels_use_no_scratch():
    got = _checked(PROJ)
    assert len(got) == 17
    for name, (_, v) in got.items():
        assert v["Occupancy"] >= 2, (name, v)
