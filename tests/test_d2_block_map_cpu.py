"""k_detect2's block map (vlite-fast_amd/csrc/d2_block_map.h), built on the host: every (channel group, stream) is taken
by exactly one block of the 1-D grid, and with two streams every excised workgroup -- the long-lived kind -- is
dispatched before every raw one.  (The pairing the map was first written for, a channel group's two workgroups eight
blocks apart, spared no HBM fetch and made the step longer: profiles/r09_notes.md; it is not what ships.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCG = 128          # channel groups of 32 channels

PROG = r"""
#include <stdio.h>
#include "d2_block_map.h"
int main(void)
{
    for (int ns = 1; ns <= 2; ++ns)
        for (int b = 0; b < %d * ns; ++b) {
            d2_block m = d2_block_map(b, ns);
            printf("%%d %%d %%d %%d\n", ns, b, m.cg, m.stream);
        }
    return 0;
}
""" % NCG


@pytest.fixture(scope="module")
def block_map(tmp_path_factory):
    d = tmp_path_factory.mktemp("d2map")
    src, exe = str(d / "map.c"), str(d / "map")
    with open(src, "w") as f:
        f.write(PROG)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vlite-fast_amd", "csrc"), "-o", exe, src],
                   check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, check=True, timeout=60).stdout.decode().split("\n")
    maps = {1: {}, 2: {}}
    for line in out:
        if line.split():
            ns, b, cg, stream = map(int, line.split())
            maps[ns][b] = (cg, stream)
    return maps


@pytest.mark.parametrize("nstream", [1, 2])
def test_map_is_a_bijection(block_map, nstream):
    m = block_map[nstream]
    assert sorted(m) == list(range(NCG * nstream))
    assert sorted(m.values()) == [(cg, s) for cg in range(NCG) for s in range(nstream)]


def test_excised_workgroups_are_dispatched_first(block_map):
    m = block_map[2]
    assert all(m[b][1] == 1 for b in range(NCG)) and all(m[b][1] == 0 for b in range(NCG, 2 * NCG))
    assert all(m[b][0] == m[b + NCG][0] for b in range(NCG))
