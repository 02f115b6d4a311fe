"""The recipe that compiles the reference's own kernel file (oracle/ref_kernels.mk): it builds both libraries from a
clean _ref/, they export refk_* and none of the reference's kernel names, and nothing of oracle/_ref is in git.

No GPU needed: hipcc cross-compiles.  The build part runs where the reference's source is present (the build container);
elsewhere the libraries that travelled with the tree are inspected, if there are any."""
import os
import shutil
import subprocess

import pytest

from helpers import ROOT
from ref_kernels import ENTRY_POINTS, KERNEL_NAMES, LIBS, REF_DIR

ORACLE = os.path.join(ROOT, "oracle")
REF_SRC = "/root/reference/src/pb_kernels.cu"
RECIPE = ("ref_kernels.mk", "ref_kernels.map", "ref_kernels_driver.hip", os.path.join("ref_shim", "cufft.h"))


def dynamic_symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, check=True).stdout.decode()
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def check_exports(path):
    syms = dynamic_symbols(path)
    assert sorted(s for s in syms if s.startswith("refk_")) == sorted(ENTRY_POINTS)
    # nothing else: not the kernels (plain or mangled, code or handle), not the driver's helpers
    assert [s for s in syms if not s.startswith("refk_")] == []
    for k in KERNEL_NAMES:
        assert not any(k in s and not s.startswith("refk_") for s in syms), k


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if not (os.path.exists(REF_SRC) and os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("the reference's src/pb_kernels.cu or hipcc is not on this machine")
    d = tmp_path_factory.mktemp("ref_kernels_build")
    for f in RECIPE:
        os.makedirs(os.path.dirname(os.path.join(str(d), f)), exist_ok=True)
        shutil.copy(os.path.join(ORACLE, f), os.path.join(str(d), f))
    assert not os.path.exists(os.path.join(str(d), "_ref"))
    r = subprocess.run(["make", "-j2", "-C", str(d), "-f", "ref_kernels.mk"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600)
    assert r.returncode == 0, r.stdout.decode()
    return str(d), r.stdout.decode()


def test_recipe_builds_both_libraries_from_a_clean_ref(built):
    d, log = built
    assert "warning" not in log.lower(), log                 # the reference's file compiles as it lies, with no warning
    for name in LIBS.values():
        assert os.path.getsize(os.path.join(d, "_ref", name)) > 10000
    # the two differ in the one flag, written out on each line
    lines = [l for l in log.splitlines() if "pb_kernels.cu" in l and "hipcc" in l]
    assert len(lines) == 2
    strict = [l for l in lines if "libref_kernels.so" in l][0]
    fmad = [l for l in lines if "libref_kernels_fmad.so" in l][0]
    assert "-ffp-contract=off" in strict and "-ffp-contract=fast" in fmad
    for l in lines:
        for flag in ("--offload-arch=gfx950", "-O2", "-fvisibility=hidden", "-fhip-fp32-correctly-rounded-divide-sqrt",
                     "-fno-fast-math"):
            assert flag in l.split(), (flag, l)
        assert "xnack" not in l and "-ffast-math" not in l.split()


def test_fresh_libraries_export_refk_only(built):
    for name in LIBS.values():
        check_exports(os.path.join(built[0], "_ref", name))


def test_libraries_in_the_tree_export_refk_only():
    have = [os.path.join(REF_DIR, n) for n in LIBS.values() if os.path.exists(os.path.join(REF_DIR, n))]
    if not have:
        pytest.skip("oracle/_ref/libref_kernels*.so not built in this tree")
    for path in have:
        check_exports(path)


def test_nothing_of_ref_is_committed():
    ignore = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "oracle/_ref/" in ignore and "*.so" in ignore
    if os.path.isdir(os.path.join(ROOT, ".git")) and shutil.which("git"):
        r = subprocess.run(["git", "-C", ROOT, "ls-files", "oracle/_ref"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode == 0:
            assert r.stdout.decode().strip() == ""
    # the committed recipe holds no kernel: every __global__ comes from the reference's file
    src = open(os.path.join(ORACLE, "ref_kernels_driver.hip")).read()
    assert "__global__ void" not in src and "__device__" not in src
    shim = [l for l in open(os.path.join(ORACLE, "ref_shim", "cufft.h")).read().splitlines() if l.strip()]
    assert shim == ["#include <hip/hip_runtime.h>", "typedef float cufftReal;", "typedef float2 cufftComplex;"]
