"""The search's RFI cleaning without a GPU: argument refusals of pb_search_set_rfi, the CLI flags, the new kernels'
compiled resources, and the NumPy restatement (tests/search_rfi_ref.py) on hand-made rows."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import search_rfi_ref as R
from helpers import libpb
from test_kernel_resources import _usage

search = importlib.import_module("vlite-fast_amd.search")
EINVAL = -22          # PB_EINVAL


def test_set_rfi_refuses_bad_arguments():
    L = libpb().load()

    def err():
        return L.pb_search_last_error(None).decode()

    for tol in (0.0, -1.0, float("nan"), float("inf")):
        assert L.pb_search_set_rfi(None, 1, 1, tol, 16) == EINVAL and "tol" in err(), tol
    for bm in (0, -4, 3, 12, 128):
        assert L.pb_search_set_rfi(None, 1, 1, 5.0, bm) == EINVAL and "power of two" in err(), bm
    # good arguments: refused only for the missing handle
    for bm in (1, 2, 16, 64):
        assert L.pb_search_set_rfi(None, 1, 0, 5.0, bm) == EINVAL and "no search handle" in err(), bm
    n, b, ms = C.c_uint64(), C.c_int(), C.c_float()
    assert L.pb_search_rfi_info(None, C.byref(n), C.byref(b), C.byref(ms)) == EINVAL
    buf = (C.c_uint8 * 16)()
    assert L.pb_search_fetch_clean(None, buf, 16) == EINVAL


def test_cli_rfi_flags():
    ap = search.arg_parser()
    a = ap.parse_args(["-f", "x.fil"])
    assert (a.rfi_clean, a.rfi_tol, a.rfi_no_narrow, a.rfi_no_broad) == (False, 5.0, False, False)
    a = ap.parse_args(["-f", "x.fil", "-rfi_clean", "-rfi_tol", "3.5", "-rfi_no_narrow"])
    assert (a.rfi_clean, a.rfi_tol, a.rfi_no_narrow, a.rfi_no_broad) == (True, 3.5, True, False)
    a = ap.parse_args(["-f", "x.fil", "-rfi_clean", "-rfi_no_broad"])
    assert (a.rfi_clean, a.rfi_no_narrow, a.rfi_no_broad) == (True, False, True)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_cleaning_kernels_use_no_scratch():
    u = _usage("search_run.hip")
    for name in ("k_rfi_narrow", "k_rfi_broad_list", "k_rfi_broad_mask"):
        k = next(v for sym, v in u.items() if name in sym)
        assert k["ScratchSize"] == 0 and k["Occupancy"] >= 4, (name, k)
        assert k["LDSByteSize"] <= 8 * 1024, (name, k)
    # the reused stages stay scratch-free as well
    assert all(v["ScratchSize"] == 0 for v in u.values()), u


def test_restatement_median_and_mad_by_hand():
    assert R.med_mad(np.array([3, 1, 2], np.uint8)) == (2, 1)
    assert R.med_mad(np.array([1, 2, 3, 4], np.uint8)) == (2, 1)             # ceil(4/2) = 2 -> the lower median
    assert R.med_mad(np.array([0, 0, 0, 255], np.uint8)) == (0, 0)
    rng = np.random.default_rng(5)
    for n in (1, 7, 64, 1001):
        row = rng.integers(0, 256, n).astype(np.uint8)
        med, mad = R.med_mad(row)
        s = np.sort(row)
        assert med == s[(n + 1) // 2 - 1]
        assert mad == np.sort(np.abs(row.astype(int) - med))[(n + 1) // 2 - 1]


def test_restatement_narrow_flags_outliers_and_nothing_at_two_bits():
    rng = np.random.default_rng(6)
    xt = rng.integers(120, 136, (4, 500)).astype(np.uint8)
    xt[1, 17] = 250
    xt[2, 400] = 3
    out, n, meds = R.narrow(xt, [0, 1, 2], 5.0)
    assert n == 2 and out[1, 17] == meds[1] and out[2, 400] == meds[2]
    assert np.array_equal(out[3], xt[3])                                     # not in the channel list
    two = rng.integers(0, 4, (8, 300)).astype(np.uint8)
    assert R.narrow(two, range(8), 3.0)[1] == 0


def test_restatement_pack_roundtrip():
    rng = np.random.default_rng(7)
    for nbit in (2, 4, 8):
        x = rng.integers(0, 1 << nbit, (96, 64)).astype(np.uint8)
        assert np.array_equal(R.unpack(R.pack(x, nbit), 96, 64, nbit), x)
