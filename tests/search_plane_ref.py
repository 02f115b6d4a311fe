"""NumPy restatement of pb_search_push_f32's quantiser (include/pb_hip.h), operation by operation: a binary32 product, a
binary64 quotient and sum, the sum rounded to binary32, a three-way select that sends NaN to 0, a truncating cast.  For
every value that is not a NaN it is the reference's sel_and_dig_8b (src/pb_kernels.cu:711-735;
tests/test_search_plane_cpu.py pins it to the oracle's)."""
import numpy as np

STEP, MID = 0.02957, 127.5


def quantise8(plane, scale=1.0):
    """plane: float32, any shape -> uint8 of the same shape"""
    x = np.asarray(plane, np.float32)
    with np.errstate(all="ignore"):
        v = x * np.float32(scale)                                   # binary32
        assert v.dtype == np.float32
        tmp = (v.astype(np.float64) / STEP + MID).astype(np.float32)
        pos = tmp > 0                                               # False for NaN
        inner = np.where(pos & (tmp < 255), tmp, np.float32(0)).astype(np.uint8)      # the cast truncates
    return np.where(pos, np.where(tmp >= 255, np.uint8(255), inner), np.uint8(0)).astype(np.uint8)


def edges():
    """float32((k - 127.5) * 0.02957) for k = 0 .. 256 and its two neighbours in binary32 on each side: every cell edge of
    the quantiser, approached from both sides"""
    e = ((np.arange(257) - MID) * STEP).astype(np.float32)
    out = [e]
    lo = hi = e
    for _ in range(2):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.concatenate(out).astype(np.float32)


SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, 1e30, -1e30], np.float32)


def test_values(seed, n):
    """n float32 values: a unit-variance Gaussian with the edges, the specials and NaN planted at seeded places"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, n).astype(np.float32)
    plant = np.concatenate([edges(), SPECIAL, np.array([np.nan, -np.nan], np.float32)])
    reps = max(1, min(3, n // (4 * plant.size)))
    where = rng.choice(n, size=min(n, reps * plant.size), replace=False)
    x[where] = np.resize(plant, where.size)
    return x


test_values.__test__ = False
