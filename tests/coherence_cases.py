"""The seeded cases of the coherence chain (AA, BB, CR, CI; include/pb_hip.h), importable without a
GPU: tests/test_coherence_cases_cpu.py checks what they cover and holds tests/coherence_ref.py to the oracle on exactly
these inputs; tests/test_gpu_coherence_fuzz.py holds the GPU to tests/coherence_ref.py on them.

k_detect_coh<T, NBIT, MODE> has 18 instantiations (T = 32 when rows_per_seg % 32 == 0, else 8; 8 / 4 / 2 bits; RFI
mode 0 / 1 / 2).  seed % 18 fixes the instantiation, so each occurs three times in the 54 cases whatever the generator
draws; everything else -- rows per segment, segments per call, a max_seg beyond the call, batches, buffer sets, the lag
of the collection, one or two antennas with their OWN data, injection, keep_ave, and per antenna one content mutation
-- comes from the case's generator."""
import numpy as np

from helpers import make_input

NCASES = 54
STREAM_SEED = 7000                       # the generator of case `seed` is default_rng(STREAM_SEED + seed)
NKINDS = 7
PRODUCTS = ("AA", "BB", "CR", "CI")
NFFT = 12500


def instantiation(seed):
    """-> (T, nbit, rfi_mode) of case `seed`"""
    v = seed % 18
    return (32, 8)[v // 9], (8, 4, 2)[(v // 3) % 3], v % 3


def streams(rfi_mode):
    return (0,) if rfi_mode == 0 else (1,) if rfi_mode == 1 else (0, 1)


def _mutate(data, rng):
    """content the fixed fixtures do not have in these combinations: kinds 0 .. 4 are test_gpu_fuzz.py's, 5 and 6 are
    aimed at CR / CI (one pol with no power; one pol's row a square wave, the other pol's row plain noise)"""
    nsegs, _, n = data.shape
    kind = int(rng.integers(0, NKINDS))
    if kind == 0:                                          # one pol dead (code 128 = 0.0) for a whole segment
        data[int(rng.integers(0, nsegs)), int(rng.integers(0, 2))] = 128
    elif kind == 1:                                        # a saturated stretch crossing block boundaries
        s, p = int(rng.integers(0, nsegs)), int(rng.integers(0, 2))
        a = int(rng.integers(0, n - 3000))
        data[s, p, a:a + 2777] = 255
    elif kind == 2:                                        # dropped frames (code 0) scattered over both pols
        for _ in range(int(rng.integers(1, 5))):
            s, p = int(rng.integers(0, nsegs)), int(rng.integers(0, 2))
            a = 5000 * int(rng.integers(0, n // 5000))
            data[s, p, a:a + 5000] = 0
    elif kind == 3:                                        # a whole FFT row of square wave in both pols: weight 0
        s, row = int(rng.integers(0, nsegs)), int(rng.integers(0, n // NFFT))
        for p in range(2):
            seg = data[s, p, row * NFFT:(row + 1) * NFFT]
            seg[:] = np.where((np.arange(seg.size) // 5) % 2 == 0, 220, 36)
    elif kind == 4:                                        # the first segment entirely dropped (bandpass initialised later)
        data[0] = 0
    elif kind == 5:                                        # one pol dead in the FIRST segment: 0 / sqrt(0), bandpass 0
        data[0, int(rng.integers(0, 2))] = 128
    elif kind == 6:                                        # a whole FFT row of square wave in one pol only
        s, row, p = int(rng.integers(0, nsegs)), int(rng.integers(0, n // NFFT)), int(rng.integers(0, 2))
        seg = data[s, p, row * NFFT:(row + 1) * NFFT]
        seg[:] = np.where((np.arange(seg.size) // 5) % 2 == 0, 220, 36)
    return kind


def case(seed, with_data=True):
    """-> dict: T, nbit, rfi_mode, R, nseg (segments per call), max_seg, nb (calls), nsets, lag, nant, inject, keep_ave,
    kinds (the mutation of each antenna) and, unless with_data is False, datas: per antenna u8 [nseg * nb][2][R * 12500]"""
    assert 0 <= seed < NCASES
    T, nbit, rfi_mode = instantiation(seed)
    rng = np.random.default_rng(STREAM_SEED + seed)
    R = int(rng.choice([32, 64] if T == 32 else [8, 16, 24, 40, 72]))
    nseg = int(rng.integers(1, 4))
    max_seg = nseg + int(rng.integers(0, 2))               # the extra segment makes the handle's S > the call's nseg
    nb = int(rng.integers(1, 4))
    nsets = int(rng.integers(1, 4))
    lag = int(rng.integers(0, nsets))                      # batches in flight before the host collects (< nsets)
    nant = int(rng.choice([1, 1, 2]))
    inject = bool(rng.choice([False, False, True]))
    keep_ave = bool(rng.choice([True, True, False]))
    kinds, datas = [], []
    for a in range(nant):
        rfi, dropped = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        if with_data:
            d = make_input(900 + 10 * seed + a, R, nseg * nb, rfi=rfi, dropped=dropped)
        else:                                              # the mutation's draws need the shape only
            d = np.empty((nseg * nb, 2, R * NFFT), np.uint8)
        kinds.append(_mutate(d, rng))
        datas.append(d)
    c = dict(seed=seed, T=T, nbit=nbit, rfi_mode=rfi_mode, R=R, nseg=nseg, max_seg=max_seg, nb=nb, nsets=nsets, lag=lag,
             nant=nant, inject=inject, keep_ave=keep_ave, kinds=kinds)
    if with_data:
        c["datas"] = datas
    return c


def describe(c):
    """the case without its data, for a failure message"""
    return {k: v for k, v in c.items() if k != "datas"}


def f32_diff(got, ref):
    """-> how many elements of got differ from ref: equal as uint32 where ref is not NaN, NaN where ref is NaN (the sign
    and payload of a NaN are not part of the definition: the CPU's and the GPU's default NaN differ)"""
    got, ref = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(ref, np.float32).ravel()
    assert got.size == ref.size, (got.size, ref.size)
    nr = np.isnan(ref)
    return int(np.where(nr, ~np.isnan(got), got.view(np.uint32) != ref.view(np.uint32)).sum())
