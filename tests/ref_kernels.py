"""ctypes face of oracle/_ref/libref_kernels{,_fmad}.so: the reference's own src/pb_kernels.cu, compiled as it lies for
gfx950 and launched by oracle/ref_kernels_driver.hip with the reference's grids (oracle/ref_kernels.mk).

TEST INFRASTRUCTURE ONLY.  The libraries are built where the reference's source is present and travel with the tree;
they are never committed.  `load()` first loads libpb_hip.so through libpb.load(), so that the process holds ONE HIP
runtime, and skips with a reason when the library is absent.

Also here: thin wrappers for the orc_* functions that oracle.py binds but does not wrap (the spectral kernels one by
one), so that a test can feed the same array to refk_X on the GPU and to orc_X on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
from helpers import ROOT, libpb

NFFT, NCHAN, NKURTO, NSCRUNCH, ROWS = O.NFFT, O.NCHAN, O.NKURTO, O.NSCRUNCH, 1024
BLK_PER_ROW = NFFT // NKURTO
SPEC_SHAPE = (2, ROWS, NCHAN)
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
LIBS = {"strict": "libref_kernels.so", "fmad": "libref_kernels_fmad.so"}
KERNEL_NAMES = ("convertarray", "kurtosis", "compute_dagostino", "compute_dagostino2", "block_kurtosis", "apply_kurtosis",
                "apply_kurtosis_fake", "histogram", "set_frb_delays", "inject_frb", "detect_and_normalize2",
                "detect_and_normalize3", "pscrunch", "pscrunch_weights", "tscrunch", "tscrunch_weights", "sel_and_dig_2b",
                "sel_and_dig_4b", "sel_and_dig_8b")
ENTRY_POINTS = tuple("refk_" + k for k in KERNEL_NAMES if k != "histogram") + ("refk_nsms", "refk_chain_time",
                                                                               "refk_chain_detect")
_loaded = {}


def lib_path(variant="strict"):
    return os.path.join(REF_DIR, LIBS[variant])


def load(variant="strict"):
    if variant in _loaded:
        return _loaded[variant]
    path = lib_path(variant)
    if not os.path.exists(path):
        pytest.skip("%s is not built: `make -C oracle -f ref_kernels.mk` needs the reference's src/pb_kernels.cu and "
                    "hipcc; the library is not committed and travels with the tree" % os.path.relpath(path, ROOT))
    libpb().load()                                          # one HIP runtime per process: libpb (and torch) first
    L = C.CDLL(path)
    fp, up, i, f, z = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_int, C.c_float, C.c_size_t
    sig = {
        "refk_nsms": [C.POINTER(C.c_int)],
        "refk_convertarray": [fp, up, z],
        "refk_kurtosis": [fp, fp, fp, z],
        "refk_compute_dagostino": [fp, fp, z],
        "refk_compute_dagostino2": [fp, fp, z],
        "refk_block_kurtosis": [fp, fp, fp, fp, fp, i],
        "refk_apply_kurtosis": [fp, fp, fp, fp, i, i],
        "refk_apply_kurtosis_fake": [fp, fp, fp, fp, i, i],
        "refk_set_frb_delays": [fp, f],
        "refk_inject_frb": [fp, fp, i, f, f],
        "refk_detect_and_normalize2": [fp, fp, f],
        "refk_detect_and_normalize3": [fp, fp, fp, f],
        "refk_pscrunch": [fp],
        "refk_pscrunch_weights": [fp, fp],
        "refk_tscrunch": [fp, fp, i],
        "refk_tscrunch_weights": [fp, fp, fp, i],
        "refk_sel_and_dig_2b": [fp, up, i],
        "refk_sel_and_dig_4b": [fp, up, i],
        "refk_sel_and_dig_8b": [fp, up, i],
        "refk_chain_time": [up, i, i] + [fp] * 9,
        "refk_chain_detect": [fp, fp, fp, fp, fp, fp, i, i, i, i, fp, fp, up, up, fp],
    }
    assert sorted(sig) == sorted(ENTRY_POINTS)
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = args, C.c_int
    _loaded[variant] = L
    return L


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _u(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ok(rc, what):
    if rc > 0:          # a HIP call failed: the device may be faulted, so nothing more is started on it in this session
        pytest.exit("%s: HIP status %d; no further GPU test is run after a failed HIP call" % (what, rc), returncode=3)
    assert rc == 0, "%s rejected its arguments" % what


def same_bits(a, b):
    return np.array_equal(_f32(a).view(np.uint32), _f32(b).view(np.uint32))


def same_bits_or_both_nan(a, b):
    """equal = the same bits, or NaN on both sides: the 0/0 of an all-zero block is -NaN on x86 and +NaN on the GPU"""
    a, b = _f32(a).ravel(), _f32(b).ravel()
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def bp_scale():
    """src/process_baseband.cu:739-741"""
    return float(np.float32(float(NFFT) / O.VLITE_RATE * NSCRUNCH / 1.0))


def spec_as_f32(spec):
    """complex64 [2][1024][6251] -> a fresh float32 copy [2][1024][6251][2] (the kernels work in place)"""
    a = np.array(spec, dtype=np.complex64, order="C").view(np.float32)
    assert a.size == 2 * 2 * ROWS * NCHAN
    return a


class Ref(object):
    """refk_* of one variant: NumPy in, NumPy out.  Shapes as the reference allocates them."""

    def __init__(self, variant="strict"):
        self.L = load(variant)
        self.variant = variant

    def nsms(self):
        n = C.c_int()
        _ok(self.L.refk_nsms(C.byref(n)), "refk_nsms")
        return n.value

    def convertarray(self, u):
        u = np.ascontiguousarray(u, np.uint8)
        out = np.empty(u.size, np.float32)
        _ok(self.L.refk_convertarray(_f(out), _u(u), u.size), "refk_convertarray")
        return out.reshape(u.shape)

    def kurtosis(self, time):
        time = _f32(time).ravel()
        nb = time.size // NKURTO
        pow_, kur = np.empty(nb, np.float32), np.empty(nb, np.float32)
        _ok(self.L.refk_kurtosis(_f(time), _f(pow_), _f(kur), nb), "refk_kurtosis")
        return pow_, kur

    def compute_dagostino(self, kur, which=0):
        kur = _f32(kur).ravel()
        dag = np.empty_like(kur)
        fn = self.L.refk_compute_dagostino2 if which else self.L.refk_compute_dagostino
        _ok(fn(_f(kur), _f(dag), kur.size // 2), "refk_compute_dagostino%s" % ("2" if which else ""))
        return dag

    def block_kurtosis(self, pow_, kur, dag):
        pow_, kur, dag = _f32(pow_).ravel(), _f32(kur).ravel(), _f32(dag).ravel()
        nfft = pow_.size // BLK_PER_ROW
        pb, kb = np.empty(nfft, np.float32), np.empty(nfft, np.float32)
        _ok(self.L.refk_block_kurtosis(_f(pow_), _f(kur), _f(dag), _f(pb), _f(kb), nfft), "refk_block_kurtosis")
        return pb, kb

    def apply_kurtosis(self, time, dag, inplace=False, fake=False):
        time, dag = _f32(time).ravel(), _f32(dag).ravel()
        nfft = time.size // NFFT
        out, norms = np.empty_like(time), np.empty(nfft, np.float32)
        fn = self.L.refk_apply_kurtosis_fake if fake else self.L.refk_apply_kurtosis
        _ok(fn(_f(time), _f(out), _f(dag), _f(norms), nfft, int(inplace)), "refk_apply_kurtosis")
        return out, norms

    def set_frb_delays(self, dm):
        d = np.empty(NCHAN, np.float32)
        _ok(self.L.refk_set_frb_delays(_f(d), C.c_float(dm)), "refk_set_frb_delays")
        return d

    def inject_frb(self, spec, delays, since, width, amp):
        a = spec_as_f32(spec)
        _ok(self.L.refk_inject_frb(_f(a), _f(_f32(delays)), since, C.c_float(width), C.c_float(amp)), "refk_inject_frb")
        return a

    def detect_and_normalize2(self, spec, bp):
        a, bp = spec_as_f32(spec), np.array(bp, np.float32)
        _ok(self.L.refk_detect_and_normalize2(_f(a), _f(bp), bp_scale()), "refk_detect_and_normalize2")
        return a, bp

    def detect_and_normalize3(self, spec, weights, bp):
        a, bp = spec_as_f32(spec), np.array(bp, np.float32)
        _ok(self.L.refk_detect_and_normalize3(_f(a), _f(_f32(weights)), _f(bp), bp_scale()), "refk_detect_and_normalize3")
        return a, bp

    def pscrunch(self, planes):
        a = np.array(planes, np.float32)
        _ok(self.L.refk_pscrunch(_f(a)), "refk_pscrunch")
        return a

    def pscrunch_weights(self, planes, weights):
        a, w = np.array(planes, np.float32), np.array(weights, np.float32)
        _ok(self.L.refk_pscrunch_weights(_f(a), _f(w)), "refk_pscrunch_weights")
        return a, w

    def tscrunch(self, planes, npol):
        ave = np.empty(O.scrunch_len(ROWS, npol), np.float32)
        _ok(self.L.refk_tscrunch(_f(_f32(planes)), _f(ave), npol), "refk_tscrunch")
        return ave

    def tscrunch_weights(self, planes, weights, npol):
        ave = np.empty(O.scrunch_len(ROWS, npol), np.float32)
        _ok(self.L.refk_tscrunch_weights(_f(_f32(planes)), _f(ave), _f(_f32(weights)), npol), "refk_tscrunch_weights")
        return ave

    def sel_and_dig(self, ave, npol, nbit):
        ave = _f32(ave).ravel()
        assert ave.size == O.scrunch_len(ROWS, npol)
        out = np.empty(O.trim_bytes(ROWS, npol, nbit), np.uint8)
        _ok(getattr(self.L, "refk_sel_and_dig_%db" % nbit)(_f(ave), _u(out), npol), "refk_sel_and_dig_%db" % nbit)
        return out

    def chain_time(self, udat, rows, rfi_mode=2):
        udat = np.ascontiguousarray(udat, np.uint8)
        assert udat.size == 2 * rows * NFFT
        r = O.SegmentResult()
        nblk = 2 * rows * BLK_PER_ROW
        r.time, r.time_kur = np.empty(udat.size, np.float32), np.empty(udat.size, np.float32)
        r.pow, r.kur, r.dag = (np.empty(nblk, np.float32) for _ in range(3))
        r.pow_fb, r.kur_fb, r.dag_fb, r.weights = (np.empty(2 * rows, np.float32) for _ in range(4))
        _ok(self.L.refk_chain_time(_u(udat), rows, rfi_mode, _f(r.time), _f(r.time_kur), _f(r.pow), _f(r.kur), _f(r.dag),
                                   _f(r.pow_fb), _f(r.kur_fb), _f(r.dag_fb), _f(r.weights)), "refk_chain_time")
        return r

    def chain_detect(self, spec_raw, spec_kur, weights, bp_raw, bp_kur, rfi_mode=2, npol=1, nbit=8, frb_delays=None,
                     inject_now=0):
        """bp_raw / bp_kur: float32 [2*6251], updated in place like oracle.segment's"""
        r = O.SegmentResult()
        sl, tb = O.scrunch_len(ROWS, npol), O.trim_bytes(ROWS, npol, nbit)
        r.ave_raw, r.ave_kur = np.zeros(sl, np.float32), np.zeros(sl, np.float32)
        r.codes_raw, r.codes_kur = np.zeros(tb, np.uint8), np.zeros(tb, np.uint8)
        r.weights = np.zeros(2 * ROWS, np.float32)
        sr = _f32(np.ascontiguousarray(spec_raw).view(np.float32)) if spec_raw is not None else None
        sk = _f32(np.ascontiguousarray(spec_kur).view(np.float32)) if spec_kur is not None else None
        assert bp_raw.dtype == np.float32 and bp_kur.dtype == np.float32
        _ok(self.L.refk_chain_detect(_f(sr), _f(sk), _f(_f32(weights)), _f(bp_raw), _f(bp_kur),
                                     _f(_f32(frb_delays)) if frb_delays is not None else None, inject_now, rfi_mode, npol,
                                     nbit, _f(r.ave_raw), _f(r.ave_kur), _u(r.codes_raw), _u(r.codes_kur), _f(r.weights)),
            "refk_chain_detect")
        return r


# ---------------------------------------------------------------------------------------------------------------------
# orc_* one by one (oracle.py binds these and wraps only the segment driver)

def orc_inject_frb(spec, delays, since, width, amp):
    a = spec_as_f32(spec)
    O.lib().orc_inject_frb(_f(a), _f(_f32(delays)), since, C.c_float(width), C.c_float(amp), ROWS)
    return a


def orc_detect_and_normalize2(spec, bp):
    a, bp = spec_as_f32(spec), np.array(bp, np.float32)
    O.lib().orc_detect_and_normalize2(_f(a), _f(bp), bp_scale(), ROWS)
    return a, bp


def orc_detect_and_normalize3(spec, weights, bp):
    a, bp = spec_as_f32(spec), np.array(bp, np.float32)
    O.lib().orc_detect_and_normalize3(_f(a), _f(_f32(weights)), _f(bp), bp_scale(), ROWS)
    return a, bp


def orc_pscrunch(planes):
    a = np.array(planes, np.float32)
    O.lib().orc_pscrunch(_f(a), ROWS * NCHAN)
    return a


def orc_pscrunch_weights(planes, weights):
    a, w = np.array(planes, np.float32), np.array(weights, np.float32)
    O.lib().orc_pscrunch_weights(_f(a), _f(w), ROWS * NCHAN)
    return a, w


def orc_tscrunch(planes, npol):
    ave = np.empty(O.scrunch_len(ROWS, npol), np.float32)
    O.lib().orc_tscrunch(_f(_f32(planes)), _f(ave), ave.size)
    return ave


def orc_tscrunch_weights(planes, weights, npol):
    ave = np.empty(O.scrunch_len(ROWS, npol), np.float32)
    O.lib().orc_tscrunch_weights(_f(_f32(planes)), _f(ave), _f(_f32(weights)), ave.size)
    return ave


def orc_apply_kurtosis_fake(time):
    """apply_kurtosis_fake (src/pb_kernels.cu:297-318) = apply_kurtosis with no block flagged"""
    time = _f32(time).ravel()
    return O.apply_kurtosis(time, np.zeros(time.size // NKURTO, np.float32))


def orc_chain_detect(spec_raw, spec_kur, weights, bp_raw, bp_kur, npol=1, nbit=8):
    """RFI mode 2's kernels after the FFTs in orc_segment's order (pb_oracle.c), from given spectra and row weights;
    bp_raw / bp_kur updated in place."""
    r = O.SegmentResult()
    d2, bp_raw[:] = orc_detect_and_normalize2(spec_raw, bp_raw)
    d3, bp_kur[:] = orc_detect_and_normalize3(spec_kur, weights, bp_kur)
    w = np.array(weights, np.float32)
    if npol == 1:
        d2 = orc_pscrunch(d2)
        d3, w = orc_pscrunch_weights(d3, w)
    r.ave_raw, r.ave_kur, r.weights = orc_tscrunch(d2, npol), orc_tscrunch_weights(d3, w, npol), w
    r.codes_raw = O.sel_and_dig(r.ave_raw, ROWS, npol, nbit)
    r.codes_kur = O.sel_and_dig(r.ave_kur, ROWS, npol, nbit)
    return r
