"""What a handle owns and when it lets go of it (csrc/pb_own.h, csrc/pb_handle.hip): pb_query's device_bytes over the
allocation paths of pb_create, of the VDIF staging (first use, regrowth) and of the coadd slots; pb_destroy with work
still queued on every stream; and the members that are made on first use, released once.  The smallest legal segment
throughout (8 rows, two segments): every allocation path still runs."""
import ctypes as C
import itertools

import numpy as np
import pytest

from helpers import libpb, make_input

pytestmark = pytest.mark.gpu

R, S = 8, 2
FRAMES_PER_SEG = R * 12500 // 5000       # per thread


def _cases():
    """(nant, nsets, taps, hipfft, rfi_mode, extra): the matrix, then each of the three options once"""
    out = []
    for nant, nsets, (taps, hipfft), rfi in itertools.product((1, 2), (1, 3), ((1, False), (4, False), (1, True)), (0, 1, 2)):
        out.append((nant, nsets, taps, hipfft, rfi, ""))
    return out + [(1, 1, 1, False, 2, "keep_ave"), (1, 1, 1, False, 2, "debug_keep"), (1, 1, 1, False, 2, "coherence")]


def _name(c):
    return "a%d-s%d-t%d-%s-r%d%s" % (c[0], c[1], c[2], "hipfft" if c[3] else "lds", c[4], "-" + c[5] if c[5] else "")


# device_bytes (after pb_create, after the first pb_submit_vdif of one segment, after one of two segments, after the
# first pb_coadd_finish) as the library gave them on an MI355X BEFORE the handle's buffers became owning members: read
# with measure() below from the library built at the commit before that change, in the same visit to the GPU as the
# first run of this test.  A coherence handle refuses the incoherent sum, so its last figure repeats the third.
EXPECTED = {
    "a1-s1-t1-lds-r0": (1544376, 1745656, 1946936, 1963320),
    "a1-s1-t1-lds-r1": (1544376, 1745656, 1946936, 1963320),
    "a1-s1-t1-lds-r2": (2068664, 2269944, 2471224, 2487608),
    "a1-s1-t4-lds-r0": (1695080, 1896360, 2097640, 2114024),
    "a1-s1-t4-lds-r1": (1695080, 1896360, 2097640, 2114024),
    "a1-s1-t4-lds-r2": (2219368, 2420648, 2621928, 2638312),
    "a1-s1-t1-hipfft-r0": (4744632, 4945912, 5147192, 5163576),
    "a1-s1-t1-hipfft-r1": (4744632, 4945912, 5147192, 5163576),
    "a1-s1-t1-hipfft-r2": (8469176, 8670456, 8871736, 8888120),
    "a1-s3-t1-lds-r0": (3426904, 3628184, 3829464, 3845848),
    "a1-s3-t1-lds-r1": (3426904, 3628184, 3829464, 3845848),
    "a1-s3-t1-lds-r2": (4999768, 5201048, 5402328, 5418712),
    "a1-s3-t4-lds-r0": (3577608, 3778888, 3980168, 3996552),
    "a1-s3-t4-lds-r1": (3577608, 3778888, 3980168, 3996552),
    "a1-s3-t4-lds-r2": (5150472, 5351752, 5553032, 5569416),
    "a1-s3-t1-hipfft-r0": (13027672, 13228952, 13430232, 13446616),
    "a1-s3-t1-hipfft-r1": (13027672, 13228952, 13430232, 13446616),
    "a1-s3-t1-hipfft-r2": (24201304, 24402584, 24603864, 24620248),
    "a2-s1-t1-lds-r0": (2551112, 2752392, 2953672, 2970056),
    "a2-s1-t1-lds-r1": (2551112, 2752392, 2953672, 2970056),
    "a2-s1-t1-lds-r2": (3599688, 3800968, 4002248, 4018632),
    "a2-s1-t4-lds-r0": (2852116, 3053396, 3254676, 3271060),
    "a2-s1-t4-lds-r1": (2852116, 3053396, 3254676, 3271060),
    "a2-s1-t4-lds-r2": (3900692, 4101972, 4303252, 4319636),
    "a2-s1-t1-hipfft-r0": (8951624, 9152904, 9354184, 9370568),
    "a2-s1-t1-hipfft-r1": (8951624, 9152904, 9354184, 9370568),
    "a2-s1-t1-hipfft-r2": (16400712, 16601992, 16803272, 16819656),
    "a2-s3-t1-lds-r0": (6316040, 6517320, 6718600, 6734984),
    "a2-s3-t1-lds-r1": (6316040, 6517320, 6718600, 6734984),
    "a2-s3-t1-lds-r2": (9461768, 9663048, 9864328, 9880712),
    "a2-s3-t4-lds-r0": (6617044, 6818324, 7019604, 7035988),
    "a2-s3-t4-lds-r1": (6617044, 6818324, 7019604, 7035988),
    "a2-s3-t4-lds-r2": (9762772, 9964052, 10165332, 10181716),
    "a2-s3-t1-hipfft-r0": (25517576, 25718856, 25920136, 25936520),
    "a2-s3-t1-hipfft-r1": (25517576, 25718856, 25920136, 25936520),
    "a2-s3-t1-hipfft-r2": (47864840, 48066120, 48267400, 48283784),
    "a1-s1-t1-lds-r2-keep_ave": (2134200, 2335480, 2536760, 2553144),
    "a1-s1-t1-lds-r2-debug_keep": (2078584, 2279864, 2481144, 2497528),
    "a1-s1-t1-lds-r2-coherence": (3166392, 3367672, 3568952, 3568952),
}


def _device_bytes(lp, h):
    s = lp.PbSizes()
    h._chk(h._L.pb_query(h._h, C.byref(s)))
    return int(s.device_bytes)


def _vdif_block(nseg, seed=3):
    vdif = __import__("importlib").import_module("vlite-fast_amd.vdif")
    d = make_input(seed, R, nseg, rfi=False, dropped=False)
    return vdif.frame_block(d[:, 0].ravel(), d[:, 1].ravel(), 3600, 33, 7)


def measure(lp, case):
    import torch
    nant, nsets, taps, hipfft, rfi, extra = case
    coh = extra == "coherence"
    with lp.PbHandle(nant=nant, nbit=8, npol=2 if coh else 1, rfi_mode=rfi, taps=taps, nsets=nsets,
                     fft_backend=lp.FFT_HIPFFT if hipfft else lp.FFT_LDS, rows_per_seg=R, max_seg=S,
                     keep_ave=extra == "keep_ave", debug_keep=extra == "debug_keep", coherence=coh) as h:
        seen = [_device_bytes(lp, h)]
        blocks = [_vdif_block(1), _vdif_block(2)]
        assert blocks[0].size == 2 * FRAMES_PER_SEG * 5032 and blocks[1].size == 2 * blocks[0].size
        for blk in blocks:
            h.submit_vdif(0, 0, blk)
            seen.append(_device_bytes(lp, h))
        if not coh:
            d_sum = torch.zeros(S * h.ave_per_seg, dtype=torch.float32, device=torch.device("cuda", 0))
            h.coadd_finish(1, d_sum.data_ptr(), 1)
        seen.append(_device_bytes(lp, h))
        h.sync()
        assert h._L.pb_last_error(h._h) == b""
    return tuple(seen)


@pytest.mark.parametrize("case", _cases(), ids=_name)
def test_device_bytes_are_what_they_were(case):
    assert measure(libpb(), case) == EXPECTED[_name(case)]


def _handle(lp, taps, nsets=3):
    return lp.PbHandle(nant=1, nbit=8, npol=1, rfi_mode=2, taps=taps, nsets=nsets, rows_per_seg=R, max_seg=S)


def _batch(h, data, fetch=True):
    for s in range(S):
        h.submit_planar(0, s, data[s, 0], data[s, 1])
    h.process(S)
    return h.fetch(0, 0, S) if fetch else None


@pytest.mark.parametrize("taps", [1, 4])
def test_destroy_with_work_queued(taps):
    """two batches processed and never fetched, a third one staged and never processed, then close(): the next handle
    of the same configuration starts where a fresh one does"""
    lp = libpb()
    data = [make_input(40 + k, R, S) for k in range(3)]
    with _handle(lp, taps) as ref:
        want = []
        for k in range(3):
            ref.select_set(k)
            want.append(_batch(ref, data[k]))
    assert want[0]["raw"].any() and want[0]["kur"].any() and not np.array_equal(want[0]["raw"], want[1]["raw"])
    h = _handle(lp, taps)
    for k in range(2):
        h.select_set(k)
        _batch(h, data[k], fetch=False)
    h.select_set(2)
    for s in range(S):
        h.submit_planar(0, s, data[2][s, 0], data[2][s, 1])
    assert h._L.pb_last_error(h._h) == b""
    h.close()
    with _handle(lp, taps) as h2:
        got = _batch(h2, data[0])
        assert h2._L.pb_last_error(h2._h) == b""
    assert np.array_equal(got["raw"], want[0]["raw"]) and np.array_equal(got["kur"], want[0]["kur"])


def _vdif_and_coadd_round(lp):
    """a handle that stages VDIF, sums its batch and requantises the sum, once each: what those made on first use"""
    import torch
    with lp.PbHandle(nant=1, nbit=8, npol=1, rfi_mode=2, rows_per_seg=R, max_seg=S, keep_ave=True) as h:
        h.submit_vdif(0, 0, _vdif_block(S, seed=8))
        h.process(S)
        out = h.fetch(0, 0, S)
        d_sum = torch.zeros(S * h.ave_per_seg, dtype=torch.float32, device=torch.device("cuda", 0))
        h.coadd_local(S, d_sum.data_ptr())
        codes = h.coadd_finish(S, d_sum.data_ptr(), 1)
        view = h.coadd_view(S).copy()
        assert h._L.pb_last_error(h._h) == b""
    return out["raw"], out["kur"], codes, view


def _array_round(lp):
    """a coherence handle whose correlator, beamformer and beam planes each made their state"""
    data = np.stack([make_input(700 + a, R, S) for a in range(2)])
    with lp.PbHandle(nant=2, nbit=8, npol=2, rfi_mode=2, rows_per_seg=R, max_seg=S, coherence=True) as h:
        for a in range(2):
            for s in range(S):
                h.submit_planar(a, s, data[a, s, 0], data[a, s, 1])
        h.process(S)
        delay = np.array([[0.0, 3.5]])
        vis, used = h.correlate(1, S, 8)
        beams, _ = h.beamform(1, S, delay, tscr=4)
        planes, _, level = h.beam_planes(1, S, delay, tscr=4)
        assert h._L.pb_last_error(h._h) == b""
    return vis, used, beams, planes, level


def test_members_made_on_first_use_are_released_once():
    lp = libpb()
    first = _vdif_and_coadd_round(lp)
    again = _vdif_and_coadd_round(lp)
    assert first[0].any() and first[1].any() and first[2].any()
    assert np.array_equal(first[2], first[3])
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    a1 = _array_round(lp)
    a2 = _array_round(lp)
    for x, y in zip(a1, a2):
        assert x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
