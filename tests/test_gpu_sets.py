"""What selecting a buffer set guarantees (pb_select_set through the Python binding): every set keeps its own device
buffers, its own coadd target and its own count of processed segments, and none of them is disturbed by visiting the
other sets.  The smallest handle with three sets; one small batch."""
import numpy as np
import pytest

from helpers import libpb, make_input

pytestmark = pytest.mark.gpu

R, NSEG, NSETS = 16, 2, 3
KUR = 1     # rfi_mode 2: the excised stream is the one a coadd target replaces


def _handle(lp):
    return lp.PbHandle(device=0, nant=1, nbit=8, npol=1, rfi_mode=2, rows_per_seg=R, max_seg=NSEG, nsets=NSETS,
                       keep_ave=True)


def _pointers(h):
    return (h.input_dev(0)[0],) + h.output_dev(0, 0) + h.output_dev(0, 1)


def test_every_set_has_its_own_buffers_and_keeps_them():
    lp = libpb()
    with _handle(lp) as h:
        first = []
        for i in range(NSETS):
            h.select_set(i)
            first.append(_pointers(h))
        for k in range(len(first[0])):            # input, codes and fp32 plane of either stream
            assert all(p[k] for p in first)
            assert len({p[k] for p in first}) == NSETS
        for i in range(NSETS):
            for j in range(NSETS):
                h.select_set(i)
                h.select_set(j)
                assert _pointers(h) == first[j]
                h.select_set(i)
                assert _pointers(h) == first[i]
        with pytest.raises(ValueError):
            h.select_set(NSETS)
        assert _pointers(h) == first[NSETS - 1]   # (a refused select leaves the selection alone)


def test_coadd_target_belongs_to_the_set_it_was_given_to():
    import torch
    lp = libpb()
    with _handle(lp) as h:
        tgt = torch.zeros(NSEG * h.ave_per_seg, dtype=torch.float32, device=torch.device("cuda", 0))
        own = []
        for i in range(NSETS):
            h.select_set(i)
            own.append(h.output_dev(0, KUR)[1])
        assert tgt.data_ptr() not in own

        def planes():
            out = []
            for i in range(NSETS):
                h.select_set(i)
                out.append(h.output_dev(0, KUR)[1])
            return out

        h.select_set(1)
        h.set_coadd_target(tgt.data_ptr())
        assert h.output_dev(0, KUR)[1] == tgt.data_ptr()
        assert h.output_dev(0, 0)[1] != tgt.data_ptr()           # the raw stream keeps its plane
        for _ in range(2):                                       # before and after further selects
            assert planes() == [own[0], tgt.data_ptr(), own[2]]
        h.select_set(2)
        h.select_set(1)
        h.set_coadd_target(0)
        assert h.output_dev(0, KUR)[1] == own[1]
        assert planes() == own


def test_processed_segments_are_counted_per_set():
    import torch
    lp = libpb()
    data = make_input(5, R, NSEG)
    with _handle(lp) as h:
        d_sum = torch.zeros(NSEG * h.ave_per_seg, dtype=torch.float32, device=torch.device("cuda", 0))
        h.select_set(0)
        for s in range(NSEG):
            h.submit_planar(0, s, data[s, 0], data[s, 1])
        h.process(NSEG)
        out = h.fetch(0, 0, NSEG)
        assert out["raw"].any() and out["kur"].any()
        h.coadd_local_codes(NSEG, d_sum.data_ptr())
        for other in (1, 2):
            h.select_set(other)
            with pytest.raises(ValueError, match="more segments than the batch holds"):
                h.coadd_local_codes(NSEG, d_sum.data_ptr())
        h.select_set(0)
        h.coadd_local_codes(NSEG, d_sum.data_ptr())
        again = h.fetch(0, 0, NSEG)
        assert np.array_equal(again["raw"], out["raw"])
        assert np.array_equal(again["kur"], out["kur"])
        h.sync()
