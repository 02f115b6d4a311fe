"""The seam between the filterbank on the GPU and the search: the code bytes that pb_process / the coadd leave on the
device go into pb_search_* where they lie (codes_on_device = 1, the path production uses), and every output is held to

  * the same search fed the host copy of the same bytes (h.fetch / coadd_finish), bit for bit, and
  * NumPy on that host copy: oracle.search_delays / dedisperse_series / boxcar_best with the level and rms of
    tests/search_stats_ref.py -- never the search itself.

What the two halves each wrote down on their own, and what compares them here:
  * the order of 4- and 2-bit samples within a byte (k_detect2 / k_coadd_digitise against k_transpose_codes): the fp32
    plane is requantised with the reference's sel_and_dig arithmetic restated below, value by value with no packing at
    all, and must equal the search's unpacking of the bytes; the oracle's own sel_and_dig packs the same plane into the
    same bytes;
  * [time][4096] across segments, which end of the band is channel 0, FCH1 / FOFF / TSAMP (tests/test_host_formats.py
    ties them to the SIGPROC header) and the time reference of the injected pulse: the reference's self-test pulse
    (set_frb_delays / inject_frb, src/pb_kernels.cu:338-391) must come out at its own DM and at its own arrival row in
    output channel 0, and must be lost when the channel axis is reversed;
  * one search handle over unequal blocks and bit widths: nothing of an earlier block reaches a later output.

tests/search_rfi_ref.pack / unpack are the search's convention of a packed byte (low bits first; the module that holds
the search tests' packing helpers), used here only as the thing under test."""
import functools
import importlib

import numpy as np
import pytest

import search_stats_ref as SR
from helpers import CHANMIN, NCHAN, NFFT, libpb, make_input
from search_rfi_ref import pack, unpack

pytestmark = pytest.mark.gpu
search = importlib.import_module("vlite-fast_amd.search")

NCO = 4096


def _f32(v):
    return float(np.float32(v))


# the band and the sample time as the C interface carries them (binary32; include/pb_hip.h, pb_search_create)
FCH1, FOFF, TSAMP = _f32(search.FCH1), _f32(search.FOFF), _f32(search.TSAMP)


def requantise(plane, nbit):
    """The reference's sel_and_dig arithmetic (src/pb_kernels.cu:711-735, :672-708, :633-669; the three formulas of
    k_coadd_digitise) on an fp32 plane, one VALUE per sample and no packing: the division and the offset in double,
    rounded to binary32, clipped, truncated (8 and 4 bits); three thresholds compared in double (2 bits)."""
    x = np.asarray(plane, np.float32).astype(np.float64)
    assert np.isfinite(x).all()
    if nbit == 2:
        return ((x >= -0.6109).astype(np.uint8) + (x >= 0.3970) + (x >= 1.4050)).astype(np.uint8)
    step, off, top = (0.02957, 127.5, 255) if nbit == 8 else (0.3188, 7.5, 15)
    tmp = (x / step + off).astype(np.float32)
    return np.where(tmp <= 0, 0, np.where(tmp >= top, top, np.floor(tmp))).astype(np.uint8)


def zap_mask(nchan, zap):
    m = np.zeros(nchan, bool)
    for lo, hi in zap:
        m[lo:hi] = True
    return m


def ref_series(oracle, samples, dms, zap, fch1=FCH1, foff=FOFF, tsamp=TSAMP):
    """samples u8 [T][nchan] -> (series [ndm][tout] exact, tout, delays)"""
    nchan = samples.shape[1]
    delays = oracle.search_delays(dms, fch1, foff, nchan, tsamp)
    series, tout = oracle.dedisperse_series(samples, delays, zap_mask(nchan, zap))
    return series, tout, delays


def ref_planes(oracle, series, nbox, got_stats, W=0):
    """level and rms of the definition (search_stats_ref, exact sums), which the run's statistics `got_stats` must equal
    to the tolerances of tests/test_gpu_search_stats.py (rms 1 binary32 ulp; level 1 ulp + the summation bound), and
    oracle.boxcar_best from the reference's level and rms: the S/N planes [ndm][tout] float64"""
    snr = np.empty(series.shape)
    for i, x in enumerate(series):
        x = x.astype(np.int64)
        level, rms, on_edge = SR.series_stats(x, W)
        assert on_edge == 0                              # no sample on the clip's rounding boundary
        assert abs(float(got_stats[i, 0]) - float(level)) <= SR.level_tolerance(x, W, level), (i, got_stats[i], level)
        assert abs(float(got_stats[i, 1]) - float(rms)) <= float(np.spacing(rms)), (i, got_stats[i], rms)
        snr[i] = oracle.boxcar_best(x, level, rms, nbox)[0] if rms > 0 else 0.0
    return snr


def same_bits(a, b):
    """every array of two Searcher.run results, bit for bit (floats as uint32)"""
    assert a["tout"] == b["tout"]
    for k in ("snr", "stats"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert np.array_equal(a["width_log2"], b["width_log2"])
    assert (a["series"] is None) == (b["series"] is None)
    if a["series"] is not None:
        assert np.array_equal(a["series"], b["series"])


def point_set(pk):
    """a peak list as a sorted list (the arrival order is unspecified), S/N as bits"""
    assert pk["total"] == pk["dmi"].size           # nothing was cut off
    return (pk["tout"], sorted(zip(pk["dmi"].tolist(), pk["t"].tolist(), pk["snr"].view(np.uint32).tolist(),
                                   pk["width_log2"].tolist())))


def peak_of(r):
    """(trial DM index, sample, S/N) of the largest S/N of a run's planes"""
    k = np.unravel_index(np.argmax(r["snr"]), r["snr"].shape)
    return int(k[0]), int(k[1]), float(r["snr"][k])


# ---------------------------------------------------------------------------------------------------------------------
# 1. device path = host path = NumPy, at 8, 4 and 2 bits

R1, S1 = 64, 16                     # 16 segments of 64 rows: 128 time samples x 4096 channels
T1 = R1 * S1 // 8


def _process(h, data, nseg, **kw):
    for s in range(nseg):
        h.submit_planar(0, s, data[s, 0], data[s, 1])
    h.process(nseg, **kw)
    h.sync()


def _check_block(oracle, h, nbit, first, dm_max):
    """The selected set's excised stream from time sample `first` on: device search = host search = NumPy."""
    out = h.fetch(0, 0, S1, ave=True)
    codes_dev, _ = h.output_dev(0, 1)
    host = out["kur"]
    plane = out["ave_kur"].reshape(T1, NCO)
    # the pack-order check.  (a) the reference's own sel_and_dig packs the plane into these very bytes ...
    full = np.zeros((T1, NCHAN), np.float32)
    full[:, CHANMIN:CHANMIN + NCO] = plane
    assert np.array_equal(oracle.sel_and_dig(full, R1 * S1, npol=1, nbit=nbit), host)
    # ... and (b) what the search makes of a byte is the plane requantised value by value, in [time][4096] order
    samples = requantise(plane, nbit)
    assert np.array_equal(unpack(host, T1, NCO, nbit), samples)
    assert samples.max() > samples.min() + 1
    nsamp = T1 - first
    off = first * NCO * nbit // 8
    zap = search.HEIMDALL_ZAP
    with search.Searcher(nchan=NCO, max_samples=T1, dm_min=0, dm_max=dm_max, dm_step=2, boxcar_max=4, zap=zap) as s:
        assert nsamp - s.max_delay >= 64
        rd = s.run(None, nbit=nbit, want_series=True, device_ptr=codes_dev + off, nsamp=nsamp)
        rh = s.run(host[off:], nbit=nbit, want_series=True)
        same_bits(rd, rh)
        pd = s.peaks(None, 1.0, nbit=nbit, device_ptr=codes_dev + off, nsamp=nsamp)
        ph = s.peaks(host[off:], 1.0, nbit=nbit)
        assert pd["total"] > 0 and point_set(pd) == point_set(ph)
        idm, it = np.nonzero(rh["snr"] >= 1.0)              # and the list is the thresholded plane
        assert point_set(ph)[1] == sorted(zip(idm.tolist(), it.tolist(), rh["snr"][idm, it].view(np.uint32).tolist(),
                                              rh["width_log2"][idm, it].tolist()))
        dms, maxd, nbox = s.dms, s.max_delay, s.nbox
    series, tout, delays = ref_series(oracle, samples[first:], dms, zap)
    assert tout == rd["tout"] == nsamp - maxd and maxd == int(delays[-1][~zap_mask(NCO, zap)].max())
    assert np.array_equal(rd["series"], series)
    snr = ref_planes(oracle, series, nbox, rd["stats"])
    np.testing.assert_allclose(rd["snr"], snr, rtol=3e-5, atol=3e-4)
    return host


@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("nbit", [8, 4, 2])
def test_device_codes_equal_host_codes(oracle, nbit, first):
    """pb_process's excised stream searched where it lies.  first = 3: the block starts at an odd time sample of the
    device buffer (byte offset 3 * 4096 * nbit / 8; 125 samples).  DM 0..6 leaves exactly the 64 output samples a block
    must yield (the largest delay of an unzapped channel is 64 samples); the 125-sample block takes DM 0..4."""
    lp = libpb()
    data = make_input(300 + nbit, R1, S1)
    with lp.PbHandle(nbit=nbit, rfi_mode=2, rows_per_seg=R1, max_seg=S1, keep_ave=True) as h:
        _process(h, data, S1)
        _check_block(oracle, h, nbit, first, dm_max=6 if first == 0 else 4)


def test_device_codes_of_set_1_after_set_0_was_reprocessed(oracle):
    """nsets = 2: set 1's device bytes are still set 1's batch after set 0 has been filled and processed again."""
    lp = libpb()
    nbit = 4
    batches = [make_input(310 + i, R1, S1) for i in range(3)]
    with lp.PbHandle(nbit=nbit, rfi_mode=2, rows_per_seg=R1, max_seg=S1, keep_ave=True, nsets=2) as h:
        for i, st in enumerate((0, 1, 0)):
            h.select_set(st)
            _process(h, batches[i], S1)
            if i == 0:
                first0 = h.fetch(0, 0, S1)["kur"].copy()
        set0 = h.fetch(0, 0, S1)["kur"].copy()
        h.select_set(1)
        set1 = _check_block(oracle, h, nbit, 0, dm_max=6)
    assert not np.array_equal(set1, set0) and not np.array_equal(set1, first0) and not np.array_equal(set0, first0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. and 3.  the reference's self-test pulse through the seam

R2, S2 = 1024, 4                    # 4096 rows = 512 time samples
T2 = R2 * S2 // 8
PULSE_DM, PULSE_AMP = 14.0, 1.05
DMS2 = dict(dm_min=0, dm_max=28, dm_step=2)         # 15 trial DMs: not a multiple of the kernel's 4 DMs per workgroup
# The reference chain alone on the bytes of _noise(0), searched by NumPy at these DMs with the production zap and boxcars
# up to 16 -- reference_chain_snr() below is the recipe, it needs no GPU and no test runs it (half a minute on a CPU) --
# gives S/N 32.82 at trial DM 14, sample 64 (30.17 on _noise(1)); with the band reversed 4.00 at trial DM 6.  The
# detection threshold is half of it.  The oracle's pulse amplitude is the reference's 1.05, which is what the test
# sets.
REF_SNR = 32.82
MARGIN = 4                          # samples; the margin of the pulse tests in tests/test_gpu_search.py


@functools.lru_cache(maxsize=None)
def _noise(ant):
    """u8 [S2][2][R2 * 12500]: the seeded genbase-style noise of test_config3_snr_within_one_percent_of_oracle (NumPy
    PCG64, so that the oracle can consume the same bytes); antenna `ant` has its own seed"""
    rng = np.random.default_rng(20261018 + ant)
    n = R2 * NFFT
    out = np.empty((S2, 2, n), np.uint8)
    for s in range(S2):
        out[s] = np.clip(rng.standard_normal((2, n), dtype=np.float32) * np.float32(16.9) + np.float32(128.5),
                         0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def reference_chain_snr(oracle, ant=0, reverse_band=False):
    """How REF_SNR was obtained: helpers.oracle_run on _noise(ant) with rfi_mode=1, frb_delays=set_frb_delays(14, 1024),
    inject_now=1 (so 1 .. 4 over the four segments); the excised stream's codes as [512][4096]; ref_series at DMS2 with
    the production zap; level and rms by search_stats_ref.series_stats; oracle.boxcar_best with 5 widths.
    -> (trial DM, sample, S/N) of the largest S/N.  From the tests directory, with the repository root, oracle/ and
    tests/golden on sys.path as tests/conftest.py puts them: reference_chain_snr(oracle) after oracle.lib()."""
    from helpers import oracle_run
    res, _, _ = oracle_run(oracle, _noise(ant), R2, rfi_mode=1, npol=1, nbit=8,
                           frb_delays=oracle.set_frb_delays(PULSE_DM, R2), inject_now=1)
    samples = np.concatenate([r.codes_kur for r in res]).reshape(T2, NCO)
    if reverse_band:
        samples = np.ascontiguousarray(samples[:, ::-1])
    dms = DMS2["dm_min"] + DMS2["dm_step"] * np.arange(15.0)
    series, _, _ = ref_series(oracle, samples, dms, search.HEIMDALL_ZAP)
    snr = np.empty(series.shape)
    for i, x in enumerate(series):
        level, rms, _ = SR.series_stats(x.astype(np.int64), 0)
        snr[i] = oracle.boxcar_best(x, level, rms, 5)[0]
    k = np.unravel_index(np.argmax(snr), snr.shape)
    return float(dms[k[0]]), int(k[1]), float(snr[k])


def arrival_sample(oracle):
    """the reference's own arrival row of the pulse at output channel 0 (FFT bin 2155), in output samples"""
    return float(oracle.set_frb_delays(PULSE_DM, R2)[CHANMIN]) / 8.0


def _searcher2():
    return search.Searcher(nchan=NCO, max_samples=T2, boxcar_max=16, zap=search.HEIMDALL_ZAP, **DMS2)


def _check_pulse_search(oracle, s, r, samples):
    """a run of _searcher2 against NumPy on the same samples; returns the NumPy planes"""
    series, tout, _ = ref_series(oracle, samples, s.dms, search.HEIMDALL_ZAP)
    assert tout == r["tout"] and np.array_equal(r["series"], series)
    snr = ref_planes(oracle, series, s.nbox, r["stats"])
    np.testing.assert_allclose(r["snr"], snr, rtol=3e-5, atol=3e-4)            # every trial DM
    return snr


def test_injected_pulse_is_found_where_the_reference_puts_it(oracle):
    """One antenna, the reference's self-test pulse at DM 14 (2 ms, amplitude x1.05) injected from the block's first
    row, the excised stream's device bytes searched at DM 0, 2 .. 28.

    Reference S/N (the oracle chain alone on the same bytes, NumPy search, trial DM 14): 32.82 with amp = 1.05, at
    sample 64; the test asks for half of it.  The pulse must peak at trial DM 14 and within 4 samples (the margin of the pulse tests in
    tests/test_gpu_search.py) of set_frb_delays(14, 1024)[2155] / 8 = 63.4, the reference's arrival row in output
    channel 0 in output samples; with the channel axis reversed it must be lost."""
    lp = libpb()
    data = _noise(0)
    with lp.PbHandle(nbit=8, rfi_mode=1, rows_per_seg=R2, max_seg=S2, inject_frb=True, keep_ave=True) as h:
        h.set_frb_params(dm=PULSE_DM, width_rows=-1, amp=PULSE_AMP)
        _process(h, data, S2, inject_now=1)
        host = h.fetch(0, 0, S2, raw=False)["kur"]
        codes_dev, _ = h.output_dev(0, 1)
        with _searcher2() as s:
            assert s.ndm == 15 and s.ndm % 4
            r = s.run(None, want_series=True, device_ptr=codes_dev, nsamp=T2)
            same_bits(r, s.run(host, want_series=True))
            flipped = s.run(np.ascontiguousarray(host.reshape(T2, NCO)[:, ::-1]))
            snr = _check_pulse_search(oracle, s, r, host.reshape(T2, NCO))
            dms = s.dms
    dmi, t, sn = peak_of(r)
    print("pulse: trial DM %g, sample %d, S/N %.2f (NumPy %.2f); reference arrival %.2f, reference S/N %.2f; band "
          "reversed: trial DM %g, S/N %.2f" % (dms[dmi], t, sn, snr.max(), arrival_sample(oracle), REF_SNR,
                                                dms[peak_of(flipped)[0]], peak_of(flipped)[2]))
    assert REF_SNR >= 12 and sn >= 0.5 * REF_SNR
    assert dms[dmi] == PULSE_DM
    assert abs(t - arrival_sample(oracle)) <= MARGIN
    fd, _, fs = peak_of(flipped)
    assert dms[fd] == 0 or fs < 0.5 * sn


def test_coadded_pulse_through_the_same_seam(oracle):
    """Two antennas with independent noise and the same injected pulse: the coadded bytes that pb_coadd_digitise leaves
    on the device, searched there, against pb_coadd_finish's host bytes; the pulse at DM 14, at antenna 0's sample
    (antenna 0 is the block of the single-antenna test) within 1, and S/N(coadd) / mean S/N(single) within
    [0.8, 1.2] sqrt(2), the window test_config3_dm500_pulse_8_antennas uses for 8 antennas.  Two antennas are enough:
    the reference's planes alone (oracle chain on the same bytes, summed, requantised and searched by NumPy) give
    S/N 44.12 against 32.82 and 30.17, a ratio of 0.99 sqrt(2), at DM 14 and sample 64."""
    import torch
    lp = libpb()
    A = 2
    with lp.PbHandle(nant=A, nbit=8, rfi_mode=1, rows_per_seg=R2, max_seg=S2, inject_frb=True, keep_ave=True) as h:
        h.set_frb_params(dm=PULSE_DM, width_rows=-1, amp=PULSE_AMP)
        d_sum = torch.zeros(S2 * h.ave_per_seg, dtype=torch.float32, device="cuda")
        d_codes = torch.zeros(S2 * h.trim, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                       # torch's stream and the library's are different streams
        for a in range(A):
            for sg in range(S2):
                h.submit_planar(a, sg, _noise(a)[sg, 0], _noise(a)[sg, 1])
        h.process(S2, inject_now=1)
        h.coadd_local(S2, d_sum.data_ptr())
        host = h.coadd_finish(S2, d_sum.data_ptr(), A)
        h.coadd_digitise(d_sum.data_ptr(), S2 * h.ave_per_seg, A, d_codes.data_ptr())
        h.sync()
        singles = [h.fetch(a, 0, S2, raw=False)["kur"] for a in range(A)]
        assert np.array_equal(d_codes.cpu().numpy(), host)
        with _searcher2() as s:
            r = s.run(None, want_series=True, device_ptr=d_codes.data_ptr(), nsamp=T2)
            same_bits(r, s.run(host, want_series=True))
            assert point_set(s.peaks(None, 5.0, device_ptr=d_codes.data_ptr(), nsamp=T2)) == point_set(s.peaks(host, 5.0))
            _check_pulse_search(oracle, s, r, host.reshape(T2, NCO))
            one = [peak_of(s.run(c)) for c in singles]
            dms = s.dms
    dmi, t, sn = peak_of(r)
    ratio = sn / np.mean([p[2] for p in one])
    print("coadd: trial DM %g, sample %d, S/N %.2f; single antennas %s; ratio %.3f sqrt(2)"
          % (dms[dmi], t, sn, [(float(dms[p[0]]), p[1], round(p[2], 2)) for p in one], ratio / np.sqrt(2)))
    assert dms[dmi] == PULSE_DM and all(dms[p[0]] == PULSE_DM for p in one)
    assert abs(one[0][1] - arrival_sample(oracle)) <= MARGIN and abs(t - one[0][1]) <= 1
    assert 0.8 * np.sqrt(A) < ratio < 1.2 * np.sqrt(A)


# ---------------------------------------------------------------------------------------------------------------------
# 4. one search handle across unequal blocks

def test_one_search_handle_across_unequal_blocks(oracle):
    """4096 saturated 8-bit samples, then 1500 samples at 2 bits, then 2121 at 8 bits from device memory at an odd
    byte address, through ONE handle: each block's outputs equal a fresh handle's, bit for bit, and the series is
    NumPy's.  The channel-major copy keeps the 255s of the first block past the later blocks' ends, the series and the
    prefix sums keep its values past their tout, and the 2-bit block leaves the high bits of every byte to what the
    unpacking writes."""
    import torch
    nchan, fch1, foff = 96, _f32(361.94), -0.5
    zap = ((40, 47),)
    kw = dict(nchan=nchan, max_samples=4096, fch1=fch1, foff=foff, tsamp=TSAMP, dm_min=0, dm_max=40, dm_step=5,
              boxcar_max=16, zap=zap)
    rng = np.random.default_rng(4100)
    blocks = [(np.full((4096, nchan), 255, np.uint8), 8),
              (rng.integers(0, 4, (1500, nchan)).astype(np.uint8), 2),
              (rng.integers(0, 256, (2121, nchan)).astype(np.uint8), 8)]
    dev = torch.zeros(1 + 2121 * nchan, dtype=torch.uint8, device="cuda")
    dev[1:] = torch.from_numpy(blocks[2][0].ravel()).cuda()
    torch.cuda.synchronize()
    assert (dev.data_ptr() + 1) % 2 == 1
    with search.Searcher(**kw) as s:
        s.set_baseline(512)
        assert s.ndm == 9 and s.max_delay > 500
        for i, (x, nbit) in enumerate(blocks):
            codes = pack(x, nbit)
            where = dict(device_ptr=dev.data_ptr() + 1, nsamp=x.shape[0]) if i == 2 else {}
            r = s.run(None if where else codes, nbit=nbit, want_series=True, **where)
            pk = s.peaks(None if where else codes, 3.0, nbit=nbit, **where)
            with search.Searcher(**kw) as fresh:
                fresh.set_baseline(512)
                same_bits(r, fresh.run(codes, nbit=nbit, want_series=True))
                assert point_set(pk) == point_set(fresh.peaks(codes, 3.0, nbit=nbit))
            series, tout, _ = ref_series(oracle, x, s.dms, zap, fch1, foff, TSAMP)
            assert tout == r["tout"] == x.shape[0] - s.max_delay and np.array_equal(r["series"], series)
            if i == 0:
                assert not r["snr"].any() and pk["total"] == 0           # a constant block: rms 0, S/N 0
            else:
                assert pk["total"] > 0
