"""tests/pfb_ref.py, the composed CPU reference of the taps = 4 chain, held to what is known independently of it: the
two composers of tests/test_gpu_pfb.py (pinned to the kernels at their shapes), the float64 restatement of the
reference's polyphase_filterbank, the float64 definition of the window-energy weights, and exact identities between
its own outputs.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import pfb_ref
import test_gpu_pfb as legacy
from helpers import NCHAN, make_input

R = 16
NFFT = 12500


@pytest.fixture(scope="module")
def mode2_input():
    """the input of test_pfb_rfi_mode2_both_streams_bit_exact"""
    data = make_input(62, R, 6)
    for p in range(2):
        seg = data[3, p, 4 * NFFT:8 * NFFT]
        seg[:] = np.where((np.arange(seg.size) // 5) % 2 == 0, 220, 36)
    data.setflags(write=False)
    return data


@pytest.fixture(scope="module")
def mode2_ref(oracle, mode2_input):
    return pfb_ref.pfb_chain(oracle, mode2_input, R, 2, 1, 8)


def test_equals_legacy_mode0_composer(oracle):
    data = make_input(51, R, 4, rfi=False, dropped=False)       # test_pfb_streaming_chain_bit_exact_across_calls
    r = pfb_ref.pfb_chain(oracle, data, R, 0, 1, 8)
    assert np.array_equal(r.codes_raw, legacy._oracle_pfb_chain(oracle, data))
    assert r.codes_kur is None and r.weights is None


def test_equals_legacy_mode2_composer(oracle, mode2_input, mode2_ref):
    raw, kur, w, flags = legacy._oracle_pfb_chain_mode2(oracle, mode2_input, R)
    r = mode2_ref
    assert np.array_equal(r.codes_raw, raw)
    assert np.array_equal(r.codes_kur, kur)
    assert np.array_equal(r.w.view(np.uint32), w.view(np.uint32))
    assert np.array_equal(r.flags, flags)
    expect_w = np.where(w >= np.float32(0.2), w, np.float32(0))           # as that test forms what pb_fetch reports
    assert np.array_equal(r.weights.view(np.uint32), expect_w.view(np.uint32))
    assert (r.codes_kur != r.codes_raw).any()


def test_taps_and_energies_equal_legacy(oracle):
    t = pfb_ref.taps32(oracle)
    assert np.array_equal(t.view(np.uint32), legacy._taps32(oracle).view(np.uint32))
    E, tot = pfb_ref.tap_energy(t)
    assert np.array_equal(E.view(np.uint32), legacy._tap_energy_sequential(t).view(np.uint32))


def test_spectra_match_float64_polyphase_filterbank(oracle):
    """fp32 FIR + the oracle's FFT against the float64 restatement of analysis/baseband.py:polyphase_filterbank
    (oracle.polyphase_filterbank, pinned by tests/golden): output row g is its spectrum g - 3.  Bound: the project's
    2e-6 of the spectrum's peak (test_pfb_taps4_matches_reference_polyphase_filterbank); measured 2.0e-7 / 2.1e-7."""
    nseg = 2
    data = make_input(51, R, nseg, rfi=False, dropped=False)
    r = pfb_ref.pfb_chain(oracle, data, R, 0, 1, 8, keep_spectra=True)
    rows = nseg * R
    for p in range(2):
        volts = oracle.convertarray(np.concatenate([data[s, p] for s in range(nseg)])).astype(np.float64)
        ref = oracle.polyphase_filterbank(volts, nchan=NFFT // 2, nwindow=4)        # rows 0 .. its nspectra - 1
        n = min(ref.shape[0], rows - 3)
        assert n >= 24
        got = r.spec_raw[p][3:3 + n]
        err = np.abs(got - ref[:n]).max() / np.abs(ref[:n]).max()
        print("pol %d: %d spectra, error %.3g of the peak" % (p, n, err))
        assert err < 2e-6, err


def test_weights_match_float64_definition(oracle, mode2_ref):
    """w(g) = sum of the unflagged E / sum of E with E from the float taps in double; absent rows count as flagged.
    Bound: rtol 2e-6, atol 1e-7, what test_pfb_weights_and_excision applies to the kernel."""
    r = mode2_ref
    t = pfb_ref.taps32(oracle).astype(np.float64)
    E = (t.reshape(4, 25, 500) ** 2).sum(axis=2)
    rows = r.flags.shape[0]
    expect = np.zeros(rows)
    for g in range(rows):
        s = 0.0
        for j in range(4):
            rr = g - 3 + j
            if rr >= 0:
                s += E[j][~r.flags[rr]].sum()
        expect[g] = s / E.sum()
    np.testing.assert_allclose(r.w, expect, rtol=2e-6, atol=1e-7)
    clean = np.array([g >= 3 and not r.flags[g - 3:g + 1].any() for g in range(rows)])
    assert clean.any() and np.all(r.w[clean] == 1.0) and r.w[0] < r.w[1] < r.w[2] < 1.0
    assert (r.w == 0).any() and ((r.w > 0) & (r.w < 0.2)).any() and ((r.w >= 0.2) & (r.w < 1)).any()
    # reported weights: npol 1 zeroes what is below MIN_WEIGHT, npol 2 reports the rows' weights themselves
    assert np.array_equal(r.weights, np.where(r.w >= np.float32(0.2), r.w, 0))
    assert np.array_equal(pfb_ref.reported_weights(r.w, 2), r.w)


@pytest.mark.parametrize("rfi_mode", [0, 1, 2])
@pytest.mark.parametrize("npol", [1, 2])
def test_output_sizes_per_format(oracle, mode2_input, rfi_mode, npol):
    """every nbit output has trim_bytes(R, npol, nbit) bytes per segment (the 8-bit codes do not determine the 4- or
    2-bit ones: the quantisers have their own steps), and flags, weights and bandpass state do not depend on nbit"""
    data = mode2_input[:2]
    rs = {nbit: pfb_ref.pfb_chain(oracle, data, R, rfi_mode, npol, nbit) for nbit in (8, 4, 2)}
    for nbit, r in rs.items():
        n = 2 * oracle.trim_bytes(R, npol, nbit)
        assert (r.codes_raw is None) == (rfi_mode == 1) and (r.codes_kur is None) == (rfi_mode == 0)
        for c in (r.codes_raw, r.codes_kur):
            assert c is None or (c.dtype == np.uint8 and c.size == n)
        assert np.array_equal(r.bp_raw.view(np.uint32), rs[8].bp_raw.view(np.uint32))
        assert np.array_equal(r.bp_kur.view(np.uint32), rs[8].bp_kur.view(np.uint32))
        assert np.array_equal(r.w, rs[8].w)
    if rfi_mode == 1:
        assert not rs[8].bp_kur.any() and rs[8].bp_raw.any()         # mode 1 normalises into bp_raw
    if rfi_mode == 0:
        assert not rs[8].bp_kur.any()


@pytest.mark.parametrize("nbit", [8, 4, 2])
def test_two_pol_raw_stream_is_tscrunch_of_the_unsummed_planes(oracle, nbit):
    """npol = 2, RFI mode 0: the codes are orc_tscrunch + sel_and_dig of the two pols' normalised planes, which
    pscrunch never touches -- composed here step by step from the module's FIR"""
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    nseg = 2
    data = make_input(51, R, nseg, rfi=False, dropped=False)
    r = pfb_ref.pfb_chain(oracle, data, R, 0, 2, nbit)
    t = pfb_ref.taps32(oracle)
    start = np.zeros(nseg * R, np.int64)
    spec = [pfb_ref.fir_spectra(oracle, t, oracle.convertarray(np.concatenate([data[s, p] for s in range(nseg)]))
                                .reshape(nseg * R, NFFT), start) for p in range(2)]
    bp = np.zeros(2 * NCHAN, np.float32)
    codes = []
    for s in range(nseg):
        fo = np.ascontiguousarray(np.stack([spec[0][s * R:(s + 1) * R], spec[1][s * R:(s + 1) * R]])).view(np.float32)
        L.orc_detect_and_normalize2(fo.ctypes.data_as(fp), bp.ctypes.data_as(fp), C.c_float(pfb_ref.SCALE), R)
        ave = np.zeros(2 * (R // 8) * NCHAN, np.float32)
        L.orc_tscrunch(fo.ctypes.data_as(fp), ave.ctypes.data_as(fp), ave.size)
        codes.append(oracle.sel_and_dig(ave, R, 2, nbit))
    assert np.array_equal(r.codes_raw, np.concatenate(codes))
    assert np.array_equal(r.bp_raw.view(np.uint32), bp.view(np.uint32))
    # and it is not the one-pol stream in another layout
    assert r.codes_raw.size == 2 * pfb_ref.pfb_chain(oracle, data, R, 0, 1, nbit).codes_raw.size


@pytest.mark.parametrize("rfi_mode,npol,nbit", [(0, 1, 8), (1, 1, 2), (2, 1, 2), (2, 2, 4)])
def test_reset_restarts_the_stream(oracle, mode2_input, rfi_mode, npol, nbit):
    """resets=(k,): the first k segments of the uninterrupted stream, then the stream of data[k:] alone"""
    k = 2
    data = mode2_input[:4]
    whole = pfb_ref.pfb_chain(oracle, data, R, rfi_mode, npol, nbit)
    tail = pfb_ref.pfb_chain(oracle, data[k:], R, rfi_mode, npol, nbit)
    r = pfb_ref.pfb_chain(oracle, data, R, rfi_mode, npol, nbit, resets=(k,))
    for name in ("codes_raw", "codes_kur"):
        a, b, c = getattr(r, name), getattr(whole, name), getattr(tail, name)
        if a is None:
            assert b is None and c is None
            continue
        cut = k * oracle.trim_bytes(R, npol, nbit)
        assert np.array_equal(a[:cut], b[:cut]) and np.array_equal(a[cut:], c)
        assert not np.array_equal(a[cut:], b[cut:])                      # the restart is visible
    if rfi_mode:
        assert np.array_equal(r.weights[:k * R], whole.weights[:k * R])
        assert np.array_equal(r.weights[k * R:], tail.weights)
        assert r.w[k * R] < r.w[k * R + 1] < r.w[k * R + 2] < 1.0 and whole.w[k * R + 2] == 1.0
    assert np.array_equal(r.bp_raw.view(np.uint32), tail.bp_raw.view(np.uint32))
    assert np.array_equal(r.bp_kur.view(np.uint32), tail.bp_kur.view(np.uint32))


def test_injection_follows_orc_segment_since(oracle):
    """the pulse: orc_segment's width and amplitude, since = (inject_now - 1) * R counted from inject_from"""
    data = make_input(41, R, 5, rfi=False, dropped=False)
    delays = oracle.set_frb_delays(80.0, R)
    assert 2 * R < delays[2155] < 3 * R                 # the pulse enters the output band 45 rows after it starts
    plain = pfb_ref.pfb_chain(oracle, data, R, 2, 1, 8)
    inj = pfb_ref.pfb_chain(oracle, data, R, 2, 1, 8, frb_delays=delays, inject_from=1)
    n = 3 * oracle.trim_bytes(R, 1, 8)
    assert np.array_equal(inj.codes_raw[:n], plain.codes_raw[:n])        # nothing in the band before that
    assert not np.array_equal(inj.codes_raw[n:], plain.codes_raw[n:])
    assert not np.array_equal(inj.codes_kur[n:], plain.codes_kur[n:])
    assert pfb_ref.frb_width(R) == np.float32(2e-3 * 10 * (R * 12500 * 10.) / 10 / 12500)
