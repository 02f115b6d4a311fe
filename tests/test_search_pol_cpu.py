"""The NumPy restatement of the polarisation stage (tests/search_pol_ref.py) pinned to answers worked out by hand, and the
command line's refusals around -pol, which come before the library is loaded.  No GPU."""
import importlib

import numpy as np
import pytest

import search_pol_ref as R

search = importlib.import_module("vlite-fast_amd.search")
sigproc = importlib.import_module("vlite-fast_amd.sigproc")

NCHAN, FCH1, FOFF, TSAMP = 96, 384.0, -0.5, 781.25e-6
ZAP = ((0, 3), (90, 96))
DMS = np.arange(0.0, 61.0, 2.0)
DELAY = R.delays(DMS, FCH1, FOFF, NCHAN, TSAMP)
ZAPPED = R.zap_mask(NCHAN, ZAP)
LAM2 = R.lambda2(FCH1, FOFF, NCHAN)


def test_geometry_of_the_tests():
    assert DELAY[15].max() == 327 and DELAY.shape == (31, NCHAN)            # DM 30: the largest delay is 327 samples
    assert abs((LAM2[-1] - LAM2[0]) - 0.19) < 0.01
    assert LAM2[0] == (299.792458 / 384.0) ** 2


def test_i_code_rule():
    assert R.icode([0, 0, 255, 255], [0, 1, 254, 255]).tolist() == [0, 1, 255, 255]
    a, b = np.meshgrid(np.arange(256), np.arange(256))
    assert np.array_equal(R.icode(a, b), np.floor((a + b) / 2.0 + 0.5).astype(np.uint8))
    blk = np.arange(2 * 4 * 3, dtype=np.uint8).reshape(2, 4, 3)
    p4, xt = R.planes(blk)
    assert p4.shape == (4, 3, 2) and p4[2, 1, 1] == blk[1, 2, 1] and np.array_equal(xt, R.icode(p4[0], p4[1]))


def test_constant_planes_give_nothing():
    p4 = np.stack([np.full((NCHAN, 1200), v, np.uint8) for v in (100, 140, 90, 201)])
    r = R.pol(p4, DELAY, ZAPPED, LAM2, [(15, 400, 8), (0, 0, 1)], 64, 8, -50.0, 1.0, 101)
    assert np.all(r["q"][:, ~ZAPPED] == 0) and np.all(r["u"][:, ~ZAPPED] == 0) and np.all(r["F"] == 0)
    assert np.all(r["summary"][:, 2:5] == 0) and np.all(r["summary"][:, 0] == 87) and r["kbest"].tolist() == [0, 0]
    assert np.all(r["on"][0][:, ~ZAPPED] == np.array([100, 140, 90, 201])[:, None] * 8) and np.all(r["on"][:, :, ZAPPED] == 0)


def test_window_clipping_counts():
    """nsamp 1000, L 64, g 8, DM 30 (index 15): channel 3 has delay 8 there, channel 89 -- the last unzapped one -- 302."""
    p4 = np.ones((4, NCHAN, 1000), np.uint8)
    assert DELAY[15, 3] == 8 and DELAY[15, 89] == 302 and np.all(DELAY[0] == 0)
    # at the block's start: t_pk 0, w 7 -> on [0, 7); off [-72, -8) and [15, 79)
    on, non, off, noff = R.spectra(p4, DELAY, ZAPPED, 15, 0, 7, 64, 8)
    assert non[3] == 7 and noff[3] == 64                 # [8, 15); [-64, 0) lies before the block, [23, 87) inside
    assert non[89] == 7 and noff[89] == 128              # [302, 309); [230, 294) and [317, 381) both inside
    assert np.array_equal(on[:, 3], [7] * 4) and np.array_equal(off[:, 89], [128] * 4)
    # t_pk 40: the early window [-32, 32) + 8 = [-24, 40) keeps 40 samples
    assert R.spectra(p4, DELAY, ZAPPED, 15, 40, 7, 64, 8)[3][3] == 40 + 64
    # at DM 0 nothing is delayed: t_pk 0 keeps the late window only, in every channel
    assert np.all(R.spectra(p4, DELAY, ZAPPED, 0, 0, 1, 64, 0)[3][~ZAPPED] == 64)
    # near the block's end: t_pk 672, w 64 -> on [672, 736), off [600, 664) and [744, 808)
    on, non, off, noff = R.spectra(p4, DELAY, ZAPPED, 15, 672, 64, 64, 8)
    assert non[3] == 64 and noff[3] == 128
    assert non[89] == 26 and noff[89] == 64              # [974, 1038) cut at 1000; [902, 966) inside, [1046, 1110) past the end
    assert np.array_equal(on[:, 89], [26] * 4)
    assert np.all(non[ZAPPED] == 0) and np.all(noff[ZAPPED] == 0)
    # a channel without an on sample, or without an off sample, has weight 0
    i, q, u, v, w = R.stokes(on, np.where(np.arange(NCHAN) == 10, 0, non), off, np.where(np.arange(NCHAN) == 11, 0, noff), ZAPPED)
    assert not w[10] and not w[11] and w[12] and w.sum() == 85 and np.isnan(q[10])


def _screen(rm, chi0, p, rm_lo, rm_step, nrm):
    psi2 = 2.0 * (rm * LAM2 + chi0)
    w = ~ZAPPED
    q, u = np.where(w, p * np.cos(psi2), np.nan), np.where(w, p * np.sin(psi2), np.nan)
    i = np.where(w, 1.0, np.nan)
    F, kbest, summary, theta = R.rm_synth(i, q, u, 0.0 * i, w, LAM2, rm_lo, rm_step, nrm)
    return F, kbest, summary, theta, psi2


def test_noiseless_faraday_screen():
    """q + i u = p exp(2 i (RM lambda^2 + chi0)) with RM on the grid: at that trial every term is p exp(2 i (RM lambda0^2 +
    chi0)) up to rounding, so |F| = p and arg F / 2 = RM lambda0^2 + chi0 mod pi.  Tolerance, relative to p: the screen's
    phase 2 psi is rounded (|2 psi| 2^-53 from the product and the sum, twice), so is theta (|theta| 2^-53), the four
    sines and cosines are good to an ulp or two, each product and sum adds 2^-53, and the n terms are accumulated with at
    most n 2^-53: eps = (max|2 psi| + max|theta| + 16) 2^-52 + n 2^-53, ~5e-14 here."""
    rm, chi0, p = 37.0, 0.4, 0.8
    F, kbest, summary, theta, psi2 = _screen(rm, chi0, p, -200.0, 1.0, 401)
    n = int((~ZAPPED).sum())
    eps = (np.abs(psi2).max() + np.abs(theta[kbest]).max() + 16) * 2.0 ** -52 + n * 2.0 ** -53
    assert eps < 1e-13
    assert kbest == 237 and summary[5] == rm and summary[0] == n
    assert abs(summary[4] - p) <= eps * p
    l0 = summary[1]
    assert abs(l0 - LAM2[~ZAPPED].mean()) < 1e-15
    ang = 0.5 * np.arctan2(F[kbest, 1], F[kbest, 0])
    d = (ang - (rm * l0 + chi0) + np.pi / 2) % np.pi - np.pi / 2
    assert abs(d) <= eps + (rm * l0 + chi0) * 2.0 ** -52                     # (the comparison's own rounding)
    # every other trial has lost coherence: the next trials by a little, the far ones to the RMSF's sidelobes
    mag = np.hypot(F[:, 0], F[:, 1])
    assert mag[236] < p and mag[238] < p and mag[:200].max() < 0.3 * p
    # an RM between two trials peaks at one of its neighbours
    assert _screen(37.4, chi0, p, -200.0, 1.0, 401)[1] == 237 and _screen(37.6, chi0, p, -200.0, 1.0, 401)[1] == 238


def _pulse_planes(aa, bb, cr, ci):
    """planes of 100 everywhere with an excess over [400, 408) dedispersed at DM 30"""
    p4 = np.full((4, NCHAN, 1200), 100, np.uint8)
    for c in range(NCHAN):
        d = int(DELAY[15, c])
        for k, e in enumerate((aa, bb, cr, ci)):
            p4[k, c, 400 + d:408 + d] = 100 + e
    return p4


def test_swapped_hands_and_negated_ci():
    req, kw = [(15, 400, 8)], dict(L=64, g=8, rm_lo=-5.0, rm_step=1.0, nrm=11)
    a = R.pol(_pulse_planes(40, 10, 0, 20), DELAY, ZAPPED, LAM2, req, **kw)
    b = R.pol(_pulse_planes(10, 40, 0, -20), DELAY, ZAPPED, LAM2, req, **kw)
    assert np.all(a["q"][0, ~ZAPPED] == 30.0) and np.all(a["u"][0, ~ZAPPED] == 0.0) and a["kbest"][0] == 5 == b["kbest"][0]
    assert a["summary"][0, 2] == 50.0 and a["summary"][0, 4] == 30.0
    ang = lambda r: 0.5 * np.arctan2(r["F"][0, 5, 1], r["F"][0, 5, 0])
    assert ang(a) == 0.0 and abs(ang(b)) == np.pi / 2                        # swapping AA and BB turns the angle by pi/2
    assert abs(a["summary"][0, 3] - R.SQRT2 * 20.0) < 1e-13 and a["summary"][0, 3] == -b["summary"][0, 3]       # negating the CI excursion negates v
    c = R.pol(_pulse_planes(25, 25, 30, 0), DELAY, ZAPPED, LAM2, req, **kw)  # pure U: 45 degrees
    assert abs(0.5 * np.arctan2(c["F"][0, 5, 1], c["F"][0, 5, 0]) - np.pi / 4) < 1e-15
    assert abs(c["summary"][0, 4] - R.SQRT2 * 30.0) < 1e-13


def test_no_weight_gives_nan_and_minus_one():
    p4 = _pulse_planes(40, 10, 5, 5)
    r = R.pol(p4, DELAY, np.ones(NCHAN, bool), LAM2, [(15, 400, 8)], 64, 8, -5.0, 1.0, 11)
    assert r["kbest"][0] == -1 and np.all(np.isnan(r["F"])) and r["summary"][0, 0] == 0 and np.all(np.isnan(r["summary"][0, 1:]))
    assert np.all(r["on"] == 0) and np.all(r["noff"] == 0)


def test_simulated_pulse_recovers_its_rm_and_angle():
    """the fixture of tests/test_gpu_search_pol.py's RM test: the restatement alone finds RM 37 with a margin, and the
    position angle at lambda0 within 0.05 rad of RM lambda0^2 + chi0"""
    blk = R.simulate(*R.RM_FIXTURE[0], NCHAN, FCH1, FOFF, DELAY[15], [R.RM_FIXTURE[1]])
    p4, _ = R.planes(blk)
    r = R.pol(p4, DELAY, ZAPPED, LAM2, [(15, 700, 8)], 64, 8, -200.0, 1.0, 401)
    p = (r["F"][0] ** 2).sum(axis=1)
    best2 = np.sort(p)[-2:]
    print("kbest", r["kbest"][0], "relative gap of the best two", (best2[1] - best2[0]) / best2[1], "summary", r["summary"][0])
    assert r["kbest"][0] == 237 and (best2[1] - best2[0]) / best2[1] > 5e-3          # 8.3e-3 here
    l0 = r["summary"][0, 1]
    ang = 0.5 * np.arctan2(r["F"][0, 237, 1], r["F"][0, 237, 0])
    d = (ang - (37.0 * l0 + 0.4) + np.pi / 2) % np.pi - np.pi / 2
    print("angle off by", d, "L/I", r["summary"][0, 4] / r["summary"][0, 2])
    assert abs(d) < 0.05
    assert 0.6 < r["summary"][0, 4] / r["summary"][0, 2] < 1.0               # p = 0.8, plus the noise's bias


def _fil(path, nifs, nbits=8, nsamp=8):
    hdr = b"".join([sigproc.send_string("HEADER_START"), sigproc.send_int("data_type", 1), sigproc.send_double("fch1", FCH1),
                    sigproc.send_double("foff", FOFF), sigproc.send_int("nchans", NCHAN), sigproc.send_int("nbits", nbits),
                    sigproc.send_double("tstart", 57570.0), sigproc.send_double("tsamp", TSAMP), sigproc.send_int("nifs", nifs),
                    sigproc.send_string("HEADER_END")])
    path.write_bytes(hdr + bytes(nsamp * nifs * NCHAN * nbits // 8))
    return str(path)


def test_cli_refusals_come_before_the_library(tmp_path, monkeypatch):
    libpb = importlib.import_module("vlite-fast_amd.libpb")

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(libpb, "load", boom)
    one, four, four4 = _fil(tmp_path / "one.fil", 1), _fil(tmp_path / "four.fil", 4), _fil(tmp_path / "four4.fil", 4, nbits=4)
    with pytest.raises(SystemExit, match="nifs 4"):
        search.main(["-f", one, "-pol"])                                     # a 1-IF file with -pol
    with pytest.raises(SystemExit, match="nifs 4"):
        search.main(["-f", four4, "-pol"])                                   # a 4-bit one
    with pytest.raises(SystemExit, match="single-IF"):
        search.main(["-f", four])                                            # today's refusal stays
    with pytest.raises(SystemExit, match="single-IF"):
        search.main(["-f", four, "-stream_chunk", "4"])
    with pytest.raises(SystemExit):
        search.main(["-f", four, "-pol", "-stream_chunk", "4"])
    for bad in (["-rm", "10", "-10"], ["-rm_step", "0"], ["-rm", "-9000", "9000", "-rm_step", "1"], ["-pol_max", "0"],
                ["-pol_off", "0", "8"], ["-pol_off", "64", "2000"]):
        with pytest.raises(SystemExit):
            search.parse_args(["-f", four, "-pol"] + bad)
    with pytest.raises(SystemExit):
        search.parse_flags("-pol")                                           # not a flag of process_baseband --search
    a = search.parse_args(["-f", four, "-pol", "-detect_thresh", "7"])
    assert a.pol_thresh == 7.0 and a.pol_max == 32 and a.rm == [-2000.0, 2000.0] and a.rm_step == 2.0 and a.pol_off == [64, 8]
    assert search.rm_trials(-2000.0, 2000.0, 2.0) == 2001


def test_pol_line_and_numbers():
    F = np.zeros((3, 2))
    F[1] = (0.0, 2.0)
    p = dict(kbest=np.int32(1), summary=np.array([87.0, 0.7, 4.0, -1.0, 2.0, 36.0]), F=F)
    assert search.pol_numbers(p) == (36.0, 0.5, -0.25, 45.0)
    c = dict(snr=9.5, peak_idx=700, peak_time=0.546875, tfilt=3, dmi=15, dm=30.0, ngiant=4, i0=698, i1=710, pol=p)
    cols = search.pol_line(c).split("\t")
    assert cols[:-4] == search.candidate_line(c).split("\t") and [float(x) for x in cols[-4:]] == [36.0, 0.5, -0.25, 45.0]
    assert all(np.isnan(x) for x in search.pol_numbers(dict(kbest=-1, summary=np.full(6, np.nan), F=F)))
