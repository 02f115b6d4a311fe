"""The seam between the correlator, the imager and the beamformer on the GPU (pb_correlate, pb_imager_*, pb_beamform) and
the host code that chains them, on a source with fractional delays and per-antenna phases (tests/array_synth.py):
the assertions of tests/test_array_conventions_cpu.py through the library; the beam as the quadratic form of the
correlator's visibilities, GPU against GPU, within the derived bound of DESIGN.md section 12; the imager's PHASE image
closing with the beam; and, bit for bit against tests/beam_ref.py, the instantiations of k_beamform that
tests/test_gpu_beamform.py leaves out: 4, 6 and 7 antennas, 2, 3, 8 and 64 beams, the windows around the length of a
workgroup's run, runs shorter than the rows in flight, and an nout below what fits."""
import importlib

import numpy as np
import pytest

import array_synth as AS
import beam_ref as BR
import correlate_ref as XR
import image_ref as IR
import test_array_conventions_cpu as CV
from helpers import libpb, make_input
from test_gpu_beamform import _beams, _case, _handle, _same, _submit

pytestmark = pytest.mark.gpu

NFFT, NCO = 12500, 4096
F = np.float32
DELAYS, BLS = CV.DELAYS, CV.BLS
loc = importlib.import_module("vlite-fast_amd.localise")


# ---- the chain through the library

@pytest.fixture(scope="module")
def chain(oracle):
    """array_synth's three antennas through a coherence handle, once: the correlator's gate over the 8 rows, the
    beams of CV.ratios, the beam of the closure, and the oracle's spectra of the same bytes for the bounds"""
    lp = libpb()
    R = CV.R
    u8 = AS.phased_antennas(5, R, DELAYS, loc.phase_turns(DELAYS))
    out = dict(gain=np.array([1.0, 0.75, 1.5], F))
    delay, psi = CV.table(DELAYS, "--phase-turns")
    with _handle(lp, 3, R, 1, 0) as h:
        _submit(h, u8[:, None])
        h.process(1)
        out["vis"], out["used"] = h.correlate(0, 1, R)
        out["ratios"] = CV.ratios(lambda d, p, g: h.beamform(0, 1, d, p, g, tscr=R)[0])
        out["beam"] = h.beamform(0, 1, delay, psi, out["gain"][None], tscr=R)[0][0]
    out["X"] = XR.batch_spectra(oracle, u8[:, None], R, 0)[0][0]
    return out


def test_the_tools_beam_adds_the_antennas_coherently(chain):
    CV.check_ratios(chain["ratios"])


def test_imager_sign_fine_delays_and_the_scan(chain):
    lp = libpb()
    u, bls = loc.weighted_vis(chain["vis"], 0, chain["used"])
    assert bls == BLS and np.all(chain["used"] == CV.R)
    coarse = loc.coarse_delays(u)
    with lp.PbImager(3, 101) as im:
        im.set_vis(u)
        r = CV.image_ratios(lambda u, dd, dpsi: im.run(dd, dpsi, mode="phase")[0], lambda u, dd: im.run(dd, mode="delay")[0], u)
        fd = loc.fine_delays(im, coarse)
    CV.check_image_ratios(r)
    CV.check_fine_delays(fd)
    ref = IR.RefImager(3)
    ref.set_vis(u)
    _, ref_scan = ref.run(fd["dd"], per_baseline=True)
    assert fd["scan"].shape == ref_scan.shape
    assert np.array_equal(fd["scan"].view(np.uint32), ref_scan.view(np.uint32))


def test_imager_closure_on_the_gpu(chain):
    """CV.test_imager_and_beamformer_close with every term from the GPU: twice the PHASE image (binary32) of
    u = g_i g_j V_ij, rounded to complex64, against the beam's AA + BB summed over the band less the autos' share.
    Bound: the beam's and the visibilities' (beam_ref.error_bound, both paths, AA and BB over the band), the imager's
    (image_ref.error_bound, twice) and the rounding of u to complex64 (2^-24 |u| per value, twice)."""
    lp = libpb()
    R, gain = CV.R, chain["gain"]
    u, rhs = CV.closure_sides(chain["vis"], chain["beam"], gain)
    u32 = u.astype(np.complex64)
    with lp.PbImager(3, 1) as im:
        im.set_vis(u32)
        lhs = 2.0 * float(im.run(loc.antenna_to_baseline(DELAYS, BLS)[None], loc.baseline_phase(DELAYS, BLS)[None], mode="phase")[0])
    X = chain["X"]
    beam_side = (BR.error_bound(X, gain[None], None, R) + BR.error_bound(X, gain[None], None, R, through="vis"))[0, 0, :2].sum()
    image_side = 2.0 * IR.error_bound(u32, 3) + 2.0 * 2.0 ** -24 * np.abs(u).sum()
    print("2 x PHASE image %.9e  beam less autos %.9e  error / bound = %.4f (bound %.3e: beam and visibilities %.3e, "
          "imager %.3e)" % (lhs, rhs, abs(lhs - rhs) / (beam_side + image_side), beam_side + image_side, beam_side, image_side))
    assert rhs > 0 and abs(lhs - rhs) <= beam_side + image_side


# ---- the beam is the quadratic form of the visibilities

_seam = {}


def _seam_case(oracle, A):
    """helpers.make_input per antenna (RFI bursts, a flagged row, a dropped frame), R = 8, three segments; on top,
    antenna a loses a row of its own (row 5 a + 2 of the 24), so that rows_used differs from baseline to baseline"""
    if A not in _seam:
        R, nseg = 8, 3
        data = np.stack([make_input(500 + 11 * a, R, nseg) for a in range(A)])
        for a in range(A):
            s, row = divmod((5 * a + 2) % (R * nseg), R)
            data[a, s, :, row * NFFT:(row + 1) * NFFT] = np.where((np.arange(NFFT) // 5) % 2 == 0, 220, 36)
        _seam[A] = (data, XR.batch_spectra(oracle, data, R, 2))
    return _seam[A]


@pytest.mark.parametrize("A", [4, 6, 7])
def test_beam_equals_the_quadratic_form_of_the_visibilities(oracle, A):
    """two GPU kernels that share nothing but the spectra: all four products, every gate and channel of five beams
    within the two bounds of beam_ref.error_bound added (the spectra for the bounds are the oracle's, which the
    channeliser equals bit for bit); and rows_used of a beam on antennas i and j alone is the baseline's"""
    lp = libpb()
    R, nseg, tscr = 8, 3, 12
    data, spec = _seam_case(oracle, A)
    delay, psi, gain = BR.five_beams(A, 70 + A)
    bls = XR.baselines(A)
    pair = np.zeros((len(bls), A), F)
    for k, (i, j) in enumerate(bls):
        pair[k, i] = pair[k, j] = 1
    with _handle(lp, A, R, nseg, 2) as h:
        _submit(h, data)
        h.process(nseg)
        got = {}
        for st in (0, 1):
            got[st] = (h.beamform(st, nseg, delay, psi, gain, tscr=tscr), h.correlate(st, nseg, tscr))
        _, pair_used = h.beamform(1, nseg, np.zeros((len(bls), A)), gain=pair, tscr=tscr)
    for st in (0, 1):
        (beams, used), (vis, vused) = got[st]
        assert beams.shape == (5, 2, 4, NCO) and vis.shape == (2, len(bls), 4, NCO)
        form = BR.from_visibilities64(vis, delay, psi, gain)
        X = spec[st][0]
        bound = BR.error_bound(X, gain, None, tscr) + BR.error_bound(X, gain, None, tscr, through="vis")
        live = bound > 0
        err = np.abs(form - beams)
        for q in range(4):
            print("A = %d stream %d product %d: largest error / bound = %.4f (%.2e of the largest value)"
                  % (A, st, q, (err[:, :, q][live[:, :, q]] / bound[:, :, q][live[:, :, q]]).max(),
                     err[:, :, q].max() / np.abs(beams[:, :, q]).max()))
        assert live.any() and np.all(err[live] <= bound[live]) and np.all(err[~live] == 0)
    # the excised stream: each antenna has lost a row of its own
    vused = got[1][1][1]
    assert pair_used.shape == (len(bls), 2, NCO)
    assert len(set(vused[:, k, 0].tobytes() for k in range(len(bls)))) > 2 and vused.min() < tscr
    for k in range(len(bls)):
        assert np.array_equal(pair_used[k], vused[:, k]), bls[k]


# ---- the instantiations that test_gpu_beamform leaves out, bit for bit

def _run(h, X, w, st, nseg, delay, psi, gain, shift, tscr, nout=None, detected=None):
    got = h.beamform(st, nseg, delay, psi, gain, shift, tscr, nout)
    _same(got, BR.beamform(X, w if st else None, delay, psi, gain, shift, tscr, nout, detected=detected))
    if st == 0:
        assert np.all(got[1] == tscr)
    return got


@pytest.mark.parametrize("A", [4, 6, 7])
def test_bit_exact_four_six_and_seven_antennas(oracle, A):
    """U = 4, 3 and 2 rows in flight; R = 16, three segments: more than one run of rows at every tscr below T"""
    lp = libpb()
    corr = importlib.import_module("vlite-fast_amd.correlate")
    R, nseg = 16, 3
    T = R * nseg
    data, spec = _case(oracle, A, R, nseg)
    delay, psi, gain = _beams(A, 10 * A + R)
    random_shift = np.random.default_rng(A).integers(0, 6, NCO).astype(np.int32)
    dm_shift = corr.dm_row0(0.25, 0, T)
    assert dm_shift[0] == 0 and dm_shift.max() >= R - 2 and len(np.unique(dm_shift)) > 5
    variants = {1: (None, None, None), 4: (psi, gain, random_shift), 5: (psi, gain, dm_shift)}
    with _handle(lp, A, R, nseg, 2) as h:
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            X, w = spec[st]
            for nbeam, (ps, ga, sh) in variants.items():
                cut = lambda v: None if v is None else v[:nbeam]
                P = BR.detect(X, delay[:nbeam], cut(ps), cut(ga))
                for tscr in (1, 3, 8, T):
                    _run(h, X, w, st, nseg, delay[:nbeam], cut(ps), cut(ga), None if tscr == T else sh, tscr, detected=P)


@pytest.mark.parametrize("nbeam", [2, 3, 8, 64])
def test_bit_exact_beam_counts(oracle, nbeam):
    """2 and 3: the half-filled and the clamped pair of one tile; 8: two full tiles; 64: the 16 tiles of a run side by
    side in the grid.  Every beam is compared."""
    lp = libpb()
    A, R, nseg = 2, 8, 2
    data, spec = _case(oracle, A, R, nseg)
    rng = np.random.default_rng(900 + nbeam)
    delay = rng.uniform(-20000.0, 20000.0, (nbeam, A))
    psi = rng.uniform(-2.0, 2.0, (nbeam, A))
    gain = rng.uniform(0.5, 1.5, (nbeam, A)).astype(F)
    gain[nbeam - 1, 0] = 0
    shift = rng.integers(0, 5, NCO).astype(np.int32)
    with _handle(lp, A, R, nseg, 2) as h:
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            X, w = spec[st]
            P = BR.detect(X, delay, psi, gain)
            for tscr, sh in ((1, shift), (3, shift), (R * nseg, None)):
                beams, _ = _run(h, X, w, st, nseg, delay, psi, gain, sh, tscr, detected=P)
                assert beams.shape[0] == nbeam


def test_bit_exact_around_the_length_of_a_run(oracle):
    """a workgroup's run is max(1, 32 / tscr) output samples: two at 16, one from 17 on, and from 32 on by the branch
    of its own; T = 80 is a multiple of neither 17 nor 33, and the shifts reach 7 rows"""
    lp = libpb()
    A, R, nseg = 3, 16, 5
    T = R * nseg
    data, spec = _case(oracle, A, R, nseg)
    delay, psi, gain = _beams(A, 33)
    shift = np.random.default_rng(17).integers(0, 8, NCO).astype(np.int32)
    assert shift.max() == 7 and shift.min() == 0
    with _handle(lp, A, R, nseg, 2) as h:
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            X, w = spec[st]
            P = BR.detect(X, delay, psi, gain)
            for tscr in (16, 17, 31, 32, 33, 40):
                beams, _ = _run(h, X, w, st, nseg, delay, psi, gain, shift, tscr, detected=P)
                assert beams.shape[1] == (T - 7) // tscr


def test_bit_exact_runs_shorter_than_the_rows_in_flight(oracle):
    """one antenna holds 16 rows in flight.  tscr = 1, nout = 33: the second run is one row; nout = 1: the only run is;
    tscr = 3, nout = 1: three rows.  The largest shift puts the last window's last row on the batch's last row."""
    lp = libpb()
    A, R, nseg = 1, 8, 5
    T = R * nseg
    data, spec = _case(oracle, A, R, nseg)
    delay, psi, gain = _beams(A, 44)
    rng = np.random.default_rng(3)
    with _handle(lp, A, R, nseg, 2) as h:
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            X, w = spec[st]
            P = BR.detect(X, delay, psi, gain)
            for tscr, nout in ((1, 33), (1, 1), (3, 1)):
                top = T - nout * tscr
                shift = rng.integers(0, top + 1, NCO).astype(np.int32)
                shift[[0, 77, 4095]] = top, 0, top
                beams, used = _run(h, X, w, st, nseg, delay, psi, gain, shift, tscr, nout, detected=P)
                assert beams.shape == (5, nout, 4, NCO) and used.shape == (5, nout, NCO)


def test_an_nout_below_what_fits(oracle):
    lp = libpb()
    A, R, nseg, tscr = 5, 8, 3, 3
    data, spec = _case(oracle, A, R, nseg)
    delay, psi, gain = _beams(A, 55)
    shift = np.random.default_rng(5).integers(0, 4, NCO).astype(np.int32)
    with _handle(lp, A, R, nseg, 2) as h:
        _submit(h, data)
        h.process(nseg)
        for st in (0, 1):
            X, w = spec[st]
            P = BR.detect(X, delay, psi, gain)
            full = _run(h, X, w, st, nseg, delay, psi, gain, shift, tscr, detected=P)
            assert full[0].shape[1] == (R * nseg - 3) // tscr == 7
            for nout in (5, 1):
                part = _run(h, X, w, st, nseg, delay, psi, gain, shift, tscr, nout, detected=P)
                assert part[0].shape == (5, nout, 4, NCO) and part[1].shape == (5, nout, NCO)
                assert part[0].tobytes() == full[0][:, :nout].tobytes() and np.array_equal(part[1], full[1][:, :nout])
