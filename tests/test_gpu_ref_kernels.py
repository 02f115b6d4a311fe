"""pb_oracle.c against the reference's OWN kernels, run on the GPU, kernel by kernel.

oracle/_ref/libref_kernels.so is /root/reference/src/pb_kernels.cu compiled as it lies (hipcc, gfx950,
-ffp-contract=off, correctly rounded division and sqrt; oracle/ref_kernels.mk) behind our launch driver, which restates
the grids and buffer sizes of src/process_baseband.cu.  The same seeded array goes into refk_X on the GPU and orc_X on
the CPU; everything is compared bit for bit except compute_dagostino, whose powf the oracle replaces (deviation 1 of
DESIGN.md section 3) -- its tolerance is derived from the device's powf error measured in this test.  A disagreement
here is a misreading in pb_oracle.c, and hence in the HIP kernels that equal it.

What stays unpinned: cuFFT (the chain runs orc_rfft on the host between the two device chains), CUDA's powf, nvcc's own
contraction choices (libref_kernels_fmad.so shows a real compiler's, hipcc's), and the launch sites as the driver
restates them.

Shapes: K1-K5 carry no segment length, so they run at R = 8 rows per pol (block_kurtosis: 2 workgroups) and R = 24;
K7-K11 and the injection fix 1024 rows inside the kernels, so R = 1024 is the smallest shape that exists."""
import numpy as np
import pytest

import oracle as O
import ref_kernels as RK
import synth
from helpers import make_input
from ref_kernels import NCHAN, NFFT, NKURTO, ROWS, same_bits, same_bits_or_both_nan

pytestmark = pytest.mark.gpu

BLK = NFFT // NKURTO
DAG_THRESH = 3.0
CHANMIN = O.CHANMIN


@pytest.fixture(scope="module")
def ref():
    return RK.Ref("strict")


@pytest.fixture(scope="module")
def ref_fmad():
    return RK.Ref("fmad")


def _ulp(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# time domain, K1-K5

def time_bytes(seed, rows):
    """u8 [2][rows*12500]: make_input's noise + RFI bursts + flagged rows + dropped frame, and planted: isolated code 0
    (convertarray's == 0 branch inside a live block), a run of code 128 (voltage exactly 0 by the other branch), and a
    whole 500-sample block of code 0 in pol 0 (0/0 in kurtosis)."""
    u = make_input(seed, rows, 1, rfi=True, dropped=True)[0].copy()
    n = u.shape[1]
    hits = synth.splitmix64(seed + 901, 64) % np.uint64(n)
    u[0, hits[:32].astype(np.int64)] = 0
    u[1, hits[32:].astype(np.int64)] = 0
    u[1, 3 * NKURTO + 17:3 * NKURTO + 217] = 128
    u[0, (BLK + 2) * NKURTO:(BLK + 3) * NKURTO] = 0
    return u


class TimeCase(object):
    def __init__(self, seed, rows):
        self.rows, self.u = rows, time_bytes(seed, rows)
        self.time = O.convertarray(self.u).ravel()
        self.pow, self.kur = O.kurtosis(self.time)
        self.dag = O.compute_dagostino(self.kur)
        self.pow_fb, self.kur_fb = O.block_kurtosis(self.pow, self.kur, self.dag)
        self.dag_fb = O.compute_dagostino(self.kur_fb, which=1)
        self.time_kur, self.weights = O.apply_kurtosis(self.time, self.dag)


@pytest.fixture(scope="module", params=[(21, 8), (22, 24)], ids=["R8", "R24"])
def tcase(request, oracle):
    return TimeCase(*request.param)


def test_convertarray_bit_exact(ref, tcase):
    assert (tcase.u == 0).sum() > NKURTO and (tcase.u == 128).sum() >= 200
    assert same_bits(ref.convertarray(tcase.u).ravel(), tcase.time)


def test_kurtosis_bit_exact(ref, tcase):
    pow_, kur = ref.kurtosis(tcase.time)
    assert np.isnan(tcase.kur).sum() >= 1 and (tcase.pow == 0).sum() >= 1          # the all-zero blocks: 0/0
    assert same_bits(pow_, tcase.pow)
    assert same_bits_or_both_nan(kur, tcase.kur)


def dagostino_check(ref, kur, which, label, capsys):
    """compute_dagostino{,2} of the reference against the oracle's, within a bound DERIVED from the device's powf.

    Every kurtosis value is sent in both pol slots (kur, kur), so that the max over pols is the value's own score.
    The device's powf(t, 1./3) is read back out of the reference's own score: dag = float(|Z1 (Z2 - p)|) with p a float;
    one ulp of p moves the double product by Z1 ulp(p) >= 1.2e-6 against ulp(dag) <= 4.8e-7 (dag < 8), so the p that
    reproduces the score exactly is unique among the neighbours of the float64 value, and the test asserts that one
    does (and exactly one below a score of 8).  k = the largest |p_device - t ** float64(float32(1/3))| in ulps of p;
    the oracle's own cube root is allowed its tested 1 ulp on top:  |dag_ref - dag_orc| <= Z1 (k + 1) ulp(p) + ulp(dag).
    -> (bound per value, oracle score per value), for the flag test."""
    c = O.dag_constants(which)
    kur = np.ascontiguousarray(kur, np.float32).ravel()
    both = np.concatenate([kur, kur])
    d_ref = ref.compute_dagostino(both, which)[:kur.size]
    d_orc = O.compute_dagostino(both, which)[:kur.size]
    k64 = kur.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = ((1 - 2. / c["A"]) / (1. + (k64 - 3. - c["mu1"]) * c["Z3"])).astype(np.float32)
    live = (kur != 0) & (t > 0)                          # NaN kurtosis: t is NaN, t > 0 is false -> DAG_INF
    assert np.all(d_ref[~live] == 9.0) and np.all(d_orc[~live] == 9.0)
    assert live.sum() >= (5 if which else 0.7 * kur.size)
    tl = t[live].astype(np.float64)
    p64 = tl ** np.float64(np.float32(1. / 3))
    p0 = p64.astype(np.float32)
    cands = np.stack([np.nextafter(p0, np.float32(-np.inf)), np.nextafter(np.nextafter(p0, np.float32(-np.inf)), np.float32(-np.inf)),
                      p0, np.nextafter(p0, np.float32(np.inf)), np.nextafter(np.nextafter(p0, np.float32(np.inf)), np.float32(np.inf))])
    score = np.abs(c["Z1"] * (c["Z2"] - cands.astype(np.float64))).astype(np.float32)
    hit = score == d_ref[live][None, :]
    assert np.all(hit.any(axis=0)), "the device's powf is not within 2 ulp of float64, or t differs: %d of %d scores not " \
        "reproduced" % (int((~hit.any(axis=0)).sum()), hit.shape[1])
    # far above the threshold (score > 8: ulp(dag) approaches Z1 ulp(p)) two neighbours can give one score; the nearer
    # one is taken, which can only make k, and with it the bound, smaller
    dist = np.where(hit, np.abs(cands.astype(np.float64) - p64[None, :]), np.inf)
    p_dev = cands[np.argmin(dist, axis=0), np.arange(hit.shape[1])]
    assert np.all(hit.sum(axis=0)[d_ref[live] < 8] == 1)
    k = float(np.max(np.abs(p_dev.astype(np.float64) - p64) / _ulp(p0)))
    p_orc = np.array([O.powf_third(float(x)) for x in t[live]], np.float32)
    k_orc = float(np.max(np.abs(p_orc.astype(np.float64) - p64) / _ulp(p0)))
    assert k_orc <= 1.0                                   # the "+ 1" of the bound
    bound = c["Z1"] * (k + 1) * _ulp(p0) + _ulp(d_orc[live])
    err = np.abs(d_ref[live].astype(np.float64) - d_orc[live].astype(np.float64))
    with capsys.disabled():
        print("\n[ref kernels] %s: %d scores, device powf k = %.3f ulp (oracle's cube root %.3f ulp), Z2_1 = %.2f, "
              "largest |dag_ref - dag_orc| = %.3g, observed / bound = %.3f, %d of %d scores bit-equal"
              % (label, int(live.sum()), k, k_orc, c["Z1"], err.max(), float(np.max(err / bound)),
                 int((d_ref[live] == d_orc[live]).sum()), int(live.sum())))
    assert np.all(err <= bound)
    full = np.zeros(kur.size)
    full[live] = bound
    return full, d_orc


def test_compute_dagostino_within_the_powf_bound_and_flags_equal(ref, tcase, capsys):
    bound, d_one = dagostino_check(ref, tcase.kur, 0, "compute_dagostino R=%d" % tcase.rows, capsys)
    # the reference's layout: pol 0 then pol 1, max over the pols, duplicated
    d_ref = ref.compute_dagostino(tcase.kur)
    n = tcase.kur.size // 2
    assert np.array_equal(d_ref[:n], d_ref[n:]) and same_bits(np.maximum(d_one[:n], d_one[n:]), tcase.dag[:n])
    pair_bound = np.maximum(bound[:n], bound[n:])
    near = np.abs(tcase.dag[:n].astype(np.float64) - DAG_THRESH) <= pair_bound
    # the share of blocks left out of the flag comparison is capped at ZERO: a change of input cannot hide a flag
    assert near.sum() == 0
    assert np.array_equal(d_ref > DAG_THRESH, tcase.dag > DAG_THRESH)
    assert 0 < (tcase.dag[:n] > DAG_THRESH).sum() < n
    with capsys.disabled():
        print("[ref kernels] flags R=%d: %d of %d blocks flagged on both sides; closest oracle score to the threshold "
              "%.3g away = %.0f bounds" % (tcase.rows, int((tcase.dag[:n] > DAG_THRESH).sum()), n,
                                           float(np.min(np.abs(tcase.dag[:n] - DAG_THRESH))),
                                           float(np.min(np.abs(tcase.dag[:n].astype(np.float64) - DAG_THRESH) /
                                                        np.maximum(pair_bound, 1e-30)))))


def test_block_kurtosis_bit_exact(ref, tcase):
    """K4, dead with respect to every output.  Its reduction is warp-synchronous for 32-lane warps; on wave64 a 32-lane
    group lies inside one wave, so the lock-step it relies on holds."""
    pb, kb = ref.block_kurtosis(tcase.pow, tcase.kur, tcase.dag)
    assert same_bits_or_both_nan(pb, tcase.pow_fb)
    assert same_bits_or_both_nan(kb, tcase.kur_fb)
    assert np.isfinite(tcase.kur_fb).sum() >= tcase.rows          # not vacuous


def test_compute_dagostino2_within_the_powf_bound(ref, tcase, capsys):
    bound, d_one = dagostino_check(ref, tcase.kur_fb, 1, "compute_dagostino2 R=%d" % tcase.rows, capsys)
    d_ref = ref.compute_dagostino(tcase.kur_fb, which=1)
    n = tcase.kur_fb.size // 2
    assert np.array_equal(d_ref[:n], d_ref[n:])
    err = np.abs(d_ref[:n].astype(np.float64) - tcase.dag_fb[:n].astype(np.float64))
    assert np.all(err <= np.maximum(bound[:n], bound[n:]))


@pytest.mark.parametrize("inplace", [False, True], ids=["second-buffer", "in-place"])
def test_apply_kurtosis_bit_exact(ref, tcase, inplace):
    """fed the ORACLE's dag; the 25 atomicAdds of one row all add the same constant, so their order cannot matter"""
    out, norms = ref.apply_kurtosis(tcase.time, tcase.dag, inplace=inplace)
    assert same_bits(out, tcase.time_kur)
    assert same_bits(norms, tcase.weights)
    assert len(set(tcase.weights.tolist())) >= 4                    # full, partial and empty rows


def test_apply_kurtosis_fake_bit_exact(ref, tcase):
    out, norms = ref.apply_kurtosis(tcase.time, tcase.dag, fake=True)
    want, wnorms = RK.orc_apply_kurtosis_fake(tcase.time)
    assert same_bits(out, want) and same_bits(out, tcase.time)
    assert same_bits(norms, wnorms)


def test_chain_time_equals_the_kernels_one_by_one(ref, tcase):
    """K1 -> K5 on the device without round trips, in the order of src/process_baseband.cu:1152-1203"""
    r = ref.chain_time(tcase.u, tcase.rows, rfi_mode=2)
    assert same_bits(r.time, tcase.time)
    assert same_bits(r.pow, tcase.pow) and same_bits_or_both_nan(r.kur, tcase.kur)
    assert np.array_equal(r.dag > DAG_THRESH, tcase.dag > DAG_THRESH)
    assert same_bits(r.time_kur, tcase.time_kur) and same_bits(r.weights, tcase.weights)
    r1 = ref.chain_time(tcase.u, tcase.rows, rfi_mode=1)             # fft_in_kur == fft_in
    assert same_bits(r1.time, tcase.time_kur) and same_bits(r1.weights, tcase.weights)


# ---------------------------------------------------------------------------------------------------------------------
# spectral, K7-K11 and the injection: R = 1024

ZERO_ROW, GROUP_LOW = 7, 40                     # a row of exact zeros; an 8-row group whose weight sum is below MIN_WEIGHT


def row_weight(k):
    """k unflagged blocks of a row, as apply_kurtosis accumulates them: k additions of float(500)/12500"""
    w = np.float32(0)
    for _ in range(k):
        w = np.float32(w + np.float32(NKURTO) / np.float32(NFFT))
    return w


def make_spectra(seed):
    """complex64 [2][1024][6251] with full mantissas (a float64 product, rounded once): approximately Gaussian re / im
    under a smooth bandpass, one row of exact zeros, and cells far above 11x the bandpass."""
    n = 2 * ROWS * NCHAN
    w = synth.splitmix64(seed, n)
    re = np.zeros(n, np.int32)
    im = np.zeros(n, np.int32)
    for b in range(4):
        re += ((w >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.int32)
        im += ((w >> np.uint64(32 + 8 * b)) & np.uint64(0xFF)).astype(np.int32)
    gain = (1.0 + 0.5 * np.sin(np.arange(NCHAN) * 0.013)) * 0.0731957
    spec = np.empty((2, ROWS, NCHAN), np.complex64)
    spec.real = (re.reshape(2, ROWS, NCHAN) - 510) * gain
    spec.imag = (im.reshape(2, ROWS, NCHAN) - 510) * (gain * 1.0000123)
    spec[:, ZERO_ROW, :] = 0
    hot = synth.splitmix64(seed + 5, 4000) % np.uint64(n)
    spec.reshape(-1)[hot.astype(np.int64)] *= np.float32(9.3)          # power x 86: clipped by detect_and_normalize3
    spec[:, 300:303, 1000:1040] *= np.float32(5.1)
    return spec


def make_weights(seed):
    """[2048] row weights, equal in both pols as the pipeline produces them (both pols share the flag, DESIGN.md
    section 7): mostly 1, planted 0, 0.16, 0.2, 0.24 (4, 5 and 6 blocks of 25: either side of MIN_WEIGHT), and one
    8-row group with seven weight-0 rows (its sum / 8 is below MIN_WEIGHT).  With equal weights pscrunch_weights' race
    (it rewrites the row weight that other lanes still read, src/pb_kernels.cu:535-536 against :544,550,556) cannot
    change a result: a row of two good pols is rewritten with its own value, a row of two bad ones with 0, still bad.
    Unequal pol weights are therefore not tested."""
    w = np.full(ROWS, row_weight(25), np.float32)
    g = synth.splitmix64(seed, 120) % np.uint64(ROWS)
    for j, k in enumerate((0, 4, 5, 6)):
        w[g[30 * j:30 * j + 30].astype(np.int64)] = row_weight(k)
    w[3], w[4], w[5], w[6] = row_weight(0), row_weight(4), row_weight(5), row_weight(6)
    w[8 * GROUP_LOW:8 * GROUP_LOW + 8] = 0
    w[8 * GROUP_LOW + 2] = row_weight(25)
    return np.concatenate([w, w])


class SpecCase(object):
    """the oracle's side, computed once: each kernel is fed the ORACLE's previous stage"""

    def __init__(self):
        self.spec = make_spectra(31)
        self.w = make_weights(32)
        self.bp0 = np.zeros(2 * NCHAN, np.float32)
        self.d2, self.bp2 = RK.orc_detect_and_normalize2(self.spec, self.bp0)
        self.d3, self.bp3 = RK.orc_detect_and_normalize3(self.spec, self.w, self.bp0)
        self.p2 = RK.orc_pscrunch(self.d2)
        self.p3, self.w3 = RK.orc_pscrunch_weights(self.d3, self.w)
        self._chain = None

    def chain(self):
        """RFI mode 2's kernels after the FFTs, the strict oracle's, on (spec, spec, w) from zero bandpass state"""
        if self._chain is None:
            self._chain = RK.orc_chain_detect(self.spec, self.spec, self.w, self.bp0.copy(), self.bp0.copy(), npol=1, nbit=8)
        return self._chain


@pytest.fixture(scope="module")
def scase(oracle):
    return SpecCase()


@pytest.mark.parametrize("dm", [80.0, 500.0])
def test_set_frb_delays_bit_exact(ref, oracle, dm):
    assert same_bits(ref.set_frb_delays(dm), O.set_frb_delays(dm, ROWS))


@pytest.mark.parametrize("since,width", [(0, 20.48), (1024, 20.48), (5000, 2000.0)], ids=["first", "second", "clips-both-ends"])
def test_inject_frb_bit_exact(ref, scase, since, width):
    delays = O.set_frb_delays(80.0, ROWS)
    lo = (delays.astype(np.float64) + 0.5).astype(np.int64) - since
    hi = (delays.astype(np.float64) + np.float32(width) + 0.5).astype(np.int64) - since
    touched = (lo < ROWS) & (hi >= 0)
    assert 0 < touched.sum() < NCHAN
    if width > ROWS:
        assert ((lo < 0) & (hi >= ROWS)).sum() > 0                   # both ends clipped in one channel
    got = ref.inject_frb(scase.spec, delays, since, width, 1.05)
    want = RK.orc_inject_frb(scase.spec, delays, since, width, 1.05)
    assert not same_bits(want, scase.spec.view(np.float32))
    assert same_bits(got, want)


def test_detect_and_normalize2_bit_exact(ref, scase):
    """bandpass state zero: initialised from the mean; then the state it left, non-zero"""
    got, bp = ref.detect_and_normalize2(scase.spec, scase.bp0)
    assert same_bits(got, scase.d2) and same_bits(bp, scase.bp2)
    assert np.all(scase.d2.reshape(2, ROWS, NCHAN, 2)[:, ZERO_ROW, :, 0] == -1)          # the row of zeros: 0 / bp - 1
    got, bp = ref.detect_and_normalize2(scase.spec, scase.bp2)
    want, wbp = RK.orc_detect_and_normalize2(scase.spec, scase.bp2)
    assert same_bits(got, want) and same_bits(bp, wbp) and not same_bits(wbp, scase.bp2)


def test_detect_and_normalize3_bit_exact(ref, scase):
    got, bp = ref.detect_and_normalize3(scase.spec, scase.w, scase.bp0)
    assert same_bits(got, scase.d3) and same_bits(bp, scase.bp3)
    x = scase.d3.reshape(2, ROWS, NCHAN, 2)[..., 0]
    assert (x == 10).sum() > 1000 and np.all(x[:, 3, :] == 0)                            # clipped cells; a weight-0 row
    got, bp = ref.detect_and_normalize3(scase.spec, scase.w, scase.bp3)                  # non-zero state
    want, wbp = RK.orc_detect_and_normalize3(scase.spec, scase.w, scase.bp3)
    assert same_bits(got, want) and same_bits(bp, wbp)


def test_detect_and_normalize3_all_weight_zero_first_segment(ref, scase):
    """no good sample to initialise from: bp_l = 1 (src/pb_kernels.cu:454-458), every output 0, the state stays 1"""
    w0 = np.zeros(2 * ROWS, np.float32)
    got, bp = ref.detect_and_normalize3(scase.spec, w0, scase.bp0)
    want, wbp = RK.orc_detect_and_normalize3(scase.spec, w0, scase.bp0)
    assert np.all(wbp == 1) and np.all(want.reshape(-1, 2)[:, 0] == 0)
    assert same_bits(got, want) and same_bits(bp, wbp)


def test_pscrunch_bit_exact(ref, scase):
    assert same_bits(ref.pscrunch(scase.d2), scase.p2)


def test_pscrunch_weights_bit_exact(ref, scase):
    got, w = ref.pscrunch_weights(scase.d3, scase.w)
    assert same_bits(got, scase.p3) and same_bits(w, scase.w3)
    assert (scase.w3[:ROWS] != scase.w[:ROWS]).sum() >= 30                               # 0.16 rows rewritten to 0


@pytest.mark.parametrize("npol", [1, 2])
def test_tscrunch_bit_exact(ref, scase, npol):
    src = scase.p2 if npol == 1 else scase.d2
    assert same_bits(ref.tscrunch(src, npol), RK.orc_tscrunch(src, npol))


@pytest.mark.parametrize("npol", [1, 2])
def test_tscrunch_weights_bit_exact(ref, scase, npol):
    src, w = (scase.p3, scase.w3) if npol == 1 else (scase.d3, scase.w)
    want = RK.orc_tscrunch_weights(src, w, npol)
    assert np.all(want.reshape(-1, ROWS // 8, NCHAN)[:, GROUP_LOW, :] == 0)              # weight sum / 8 below MIN_WEIGHT
    assert np.count_nonzero(want.reshape(-1, ROWS // 8, NCHAN)[:, GROUP_LOW + 1, :]) > 0
    assert same_bits(ref.tscrunch_weights(src, w, npol), want)


def quantiser_plane(npol, nbit):
    """fp32 plane [(pol)][128][6251]: seeded values over the quantiser's range, and planted in the kept channels: beyond
    both ends (finite and infinite), the two floats either side of every step edge, and NaN."""
    n = O.scrunch_len(ROWS, npol)
    w = synth.splitmix64(700 + 10 * npol + nbit, n)
    a = ((w >> np.uint64(11)).astype(np.float64) / 2.0 ** 53 * 12.0 - 4.5).astype(np.float32).reshape(-1, ROWS // 8, NCHAN)
    if nbit == 2:
        edges = np.array([-0.6109, 0.3970, 1.4050])
    elif nbit == 4:
        edges = (np.arange(0, 16) - 7.5) * 0.3188
    else:
        edges = (np.arange(0, 256) - 127.5) * 0.02957
    e = edges.astype(np.float32)
    planted = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf)),
                              np.array([-100, 1e6, -1e30, 3e38, np.inf, -np.inf, np.nan, -0.0, 0.0], np.float32)])
    for p in range(a.shape[0]):
        for t in (0, 5, ROWS // 8 - 1):
            a[p, t, CHANMIN + 3:CHANMIN + 3 + planted.size] = planted
            a[p, t, NCHAN - planted.size:] = planted[::-1]
    return a.ravel()


@pytest.mark.parametrize("npol", [1, 2])
@pytest.mark.parametrize("nbit", [8, 4, 2])
def test_sel_and_dig_bit_exact(ref, oracle, nbit, npol):
    ave = quantiser_plane(npol, nbit)
    want = O.sel_and_dig(ave, ROWS, npol, nbit)
    assert len(np.unique(want)) >= (200 if nbit == 8 else 100)
    assert np.array_equal(ref.sel_and_dig(ave, npol, nbit), want)


# ---------------------------------------------------------------------------------------------------------------------
# one chain at R = 1024, RFI mode 2, 8 bits; and the same under a real compiler's contraction

class ChainCase(object):
    def __init__(self):
        self.u = make_input(11, ROWS, 1)[0]
        self.bp_raw, self.bp_kur = np.zeros(2 * NCHAN, np.float32), np.zeros(2 * NCHAN, np.float32)
        self.res = O.segment(self.u, ROWS, self.bp_raw, self.bp_kur, rfi_mode=2, npol=1, nbit=8)


@pytest.fixture(scope="module")
def ccase(oracle):
    return ChainCase()


def run_ref_chain(r, u):
    """refk_chain_time, then orc_rfft on the host (cuFFT does not exist here: deviation 2 of DESIGN.md section 3 stands),
    then refk_chain_detect"""
    t = r.chain_time(u, ROWS, rfi_mode=2)
    spec_raw, spec_kur = O.rfft(t.time), O.rfft(t.time_kur)
    bp_raw, bp_kur = np.zeros(2 * NCHAN, np.float32), np.zeros(2 * NCHAN, np.float32)
    d = r.chain_detect(spec_raw, spec_kur, t.weights, bp_raw, bp_kur, rfi_mode=2, npol=1, nbit=8)
    return t, d, bp_raw, bp_kur


def test_chain_bit_exact(ref, ccase):
    t, d, bp_raw, bp_kur = run_ref_chain(ref, ccase.u)
    o = ccase.res
    assert np.array_equal(t.dag > DAG_THRESH, o.dag > DAG_THRESH) and 0 < (o.dag > DAG_THRESH).sum() < o.dag.size
    assert same_bits(d.weights, o.weights)
    assert same_bits(d.ave_raw, o.ave_raw) and same_bits(d.ave_kur, o.ave_kur)
    assert same_bits(bp_raw, ccase.bp_raw) and same_bits(bp_kur, ccase.bp_kur)
    assert np.array_equal(d.codes_raw, o.codes_raw) and np.array_equal(d.codes_kur, o.codes_kur)
    assert not np.array_equal(o.codes_raw, o.codes_kur)


def _moved(a, b):
    d = a.astype(np.int32) - b.astype(np.int32)
    return int((d != 0).sum()), int(np.abs(d).max())


def test_real_contraction_chain(ref_fmad, ccase, capsys):
    """libref_kernels_fmad.so (-ffp-contract=fast: hipcc's own choice of which a*b + c to fuse) against the STRICT oracle:
    a code moves only by one step, no flag and no row weight moves, and at most 1e-4 of the codes move.  Printed
    beside liboracle_fmad.so's counts (the guess at the fused sites) on the same bytes."""
    t, d, _, _ = run_ref_chain(ref_fmad, ccase.u)
    o = ccase.res
    assert np.array_equal(t.dag > DAG_THRESH, o.dag > DAG_THRESH)
    assert same_bits(d.weights, o.weights)
    try:
        O.set_variant("fmad")
        g = O.segment(ccase.u, ROWS, np.zeros(2 * NCHAN, np.float32), np.zeros(2 * NCHAN, np.float32), rfi_mode=2, npol=1, nbit=8)
    finally:
        O.set_variant("strict")
    rep = []
    for name in ("codes_raw", "codes_kur"):
        n, step = _moved(getattr(d, name), getattr(o, name))
        gn, gstep = _moved(getattr(g, name), getattr(o, name))
        rep += [n, getattr(o, name).size, step, gn, gstep]
        assert step <= 1
        assert n <= 1e-4 * getattr(o, name).size
    with capsys.disabled():
        print("\n[ref kernels] real contraction, chain R=1024 x 1 segment, 8-bit: raw %d/%d codes differ (max %d step; "
              "liboracle_fmad.so: %d, max %d), excised %d/%d (max %d step; liboracle_fmad.so: %d, max %d); flags moved: 0, "
              "row weights moved: 0" % tuple(rep))


def test_real_contraction_spectral(ref_fmad, scase, capsys):
    """the planted spectral case through refk_chain_detect of the contracted library against the strict oracle's kernels
    composed in the same order"""
    want = scase.chain()
    assert same_bits(want.ave_raw, RK.orc_tscrunch(scase.p2, 1)) and same_bits(want.weights, scase.w3)
    got = ref_fmad.chain_detect(scase.spec, scase.spec, scase.w, scase.bp0.copy(), scase.bp0.copy(), rfi_mode=2, npol=1, nbit=8)
    assert same_bits(got.weights, want.weights)
    rep = []
    for name in ("codes_raw", "codes_kur"):
        n, step = _moved(getattr(got, name), getattr(want, name))
        rep += [n, getattr(want, name).size, step]
        assert step <= 1
        assert n <= 1e-4 * getattr(want, name).size
    # the contracted library IS another arithmetic: the raw fp32 plane differs from the strict reading in its last bits
    # (hipcc fuses one a*b + c in detect_and_normalize2).  The excised count is printed and not asserted: this compiler
    # fuses nothing in detect_and_normalize3 and tscrunch_weights, where the oracle's ORC_FMAD guess fuses three sites.
    planes = [int((getattr(got, n).view(np.uint32) != getattr(want, n).view(np.uint32)).sum()) for n in ("ave_raw", "ave_kur")]
    assert planes[0] > 0
    with capsys.disabled():
        print("\n[ref kernels] real contraction, planted spectra R=1024, 8-bit: raw %d/%d codes differ (max %d step), "
              "excised %d/%d (max %d step); row weights moved: 0; fp32 plane values differing in their last bits: "
              "raw %d, excised %d of %d" % tuple(rep + planes + [want.ave_raw.size]))


def test_chain_detect_strict_equals_the_kernels_one_by_one(ref, scase):
    """the device chain of src/process_baseband.cu:1231-1352 on the planted case, strict library: bit-exact"""
    want = scase.chain()
    bp_raw, bp_kur = scase.bp0.copy(), scase.bp0.copy()
    got = ref.chain_detect(scase.spec, scase.spec, scase.w, bp_raw, bp_kur, rfi_mode=2, npol=1, nbit=8)
    assert same_bits(got.ave_raw, want.ave_raw) and same_bits(got.ave_kur, want.ave_kur)
    assert same_bits(bp_raw, scase.bp2) and same_bits(bp_kur, scase.bp3) and same_bits(got.weights, want.weights)
    assert np.array_equal(got.codes_raw, want.codes_raw) and np.array_equal(got.codes_kur, want.codes_kur)
