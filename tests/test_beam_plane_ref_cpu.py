"""The restatement of pb_beam_planes' definition (tests/beam_plane_ref.py) on synthetic blocks, without a GPU: a noise
block gives zero-mean, unit-variance planes; the chunked binary64 sum is the loop it says it is; samples without rows and
channels without a level give +0.0f; a level handed in replaces the planes' own."""
import numpy as np

import beam_plane_ref as PR

F = np.float32


def _noise_block(seed, nbeam, nout, nchan, tscr):
    """[nbeam][nout][4][nchan]: AA and BB of unit-variance complex Gaussian voltages added over tscr rows (CR, CI: junk that
    must not matter), so AA + BB has mean 4 tscr and std / mean = 1 / sqrt(2 tscr)"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (nbeam, nout, 2, tscr, 2, nchan)).astype(F)        # pol, row, (re, im)
    out = np.empty((nbeam, nout, 4, nchan), F)
    out[:, :, :2] = (v * v).sum(axis=(3, 4))
    out[:, :, 2:] = np.nan
    return out


def test_noise_planes_are_zero_mean_unit_variance():
    """With k = 4 tscr degrees of freedom per value the normalised value has variance 1 and excess kurtosis 12 / k: over N
    independent values the mean's standard error is 1 / sqrt(N), the variance's sqrt((2 + 12 / k) / N).  With the true
    level handed in both hold exactly; with the planes' own level every channel's mean is taken out, which lowers the
    variance by 1 / nout -- here 1 / 2048, a twelfth of the standard error."""
    nbeam, nout, nchan, tscr = 2, 2048, 16, 8
    beams = _noise_block(1, nbeam, nout, nchan, tscr)
    used = np.full((nbeam, nout, nchan), tscr, np.int32)
    N, k = nbeam * nout * nchan, 4 * tscr
    se_mean, se_var = 1 / np.sqrt(N), np.sqrt((2 + 12 / k) / N)
    true = np.full((nbeam, nchan), 4 * tscr, F)
    for level_in in (true, None):
        p, L = PR.planes(beams, used, tscr, level_in)
        m, v = p.astype(np.float64).mean(), p.astype(np.float64).var()
        print("level_in %s: mean %.5f (se %.5f)  var %.5f (se %.5f)" % (level_in is not None, m, se_mean, v, se_var))
        assert abs(m) < 3 * se_mean and abs(v - 1) < 3 * se_var
        assert np.all(np.abs(L / (4 * tscr) - 1) < 5 / np.sqrt(2 * tscr * nout))


def test_chunked_sum_is_the_loop():
    rng = np.random.default_rng(2)
    nbeam, nout, nchan, tscr = 2, 71, 3, 3                       # two whole chunks and a short one
    beams = (rng.uniform(0.5, 2.0, (nbeam, nout, 4, nchan)) * 10.0 ** rng.integers(-3, 4, (nbeam, nout, 1, nchan))).astype(F)
    used = rng.integers(0, tscr + 1, (nbeam, nout, nchan)).astype(np.int32)
    used[0, :, 1] = 0                                            # a column without a row
    _, L = PR.planes(beams, used, tscr)
    for b in range(nbeam):
        for c in range(nchan):
            total, n = 0.0, 0
            for s0 in range(0, nout, 32):
                chunk = 0.0
                for s in range(s0, min(s0 + 32, nout)):
                    if used[b, s, c] > 0:
                        J = F(F(beams[b, s, 0, c] + beams[b, s, 1, c]) * F(F(tscr) / F(used[b, s, c])))
                        chunk = chunk + float(J)
                        n += 1
                total = total + chunk
            want = F(total / float(n)) if n else F(0)
            assert L[b, c].view(np.uint32) == want.view(np.uint32), (b, c)
    assert L[0, 1] == 0
    # the order matters at these dynamic ranges: a plain binary32 mean differs somewhere
    J = PR.power(beams, used, tscr)
    assert np.any(np.where(used > 0, J, 0).sum(axis=1, dtype=F) / np.maximum((used > 0).sum(axis=1), 1).astype(F) != L)


def test_no_rows_and_no_level_give_plus_zero():
    rng = np.random.default_rng(3)
    nbeam, nout, nchan, tscr = 1, 40, 4, 4
    beams = rng.uniform(1, 2, (nbeam, nout, 4, nchan)).astype(F)
    used = np.full((nbeam, nout, nchan), tscr, np.int32)
    used[0, 5, 0] = 0
    used[0, :, 1] = 0                                            # L = 0 in channel 1
    beams[0, :, :2, 2] = 0                                       # L = 0 from zero power in channel 2
    p, L = PR.planes(beams, used, tscr)
    zero = np.zeros(1, F).view(np.uint32)[0]
    assert p[0, 5, 0].view(np.uint32) == zero and L[0, 0] > 0
    assert L[0, 1] == 0 and L[0, 2] == 0
    assert np.all(p[0, :, 1:3].view(np.uint32) == zero)
    assert np.all(np.isfinite(p)) and np.any(p[0, :, 3] != 0)
    lev = L.copy()
    lev[0, 3] = 0                                                # a level of 0 handed in
    p2, L2 = PR.planes(beams, used, tscr, lev)
    assert np.all(p2[0, :, 3].view(np.uint32) == zero) and np.array_equal(L2, L)
    # used below tscr scales the power up to a full window
    used[0, 7, 0] = 1
    assert PR.power(beams, used, tscr)[0, 7, 0] == F(beams[0, 7, 0, 0] + beams[0, 7, 1, 0]) * F(4)


def test_level_in_overrides_the_own_level():
    rng = np.random.default_rng(4)
    nbeam, nout, nchan, tscr = 2, 33, 5, 8
    beams = rng.uniform(20, 40, (nbeam, nout, 4, nchan)).astype(F)
    used = np.full((nbeam, nout, nchan), tscr, np.int32)
    own, L = PR.planes(beams, used, tscr)
    lev = (L * F(2)).astype(F)
    p, L2 = PR.planes(beams, used, tscr, lev)
    assert np.array_equal(L2, L)                                 # level_out is the planes' own level either way
    I = beams[:, :, 0] + beams[:, :, 1]
    want = (I / lev[:, None] - F(1)) * np.sqrt(F(16))
    assert np.array_equal(p.view(np.uint32), want.astype(F).view(np.uint32))
    assert not np.array_equal(p, own)
