"""Host side of the localisation (vlite-fast_amd/localise.py) without a GPU: the fine-delay scan on the binary64 model,
the geometry, the TDOA rms map against the reference's expressions, and the tool's argument and file errors."""
import importlib

import numpy as np
import pytest

import image_ref as IR

loc = importlib.import_module("vlite-fast_amd.localise")
VLA = np.array([-1601185.4, -5041977.5, 3554875.9])


def test_fine_delays_recover_the_antennas_delays():
    """0.1 sample = 5 sigma of the expected 12500 / (2 pi 90 1182) = 0.019 (S/N 0.5 sqrt(32768), rms bin spread
    4096 / sqrt(12)); 0.031 was the largest error seen when the issue was written"""
    gate_vis, used = IR.delayed_gate(5, 8, (0, 58, 131))
    u, bls = loc.weighted_vis(gate_vis, 0, used)
    assert bls == [(0, 1), (0, 2), (1, 2)] and u.shape == (3, 2, 4096) and u.dtype == np.complex64
    coarse = loc.coarse_delays(u)
    assert np.abs(coarse - [58, 131, 73]).max() <= 12500 / 4096.0
    im = IR.RefImager(3, exact=False)
    im.set_vis(u)
    fd = loc.fine_delays(im, coarse)
    assert fd["x"].shape == (101,) and fd["x"][0] == -5.0 and fd["x"][-1] == 5.0
    dev = np.abs(fd["samples"] - [58, 131, 73])
    print("largest deviation of a baseline's delay: %.4f samples" % dev.max())
    assert dev.max() <= 0.1
    assert np.abs(fd["fit_samples"] - [0, 58, 131]).max() <= 0.1
    assert (fd["err"] > 0).all() and np.isfinite(fd["err"]).all() and (fd["peak"] > 1500).all()


def test_weighted_vis_subtracts_off_gates_and_normalises_by_their_autos():
    rng = np.random.default_rng(2)
    gv = (rng.standard_normal((3, 3, 4, 4096)) + 1j * rng.standard_normal((3, 3, 4, 4096)))
    gv[:, 0] = np.abs(gv[:, 0]) + 1.0                 # autos (0, 0) and (1, 1): positive
    gv[:, 2] = np.abs(gv[:, 2]) + 1.0
    used = np.full((3, 3, 4096), 7)
    used[1, 1, 100:110] = 0
    gv[0, 0, 0, 5] = gv[2, 0, 0, 5] = 0.0             # an auto that is not positive
    mask = np.ones(4096, bool)
    mask[2000:2100] = False
    u, bls = loc.weighted_vis(gv, 1, used, mask)
    assert bls == [(0, 1)]
    off = (gv[0] + gv[2]) / 2
    for s, prod in enumerate((0, 3)):
        with np.errstate(divide="ignore", invalid="ignore"):
            want = (gv[1, 1, prod] - off[1, prod]) / np.sqrt(off[0, prod].real * off[2, prod].real)
        ok = mask.copy()
        ok[100:110] = False
        if prod == 0:
            ok[5] = False
        assert np.allclose(u[0, s][ok], want[ok].astype(np.complex64), rtol=1e-6)
        assert not u[0, s][~ok].any()
    with pytest.raises(ValueError):
        loc.weighted_vis(gv, 3, used)
    with pytest.raises(ValueError):
        loc.weighted_vis(gv[:, :2], 0, used[:, :2])


def test_antenna_to_baseline_and_phases():
    d = np.array([[0.0, 2.0, 5.5], [1.0, 1.0, -3.0]])
    bls = [(0, 1), (0, 2), (1, 2)]
    assert np.array_equal(loc.antenna_to_baseline(d, bls), [[2.0, 5.5, 3.5], [0.0, -4.0, -4.0]])
    assert np.array_equal(loc.phase_turns(d), -3.0 * d)
    assert np.array_equal(loc.baseline_phase(d, bls), 3.0 * loc.antenna_to_baseline(d, bls))


def test_precession_matrix():
    assert np.array_equal(loc.precession_matrix(0.0), np.eye(3))
    for T in (0.2, -0.5, 1.0):
        P = loc.precession_matrix(T)
        assert np.abs(P @ P.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(P) - 1) < 1e-14
    pole = loc.precession_matrix(0.2) @ np.array([0.0, 0.0, 1.0])
    dec_arcsec = np.degrees(np.arctan2(pole[2], np.hypot(pole[0], pole[1]))) * 3600
    assert abs((90 * 3600 - dec_arcsec) - 400.8448) < 0.01


def test_gmst_and_the_delay_towards_the_zenith():
    unix = 946728000.0                                 # J2000.0: T = 0, no precession
    assert abs(loc.gmst_rad(unix) * 12 / np.pi - 18.697374558) < 1e-9
    assert abs(loc.gmst_rad(unix + 86164.0905) - loc.gmst_rad(unix)) < 1e-5            # one sidereal day
    r = np.linalg.norm(VLA)
    ra_z = loc.gmst_rad(unix) + np.arctan2(VLA[1], VLA[0])
    dec_z = np.arcsin(VLA[2] / r)
    d0 = loc.antenna_delays(VLA[None], loc.source_vector(ra_z, dec_z, unix))[0]
    assert abs(d0 - (-r / 299792458.0 * 128e6)) < 1e-6 * abs(d0)
    rng = np.random.default_rng(4)
    ra, dec = rng.uniform(0, 2 * np.pi, 2000), np.arcsin(rng.uniform(-1, 1, 2000))
    d = loc.antenna_delays(VLA[None], loc.source_vector(ra, dec, unix))[:, 0]
    assert d.shape == (2000,) and (d >= d0).all()
    near = loc.antenna_delays(VLA[None], loc.source_vector(ra_z + 1e-3, dec_z - 1e-3, unix))[0]
    assert near > d0
    # a clock delay adds its samples
    dc = loc.antenna_delays(VLA[None], loc.source_vector(ra_z, dec_z, unix), clock_ns=[100.0])[0]
    assert abs(dc - d0 - 12.8) < 1e-9


def test_sky_grid_is_gnomonic_about_its_centre():
    ra0, dec0 = np.radians(83.6), np.radians(22.0)
    ra, dec = loc.sky_grid(ra0, dec0, 30.0, 21)
    assert ra.shape == dec.shape == (441,)
    c = 10 * 21 + 10
    assert abs(ra[c] - ra0) < 1e-12 and abs(dec[c] - dec0) < 1e-12
    hw = np.radians(0.5)
    # the row through the centre runs east, the column north; tangent-plane offsets are exact
    assert abs(np.tan(dec[20 * 21 + 10] - dec0) - hw) < 1e-12 and abs(ra[20 * 21 + 10] - ra0) < 1e-12
    assert ra[c + 10] > ra0 and abs(np.tan(ra[c + 10] - ra0) * np.cos(dec0) - hw) < 1e-12
    one = loc.sky_grid(ra0, dec0, 30.0, 1)
    assert abs(one[0][0] - ra0) < 1e-12 and abs(one[1][0] - dec0) < 1e-12


def test_tdoa_rms_map_equals_the_reference_expressions():
    rng = np.random.default_rng(7)
    nbl = 28
    measured = rng.standard_normal(nbl) * 1e-7
    clock = rng.standard_normal(nbl) * 1e-8
    tau_hp = rng.standard_normal((500, nbl)) * 1e-6
    tau_zoom = rng.standard_normal((11, 13, nbl)) * 1e-6
    mask = rng.uniform(size=nbl) > 0.3
    # analysis/loc_step3.py:317-348
    total_delays_ns = measured.copy() * 1e9
    total_delays_ns += clock * 1e9
    chi_hp = total_delays_ns[None, :] + tau_hp * 1e9
    chi_zoom = total_delays_ns[None, None, :] + tau_zoom * 1e9
    rms_hp = (chi_hp[:, mask] ** 2).mean(axis=1) ** 0.5
    rms_zoom = (chi_zoom[:, :, mask] ** 2).mean(axis=-1) ** 0.5
    assert np.array_equal(loc.tdoa_rms_map(measured, clock, tau_hp, mask), rms_hp)
    assert np.array_equal(loc.tdoa_rms_map(measured, clock, tau_zoom, mask), rms_zoom)


def test_parser_refusals(capsys):
    ok = ["--vis", "a.npz", "-o", "b.npz"]
    a = loc.parse_args(ok + ["--scan-only", "--zap", "0", "100", "--zap", "4000", "4096"])
    assert a.scan_only and a.zap == [[0, 100], [4000, 4096]] and a.mode == "delay" and a.npix == 201
    a = loc.parse_args(ok + ["--antennas", "x.txt", "--centre", "83.6", "22", "--time", "1.7e9", "--mode", "phase",
                             "--clock-ns", "1", "2", "--npix", "21", "--half-width", "30"])
    assert a.centre == [83.6, 22.0] and a.clock_ns == [1.0, 2.0] and a.mode == "phase"
    for bad in (ok,                                                        # a position needs antennas, centre and time
                ok + ["--antennas", "x.txt", "--centre", "1", "2"],
                ok + ["--antennas", "x.txt", "--centre", "1", "91", "--time", "5"],
                ok + ["--antennas", "x.txt", "--centre", "1", "2", "--time", "5", "--npix", "0"],
                ok + ["--antennas", "x.txt", "--centre", "1", "2", "--time", "5", "--half-width", "0"],
                ok + ["--scan-only", "--zap", "5", "5"], ok + ["--scan-only", "--zap", "-1", "5"],
                ok + ["--scan-only", "--zap", "5", "4097"], ok + ["--scan-only", "--zap", "5"],
                ok + ["--scan-only", "--mode", "both"], ok + ["--scan-only", "--npix"],
                ["--vis", "a.npz"], ["-o", "b.npz"]):
        with pytest.raises(SystemExit):
            loc.parse_args(bad)
    capsys.readouterr()


def test_antenna_file_errors(tmp_path):
    p = tmp_path / "ants.txt"
    p.write_text("# the array\nea01 1.0 2.0 3.0\n\nea02 -4 5e3 6  # east arm\n")
    names, xyz = loc.read_antennas(str(p), 2)
    assert names == ["ea01", "ea02"] and np.array_equal(xyz, [[1, 2, 3], [-4, 5000, 6]])
    with pytest.raises(ValueError, match="2 antennas, the visibilities have 3"):
        loc.read_antennas(str(p), 3)
    p.write_text("ea01 1.0 2.0\n")
    with pytest.raises(ValueError, match=":1: expected `name X Y Z`"):
        loc.read_antennas(str(p), 1)
    p.write_text("ea01 1.0 2.0 3.0\nea02 1.0 north 3.0\n")
    with pytest.raises(ValueError, match=":2: X Y Z must be numbers"):
        loc.read_antennas(str(p), 2)
    with pytest.raises(IOError):
        loc.read_antennas(str(tmp_path / "none.txt"), 1)


def test_load_gates_takes_either_form_of_the_correlators_file(tmp_path):
    gv = np.zeros((3, 3, 4, 4096), np.complex64)
    used = np.ones((3, 3, 4096), np.int32)
    np.savez(tmp_path / "g.npz", gate_vis=gv, gate_on=np.int64(1), gate_rows_used=used, vis=gv[0], rows_used=used[0])
    g = loc.load_gates(str(tmp_path / "g.npz"))
    assert g[0].shape == gv.shape and g[1] == 1 and g[2].shape == used.shape
    np.savez(tmp_path / "v.npz", vis=gv[0], rows_used=used[0])
    g = loc.load_gates(str(tmp_path / "v.npz"))
    assert g[0].shape == (1, 3, 4, 4096) and g[1] == 0 and g[2].shape == (1, 3, 4096)
    np.savez(tmp_path / "n.npz", other=used)
    with pytest.raises(ValueError, match="neither gate_vis nor vis"):
        loc.load_gates(str(tmp_path / "n.npz"))
