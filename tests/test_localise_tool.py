"""python -m vlite-fast_amd.localise as a child process on the GPU: a noiseless point source on a 21 x 21 grid comes back
at its pixel and position, and --scan-only returns the delays of the delayed-antenna visibilities."""
import os
import subprocess
import sys

import numpy as np
import pytest

import correlate_ref as XR
import image_ref as IR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(out, *args):
    cmd = [sys.executable, "-m", "vlite-fast_amd.localise", "-o", out] + [str(a) for a in args]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return np.load(out)


def test_tool_finds_the_point_source(tmp_path):
    ps = IR.point_source()
    nant, n = len(ps["xyz"]), ps["n"]
    all_bls = XR.baselines(nant)
    vis = np.zeros((len(all_bls), 4, IR.NCHANOUT), np.complex64)
    cross = dict((b, k) for k, b in enumerate(ps["bls"]))
    for k, (i, j) in enumerate(all_bls):
        if i == j:
            vis[k] = 1.0
        else:
            vis[k, 0] = ps["u"][cross[(i, j)], 0]
            vis[k, 3] = ps["u"][cross[(i, j)], 1]
    np.savez(tmp_path / "out.npz", vis=vis, rows_used=np.ones((len(all_bls), IR.NCHANOUT), np.int64))
    with open(tmp_path / "ants.txt", "w") as f:
        f.write("# name X Y Z (m)\n")
        for a, r in enumerate(ps["xyz"]):
            f.write("ea%02d %.6f %.6f %.6f\n" % (a, r[0], r[1], r[2]))
    z = _tool(str(tmp_path / "loc.npz"), "--vis", tmp_path / "out.npz", "--antennas", tmp_path / "ants.txt", "--centre",
              repr(float(np.degrees(ps["ra0"]))), repr(float(np.degrees(ps["dec0"]))), "--time", repr(ps["unix"]),
              "--half-width", 30, "--npix", n)
    ra, dec = ps["grid"]
    assert z["image"].shape == (n, n) and z["tdoa_rms_ns"].shape == (n, n)
    assert z["peak_pixel"].tolist() == [ps["ipix"] // n, ps["ipix"] % n]
    assert abs(float(z["peak_ra_deg"]) - np.degrees(ra[ps["ipix"]])) < 1e-9
    assert abs(float(z["peak_dec_deg"]) - np.degrees(dec[ps["ipix"]])) < 1e-9
    assert np.allclose(z["grid_ra_deg"].ravel(), np.degrees(ra), atol=1e-9)
    assert z["image"].max() > 0.99 * 2 * len(ps["bls"]) * IR.NCHANOUT
    # the fine delays are the source's, so the TDOA map has its minimum there too and nothing is left at the peak
    assert np.abs(z["fine_samples"] - ps["dd"][ps["ipix"]]).max() < 0.01
    assert int(np.argmin(z["tdoa_rms_ns"])) == ps["ipix"]
    assert np.abs(z["residual_samples"]).max() < 0.01
    assert z["baselines"].tolist() == [list(b) for b in ps["bls"]]


def test_tool_scan_only_returns_the_delays(tmp_path):
    gate_vis, used = IR.delayed_gate(5, 8, (0, 58, 131))
    np.savez(tmp_path / "out.npz", vis=gate_vis[0], rows_used=used[0])
    z = _tool(str(tmp_path / "scan.npz"), "--vis", tmp_path / "out.npz", "--scan-only")
    assert "image" not in z.files
    assert z["fine_samples"].shape == (2, 3) and z["scan_x"].shape == (101,)
    assert np.abs(z["fine_samples"] - [58, 131, 73]).max() <= 0.1
    assert np.abs(z["fit_samples"] - [0, 58, 131]).max() <= 0.1
