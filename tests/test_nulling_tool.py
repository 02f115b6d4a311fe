"""python -m vlite-fast_amd.beamform --null: the options' parsing, the tool's batch loop and npz fields over a stand-in
handle made of the restatements (no GPU), and on the GPU the whole tool as a child process over four small dump files
that share an interferer of ten times their own noise (tests/null_synth.py)."""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import beam_ref as BR
import beamproj_ref as PR
import correlate_ref as XR
import null_synth as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NFFT, NCO = 12500, 4096


def tool():
    return importlib.import_module("vlite-fast_amd.beamform")


def test_parser():
    b = tool()
    base = ["--replay", "a", "b", "c", "--delays", "0", "1", "2", "-o", "x", "--rows-per-seg", "8", "--max-seg", "2"]
    a = b.parse_args(base)
    assert a.null is None and a.null_min_ratio is None and a.null_train is None
    a = b.parse_args(base + ["--null", "2"])
    assert a.null == 2 and a.null_min_ratio is None and a.null_train is None
    a = b.parse_args(base + ["--null", "1", "--null-min-ratio", "4.5", "--null-train", "0", "12"])
    assert a.null == 1 and a.null_min_ratio == 4.5 and a.null_train == [0, 12]
    assert b.parse_args(base + ["--null", "1", "--null-train", "15", "16"]).null_train == [15, 16]
    for bad in (["--null", "0"], ["--null", "3"], ["--null", "-1"], ["--null-min-ratio", "2"], ["--null-train", "0", "8"],
                ["--null", "1", "--null-min-ratio", "0"], ["--null", "1", "--null-min-ratio", "-2"],
                ["--null", "1", "--null-train", "4", "4"], ["--null", "1", "--null-train", "-1", "4"],
                ["--null", "1", "--null-train", "0", "17"], ["--null", "1", "--null-train", "3"]):
        with pytest.raises(SystemExit):
            b.parse_args(base + bad)
    with pytest.raises(SystemExit):                                   # one antenna has no direction to null
        b.parse_args(["--replay", "a", "--delays", "0", "-o", "x", "--null", "1"])


class RefHandle(object):
    """what the tool calls of a PbHandle, on given spectra through the restatements"""

    def __init__(self, X, R):
        self.X, self.rows, self.nant = X, R, X.shape[0]
        self.calls = []

    def beamform(self, stream, nseg, delay, psi=None, gain=None, shift=None, tscr=1, nout=None):
        self.calls.append(("beamform", np.atleast_2d(delay).shape[0]))
        return BR.beamform(self.X, None, delay, psi, gain, shift, tscr, nout)

    def beamform_proj(self, stream, nseg, delay, proj, psi=None, gain=None, shift=None, tscr=1, nout=None):
        self.calls.append(("beamform_proj", np.atleast_2d(delay).shape[0]))
        return PR.beamform_proj(self.X, None, delay, proj, psi, gain, shift, tscr, nout)

    def correlate_gated(self, stream, nseg, row0, nrows):
        self.calls.append(("correlate_gated", np.asarray(row0)[:, 0].tolist(), nrows))
        return XR.correlate(self.X, None, row0, nrows)


def test_tool_over_the_restatements(tmp_path, monkeypatch):
    b = tool()
    nulling = importlib.import_module("vlite-fast_amd.nulling")
    R, S, A, tscr = 8, 2, 3, 4
    rng = np.random.default_rng(6)
    handles = []
    for k in range(2):
        x = rng.standard_normal((A, 2, R * S, NCO)) + 1j * rng.standard_normal((A, 2, R * S, NCO))
        x[1, :, :, 50] = 0                                            # a channel that one antenna lacks
        x[:, 1, :, 60] = 0                                            # a zapped channel of pol 1
        handles.append(RefHandle(x.astype(np.complex64), R))
    monkeypatch.setattr(b.replay_batches, "batches", lambda args, prog: ((k, h, 0) for k, h in enumerate(handles)))
    argv = ["--replay", "a", "b", "c", "--delays", "0", "58", "131", "--rows-per-seg", str(R), "--max-seg", str(S),
            "--tscr", str(tscr)]
    plain = b.run(b.parse_args(argv + ["-o", str(tmp_path / "plain.npz")]))
    assert "null_count" not in plain and not any(k.startswith("null") for k in json.loads(str(plain["options"])))
    assert [c[0] for h in handles for c in h.calls] == ["beamform", "beamform"]
    for h in handles:
        del h.calls[:]
    out = b.run(b.parse_args(argv + ["-o", str(tmp_path / "null.npz"), "--null", "1", "--null-train", "2", "13"]))
    z = np.load(str(tmp_path / "null.npz"))
    assert sorted(z.files) == sorted(list(np.load(str(tmp_path / "plain.npz")).files) + ["null_count"])
    opts = json.loads(str(z["options"]))
    assert opts["null"] == 1 and opts["null_train"] == [2, 13] and opts["null_min_ratio"] is None
    nout = 2 * R * S // tscr
    assert z["beams"].shape == (1, nout, 4, NCO) and z["beams"].dtype == np.float32
    assert z["rows_used"].shape == (1, nout, NCO) and np.all(z["rows_used"] == tscr)
    assert z["null_count"].shape == (2, NCO) and z["null_count"].dtype == np.int64
    want = np.full((2, NCO), 2)
    want[1, 60] = 0                                                   # all zero: the identity, in both batches
    assert np.array_equal(z["null_count"], want)
    # per batch: the training rows in gates of at most a segment, the coherent beam nulled, the one-hot beams not
    for h in handles:
        assert h.calls == [("correlate_gated", [2], 8), ("correlate_gated", [10], 3), ("beamform_proj", 1), ("beamform", A)]
    # the incoherent beam and its series are those of the run without --null; the coherent beams are the restatement's
    assert np.array_equal(z["incoherent"], plain["incoherent"])
    assert np.array_equal(z["incoherent_series"], plain["incoherent_series"])
    assert np.allclose(z["ratio"], z["series"].sum(axis=-1) / z["incoherent_series"].sum())
    for k, h in enumerate(handles):
        vis = sum(XR.correlate(h.X, None, np.full((1, NCO), r0), n)[0].astype(np.complex128).sum(axis=0)
                  for r0, n in ((2, 8), (10, 3)))
        proj, _ = nulling.projectors(nulling.covariances(vis, A), 1)
        ref, _ = PR.beamform_proj(h.X, None, [[0.0, 58.0, 131.0]], proj, tscr=tscr)
        assert np.array_equal(z["beams"][:, k * nout // 2:(k + 1) * nout // 2], ref)
    assert z["series"].sum() < plain["series"].sum()
    assert np.array_equal(out["beams"], z["beams"])
    # --null-min-ratio reaches projectors: with a ratio no channel has, nothing is nulled and the beams are the plain ones
    z = b.run(b.parse_args(argv + ["-o", str(tmp_path / "ratio.npz"), "--null", "1", "--null-min-ratio", "1e9"]))
    assert not z["null_count"].any() and np.array_equal(z["beams"], plain["beams"])


@pytest.mark.gpu
def test_tool_nulls_the_interferer(tmp_path):
    genbase = importlib.import_module("vlite-fast_amd.genbase")
    R, S = 16, 4
    n = R * S * NFFT                                   # one batch of 64 rows
    u8 = NS.case_antennas()
    files = []
    for a in range(4):
        path = str(tmp_path / ("ant%d.uw" % a))
        assert genbase.write_observation(path, [(u8[a, 0], u8[a, 1])], time.time(), station=a) == n // 5000
        files.append(path)

    def run(out, *extra):
        cmd = [sys.executable, "-m", "vlite-fast_amd.beamform", "--replay"] + files + [
            "--rows-per-seg", str(R), "--max-seg", str(S), "--tscr", "1", "-o", out, "--delays"] + [
            "%r" % d for d in NS.CASE["sky_delays"]] + list(extra)
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        return np.load(out)

    plain = run(str(tmp_path / "plain.npz"))
    z = run(str(tmp_path / "null.npz"), "--null", "1", "--null-train", str(NS.TRAIN[0]), str(NS.TRAIN[1]))
    assert "null_count" not in plain.files and np.all(z["null_count"] == 1)
    assert z["beams"].shape == plain["beams"].shape == (1, 64, 4, NCO)
    off, con = NS.report("the tool, --null 1", plain["beams"], z["beams"])
    assert np.all(off <= NS.OFF_RATIO_MAX) and np.all(con >= NS.CONTRAST_RATIO_MIN)
    assert np.array_equal(z["incoherent"], plain["incoherent"]) and z["ratio"][0] < plain["ratio"][0]
