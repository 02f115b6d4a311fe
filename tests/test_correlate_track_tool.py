"""python -m vlite-fast_amd.correlate --track / --track-model: the arguments' parsing and the model's file on the CPU,
and on the GPU the whole tool as a child process over two dump files of a source whose phase and delay drift."""
import importlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import fringe_synth as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NFFT, NCO = 12500, 4096
BASE = ["--replay", "a.uw", "b.uw", "-o", "x.npz"]
GEOMETRY = ["--antennas", "ants.txt", "--centre", "83.6", "22.0", "--time", "1700000000"]


def corr():
    return importlib.import_module("vlite-fast_amd.correlate")


def test_parser():
    c = corr()
    a = c.parse_args(BASE)
    assert not a.track and a.track_model is None and a.antennas is None
    a = c.parse_args(BASE + ["--track"] + GEOMETRY + ["--clock-ns", "0", "12.5"])
    assert a.track and a.antennas == "ants.txt" and a.centre == [83.6, 22.0] and a.time == 1.7e9 and a.clock_ns == [0, 12.5]
    a = c.parse_args(BASE + ["--track-model", "m.txt"])
    assert a.track_model == "m.txt" and not a.track
    for bad in (["--track"], ["--track"] + GEOMETRY[:2], ["--track"] + GEOMETRY[2:], ["--track"] + GEOMETRY[:5],
                ["--track", "--track-model", "m.txt"] + GEOMETRY, ["--track", "--track-model", "m.txt"],
                GEOMETRY, ["--clock-ns", "1", "2"], ["--track-model", "m.txt"] + GEOMETRY,
                ["--track", "--antennas", "ants.txt", "--centre", "83.6", "95", "--time", "1"]):
        with pytest.raises(SystemExit):
            c.parse_args(BASE + bad)


def test_model_file_and_geometry(tmp_path):
    c = corr()
    path = str(tmp_path / "m.txt")
    with open(path, "w") as f:
        f.write("# delay0 delay_rate psi0 psi_rate\n0 0 0 0\n58.25 1e-2 -0.1 -6.25e-2  # antenna 1\n\n")
    a = c.parse_args(BASE + ["--track-model", path])
    assert np.array_equal(c.tracking_model(a), [[0, 0, 0, 0], [58.25, 0.01, -0.1, -0.0625]])
    assert c.tracking_model(c.parse_args(BASE)) is None
    for text in ("0 0 0 0\n", "0 0 0 0\n1 2 3\n", "0 0 0 0\n1 2 3 x\n", "0 0 0 0\n1 2 3 4\n5 6 7 8\n"):
        with open(path, "w") as f:
            f.write(text)
        with pytest.raises(SystemExit):
            c.tracking_model(a)
    # --track: localise.track_model of the position, relative to antenna 0
    loc = importlib.import_module("vlite-fast_amd.localise")
    xyz = np.array([[-1601185.4, -5041977.5, 3554875.9], [-1600185.4, -5042977.5, 3554975.9]])
    ants = str(tmp_path / "ants.txt")
    with open(ants, "w") as f:
        for k, r in enumerate(xyz):
            f.write("ea%02d %r %r %r\n" % (k, float(r[0]), float(r[1]), float(r[2])))
    a = c.parse_args(BASE + ["--track", "--antennas", ants, "--centre", "83.6", "22.0", "--time", "1700000000",
                             "--clock-ns", "0", "12.5"])
    m = c.tracking_model(a)
    full = loc.track_model(xyz, np.radians(83.6), np.radians(22.0), 1.7e9, [0, 12.5])
    assert m.shape == (2, 4) and np.all(m[0] == 0) and np.array_equal(m[1], full[1] - full[0]) and np.all(m[1] != 0)


@pytest.mark.gpu
def test_tool_stops_the_fringes_of_two_dumps(tmp_path):
    """antenna 1 sees the common signal 58.25 samples late, drifting by 0.01 samples and 1/16 turn a row: every 16-row
    gate of the plain run adds a whole turn of phase.  The model leaves the delay's start in (delay0 = 0), so that the
    tool's own fit still finds it."""
    genbase = importlib.import_module("vlite-fast_amd.genbase")
    R, S = 16, 4
    d0, d1, p0, p1 = (0.0, 58.25), (0.0, 0.01), (0.0, 0.1), (0.0, 1.0 / 16)
    u8 = FS.drifting_antennas(9, R * S, d0, d1, p0, p1)
    files = []
    for a in range(2):
        path = str(tmp_path / ("ant%d.uw" % a))
        assert genbase.write_observation(path, [(u8[a, 0], u8[a, 1])], time.time(), station=a) == R * S * NFFT // 5000
        files.append(path)
    model = str(tmp_path / "m.txt")
    with open(model, "w") as f:
        f.write("0 0 0 0\n0 %r 0 %r\n" % (d1[1], -p1[1]))

    def tool(out, *extra):
        cmd = [sys.executable, "-m", "vlite-fast_amd.correlate", "--replay"] + files + [
            "--rows-per-seg", str(R), "--max-seg", str(S), "--int-rows", "16", "-o", out] + list(extra)
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        return np.load(out)

    plain = tool(str(tmp_path / "plain.npz"))
    z = tool(str(tmp_path / "tracked.npz"), "--track-model", model, "--dm", "0.2", "--t0", "20", "--width", "8",
             "--off-gates", "1")
    assert "track_model" not in plain.files
    assert np.array_equal(z["track_model"], [[0, 0, 0, 0], [0, d1[1], 0, -p1[1]]]) and z["track_row_base"].tolist() == [0]
    print("lag_peak 0-1, tracked and plain:", z["lag_peak"][:, 0, 1], plain["lag_peak"][:, 0, 1])
    assert np.all(z["lag_peak"][:, 0, 1] >= 2 * plain["lag_peak"][:, 0, 1])
    res = NFFT / float(NCO)                          # the lag resolution, 3.05 samples
    assert np.all(np.abs(z["delay_samples"][:, 1] - d0[1]) <= 0.5 * res)
    assert z["gate_vis"].shape == (3, 3, 4, NCO) and np.all(z["gate_rows_used"] == 8)
    assert np.all(z["rows_used"] == R * S) and np.array_equal(plain["rows_used"], z["rows_used"])
