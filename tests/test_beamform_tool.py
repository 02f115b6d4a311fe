"""python -m vlite-fast_amd.beamform: its argument parser and beam tables on the CPU, and on the GPU the whole tool as a
child process over three small dump files whose antennas share half their power at delays 0, 58 and 131 samples."""
import importlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import correlate_ref as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NFFT, NCO = 12500, 4096


def tool():
    return importlib.import_module("vlite-fast_amd.beamform")


def test_parser():
    b = tool()
    a = b.parse_args(["--replay", "a.uw", "b.uw", "--delays", "0", "-58.25", "-o", "x.npz"])
    assert a.replay == ["a.uw", "b.uw"] and a.offsets == [0, 0] and a.stream == "raw" and a.delays == [0.0, -58.25]
    assert a.beams is None and a.loc is None and not a.phase_turns and a.dm is None and a.tscr == 8
    assert (a.rows_per_seg, a.max_seg, a.seconds) == (1024, 10, 0)
    a = b.parse_args(["--replay", "a", "b", "--offsets", "0", "58", "--stream", "kur", "--beams", "t.txt", "--phase-turns",
                      "--dm", "56.7", "--tscr", "4", "--rows-per-seg", "8", "--max-seg", "2", "--seconds", "3", "-o", "x"])
    assert a.offsets == [0, 58] and a.stream == "kur" and a.beams == "t.txt" and a.phase_turns and a.delays is None
    assert (a.dm, a.tscr, a.rows_per_seg, a.max_seg, a.seconds) == (56.7, 4, 8, 2, 3)
    assert b.parse_args(["--replay", "a", "--loc", "l.npz", "-o", "x"]).loc == "l.npz"
    for bad in (["--replay", "a", "-o", "x"],                                             # no beam
                ["--replay", "a", "-o", "x", "--delays", "0", "--loc", "l.npz"],         # two sources of beams
                ["--replay", "a", "b", "-o", "x", "--delays", "0"], ["--replay", "a", "-o", "x", "--delays", "nan"],
                ["--replay", "a", "-o", "x", "--delays", "0", "--offsets", "-1"],
                ["--replay", "a", "-o", "x", "--delays", "0", "--offsets", "1", "2"],
                ["--replay", "a", "-o", "x", "--delays", "0", "--tscr", "0"],
                ["--replay", "a", "-o", "x", "--delays", "0", "--tscr", "17", "--rows-per-seg", "8", "--max-seg", "2"],
                ["--replay", "a", "-o", "x", "--delays", "0", "--dm", "-1"],
                ["--replay", "a", "-o", "x", "--delays", "0", "--stream", "both"],
                ["--replay", "a", "-o", "x", "--delays", "0", "--rows-per-seg", "12"],
                ["--replay", "a", "--delays", "0"], ["--replay"] + ["a"] * 9 + ["-o", "x", "--delays"] + ["0"] * 9):
        with pytest.raises(SystemExit):
            b.parse_args(bad)


def test_beam_tables(tmp_path):
    b = tool()
    loc = importlib.import_module("vlite-fast_amd.localise")
    path = str(tmp_path / "beams.txt")
    with open(path, "w") as f:
        f.write("# three antennas\n0 58 131.5\n\n0 -58 -131.5   # negated\n")
    args = b.parse_args(["--replay", "a", "b", "c", "--beams", path, "--phase-turns", "-o", "x"])
    delay, psi = b.beam_table(args)
    # psi is added to an antenna's phase: it takes off what phase_turns says the antenna carries
    assert delay.tolist() == [[0, 58, 131.5], [0, -58, -131.5]] and np.array_equal(psi, -loc.phase_turns(delay))
    assert np.array_equal(psi, 3.0 * delay)
    with pytest.raises(ValueError, match="2 delays, 3 antennas"):
        open(path, "a").write("1 2\n")
        b.read_beams(path, 3)
    # the localise tool's per-antenna delays: fit_samples [2 slots][nant], samples later than antenna 0
    npz = str(tmp_path / "loc.npz")
    np.savez(npz, fit_samples=np.array([[0, 58.0, 131.0], [0, 58.5, 130.0]]))
    delay, psi = b.beam_table(b.parse_args(["--replay", "a", "b", "c", "--loc", npz, "-o", "x"]))
    assert delay.tolist() == [[0, 58.25, 130.5]] and psi is None
    with pytest.raises(ValueError, match="antennas"):
        b.loc_delays(npz, 2)
    d, g = b.one_hot(3)
    assert d.shape == (3, 3) and not d.any() and np.array_equal(g, np.eye(3, dtype=np.float32))
    assert np.allclose(b.ratio(np.array([[2.0, 4.0], [1.0, 2.0]]), np.array([1.0, 2.0])), [2.0, 1.0])


@pytest.mark.gpu
def test_tool_adds_three_dumps_coherently(tmp_path):
    genbase = importlib.import_module("vlite-fast_amd.genbase")
    corr = importlib.import_module("vlite-fast_amd.correlate")
    R, S, tscr = 8, 2, 4
    n = 2 * R * S * NFFT                               # two batches of 16 rows
    d = (0, 58, 131)
    u8 = XR.delayed_antennas(5, n, d)
    files = []
    for a in range(3):
        path = str(tmp_path / ("ant%d.uw" % a))
        assert genbase.write_observation(path, [(u8[a, 0], u8[a, 1])], time.time(), station=a) == n // 5000
        files.append(path)
    beams_txt = str(tmp_path / "beams.txt")
    with open(beams_txt, "w") as f:
        f.write("0 58 131\n0 -58 -131\n")

    def run(out, *extra):
        cmd = [sys.executable, "-m", "vlite-fast_amd.beamform", "--replay"] + files + [
            "--rows-per-seg", str(R), "--max-seg", str(S), "--tscr", str(tscr), "-o", out] + list(extra)
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        return np.load(out)

    z = run(str(tmp_path / "two.npz"), "--beams", beams_txt)
    nout = 2 * R * S // tscr
    assert z["beams"].shape == (2, nout, 4, NCO) and z["beams"].dtype == np.float32
    assert z["rows_used"].shape == (2, nout, NCO) and np.all(z["rows_used"] == tscr)
    assert z["sample_row"].tolist() == list(range(0, 2 * R * S, tscr)) and not z["shift"].any()
    assert z["incoherent"].shape == (nout, 4, NCO) and z["incoherent"].dtype == np.float64
    assert z["series"].shape == (2, nout) and z["incoherent_series"].shape == (nout,) and z["ratio"].shape == (2,)
    assert z["delays"].tolist() == [[0, 58, 131], [0, -58, -131]] and not z["phase_turns"].any()
    assert np.allclose(z["series"], z["beams"][:, :, :2].astype(np.float64).sum(axis=(2, 3)))
    print("coherent / incoherent: true %.4f  negated %.4f" % tuple(z["ratio"]))
    assert z["ratio"][0] >= 1.9 and z["ratio"][1] <= 1.1
    # dedispersed output samples: per batch those whose window lies in the batch in every channel
    z = run(str(tmp_path / "dm.npz"), "--delays", "0", "58", "131", "--dm", "0.05", "--stream", "kur")
    shift = corr.dm_row0(0.05, 0, R * S)
    per = (R * S - shift.max()) // tscr
    assert shift.max() >= 3 and np.array_equal(z["shift"], shift)
    assert z["beams"].shape == (1, 2 * per, 4, NCO) and z["rows_used"].shape == (1, 2 * per, NCO)
    assert z["sample_row"].tolist() == [k * R * S + tscr * s for k in range(2) for s in range(per)]
    assert z["ratio"][0] >= 1.9
