"""python -m vlite-fast_amd.correlate: its argument parser and baseline order on the CPU, and on the GPU the whole tool as
a child process over two dump files whose second antenna is 58 samples late."""
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


def corr():
    return importlib.import_module("vlite-fast_amd.correlate")


def test_baselines_are_in_the_library_order():
    c = corr()
    for nant in range(1, 9):
        bls = c.baselines(nant)
        assert len(bls) == nant * (nant + 1) // 2
        for k, (i, j) in enumerate(bls):
            assert i <= j and k == i * nant - i * (i - 1) // 2 + (j - i)
    assert c.baselines(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert np.allclose(c.chan_freqs_mhz()[[0, 4095]], [384 - 2155 * 64 / 6251., 384 - 6250 * 64 / 6251.])


def test_parser():
    c = corr()
    a = c.parse_args(["--replay", "a.uw", "b.uw", "-o", "x.npz"])
    assert a.replay == ["a.uw", "b.uw"] and a.offsets == [0, 0] and a.stream == "raw" and a.int_rows == 1024
    assert a.dm is None and a.off_gates == 2 and (a.rows_per_seg, a.max_seg) == (1024, 10)
    a = c.parse_args(["--replay", "a", "b", "--offsets", "0", "58", "--stream", "kur", "--int-rows", "512", "--seconds", "3",
                      "--dm", "56.7", "--t0", "100", "--width", "20", "--off-gates", "1", "-o", "x"])
    assert a.offsets == [0, 58] and a.stream == "kur" and a.int_rows == 512 and a.seconds == 3
    assert (a.dm, a.t0, a.width, a.off_gates) == (56.7, 100, 20, 1)
    for bad in (["--replay", "a", "-o", "x", "--offsets", "1", "2"], ["--replay", "a", "-o", "x", "--offsets", "-1"],
                ["--replay", "a", "-o", "x", "--dm", "5"], ["--replay", "a", "-o", "x", "--int-rows", "0"],
                ["--replay", "a", "-o", "x", "--int-rows", "1000"], ["--replay", "a", "-o", "x", "--stream", "both"],
                ["--replay", "a", "-o", "x", "--dm", "5", "--t0", "1", "--width", "0"], ["--replay", "a"],
                ["--replay"] + ["a"] * 9 + ["-o", "x"], ["--replay", "a", "-o", "x", "--rows-per-seg", "12"]):
        with pytest.raises(SystemExit):
            c.parse_args(bad)


@pytest.mark.gpu
def test_tool_finds_the_delay_between_two_dumps(tmp_path):
    genbase = importlib.import_module("vlite-fast_amd.genbase")
    R, S = 64, 4                                    # one batch of 256 rows; one more frame so that the late antenna,
    n = R * S * NFFT + 5000                         # advanced by 58 samples, still fills it
    u8 = XR.delayed_antennas(9, n, (0, 58))
    files = []
    for a in range(2):
        path = str(tmp_path / ("ant%d.uw" % a))
        assert genbase.write_observation(path, [(u8[a, 0], u8[a, 1])], time.time(), station=a) == n // 5000
        files.append(path)

    def tool(out, *extra):
        cmd = [sys.executable, "-m", "vlite-fast_amd.correlate", "--replay"] + files + [
            "--rows-per-seg", str(R), "--max-seg", str(S), "--int-rows", "64", "-o", out] + list(extra)
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        return np.load(out)

    res = NFFT / float(NCO)                          # the lag resolution, 3.05 samples
    z = tool(str(tmp_path / "plain.npz"), "--dm", "0.3", "--t0", "40", "--width", "8", "--off-gates", "2")
    assert z["vis"].shape == (3, 4, NCO) and z["vis"].dtype == np.complex128
    assert z["rows_used"].shape == (3, NCO) and np.all(z["rows_used"] == R * S)
    assert z["baselines"].tolist() == [[0, 0], [0, 1], [1, 1]] and z["freqs_mhz"].shape == (NCO,)
    assert int(z["rows"]) == R * S
    assert np.all(z["lag_cycles"][:, 0, 1] == 19 / 4096.0)
    assert np.all(z["delay_samples"][:, 0] == 0) and np.all(np.abs(z["delay_samples"][:, 1] - 58) <= res / 2)
    assert np.array_equal(z["fit_samples"], -z["delay_samples"])
    # the gates: two off, the on-gate, two off, eight rows each, dedispersed alike
    assert z["gate_vis"].shape == (5, 3, 4, NCO) and z["gate_vis"].dtype == np.complex64
    assert z["gate_rows_used"].shape == (5, 3, NCO) and np.all(z["gate_rows_used"] == 8)
    assert z["gate_row0"].shape == (5, NCO) and int(z["gate_on"]) == 2
    assert z["gate_row0"][:, 0].tolist() == [24, 32, 40, 48, 56]
    assert np.array_equal(z["gate_row0"][2], corr().dm_row0(0.3, 40, R * S))
    assert np.all(z["gate_vis"][:, 0, 0].real > 0)
    # the antennas lined up: no delay left
    z = tool(str(tmp_path / "lined_up.npz"), "--offsets", "0", "58")
    assert np.all(z["lag_cycles"] == 0) and np.all(z["delay_samples"] == 0)
    assert "gate_vis" not in z.files
