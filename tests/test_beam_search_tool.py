"""python -m vlite-fast_amd.beamform --search / --fil: the parser's refusals and the planes' header on the CPU; on the GPU
the whole tool as a child process over three dumps that share an undispersed burst (tests/burst_synth.py): the coherent
beam at the true delays is searched where it lies on the GPU and finds the burst at its sample with more S/N than the
same search finds in any single-antenna beam, and the .fil bytes are the restated planes' restated codes."""
import importlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import beam_plane_ref as PR
import search_plane_ref as QR
from burst_synth import burst_antennas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NFFT, NCO = 12500, 4096
BASE = ["--replay", "a", "b", "--delays", "0", "1", "-o", "x", "--rows-per-seg", "16", "--max-seg", "6"]


def tool():
    return importlib.import_module("vlite-fast_amd.beamform")


def test_parser_refusals(capsys):
    b = tool()
    a = b.parse_args(BASE + ["--search", "-dm 0 10 -detect_thresh 7", "--tscr", "2"])
    assert a.search_flags.dm == [0.0, 10.0] and a.search_flags.detect_thresh == 7.0 and a.level_alpha == 0.25
    assert a.fil is None and not a.search_single
    assert b.parse_args(BASE).search_flags is None
    a = b.parse_args(BASE + ["--fil", "d", "--search-single", "--level-alpha", "0.5"])
    assert (a.fil, a.search_single, a.level_alpha, a.tscr) == ("d", True, 0.5, 8)
    for bad, msg in ((["--search", "", "--dm", "5"], "not with --dm"), (["--fil", "d", "--dm", "5"], "not with --dm"),
                     (["--search", "", "--tscr", "5"], "must divide"), (["--search-single"], "needs --search"),
                     (["--fil", "d", "--tscr", "4"], "781.25 us"), (["--search", "", "--level-alpha", "0"], "level-alpha"),
                     (["--search", "-f x.fil"], "unrecognized"), (["--search", "-nosuchflag 1"], "unrecognized")):
        with pytest.raises(SystemExit):
            b.parse_args(BASE + bad)
        assert msg in capsys.readouterr().err, bad


def test_plane_header_is_bin_2155_plus_c():
    """plane channel c is FFT bin 2155 + c: the reference's header convention, fch1 + c foff = 384 - (2155 + c - 0.5) 64 / 6251"""
    hdr = tool().plane_header(2)
    c = np.arange(NCO, dtype=np.float64)
    assert hdr["nchans"] == NCO and hdr["tsamp"] == 2 * 12500 / 128e6
    assert np.allclose(hdr["fch1"] + c * hdr["foff"], 384.0 - (2155 + c - 0.5) * 64.0 / 6251, rtol=0, atol=1e-9)
    assert tool().plane_header(8)["tsamp"] == 781.25e-6


def test_running_level():
    b = tool()
    F = np.float32
    first = np.array([[4.0, 0.0, 2.0, 0.0]], F)
    run = b.update_level(None, first, 0.25)
    assert run.dtype == F and np.array_equal(run, first) and run is not first
    run = b.update_level(run, np.array([[8.0, 6.0, 0.0, 0.0]], F), 0.25)
    # moved a quarter of the way; a channel without a level yet takes the batch's; a batch without one changes nothing
    assert run.dtype == F and run.tolist() == [[5.0, 6.0, 2.0, 0.0]]


@pytest.mark.gpu
def test_tool_searches_the_coherent_beam(tmp_path):
    genbase = importlib.import_module("vlite-fast_amd.genbase")
    R, S = 16, 6                                       # two batches of 96 rows: 2.4 MB per pol and antenna
    nrows, d = 2 * R * S, (0, 58, 131)
    tscr, at = 2, 50                                   # the burst fills output sample 50 of 96, the third of batch 2
    u8 = burst_antennas(11, nrows, d, at * tscr, (at + 1) * tscr, 0.15)
    files = []
    for a in range(3):
        path = str(tmp_path / ("ant%d.uw" % a))
        assert genbase.write_observation(path, [(u8[a, 0], u8[a, 1])], time.time(), station=a) == nrows * NFFT // 5000
        files.append(path)

    def run(out, *extra):
        cmd = [sys.executable, "-m", "vlite-fast_amd.beamform", "--replay"] + files + [
            "--rows-per-seg", str(R), "--max-seg", str(S), "--delays", "0", "58", "131", "-o", out] + list(extra)
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        return np.load(out), r.stdout.decode()

    flags = "-dm 0 0.1 -dm_step 0.1 -boxcar_max 4 -detect_thresh 6 -baseline_length 0 -nsamps_gulp %d"
    z, text = run(str(tmp_path / "search.npz"), "--tscr", str(tscr), "--search", flags % (nrows // tscr), "--search-single")
    cands = z["search_cands"]
    print(text[-1500:])
    print("beam, S/N, peak, tfilt, dmi, dm:\n", cands)
    best = {}
    for beam, snr, peak, _, _, _ in cands:
        if int(beam) not in best or snr > best[int(beam)][0]:
            best[int(beam)] = (snr, int(peak))
    assert 1 in best and best[1][1] == at               # the coherent beam's candidate at the burst's sample
    for single in (2, 3, 4):                            # the one-hot beams through the same path: less S/N, or none at all
        assert best[1][0] > best.get(single, (0.0, at))[0], (single, best)
    assert any(b in best for b in (2, 3, 4))

    # the filterbank files, at the filterbank's own sampling
    fil = str(tmp_path / "fil")
    z, _ = run(str(tmp_path / "fil.npz"), "--fil", fil, "--search", flags % (nrows // 8), "--search-single")
    assert z["search_cands"].shape == (0, 6)            # 24 samples: less than one gulp's output
    sigproc = importlib.import_module("vlite-fast_amd.sigproc")
    assert sorted(os.listdir(fil)) == ["beam%02d.fil" % b for b in (1, 2, 3, 4)]
    per = R * S // 8
    for b in (1, 2, 3, 4):
        blob = open(os.path.join(fil, "beam%02d.fil" % b), "rb").read()
        hdr, off = sigproc.read_header(blob[:4096])
        assert (hdr["nchans"], hdr["nbits"], hdr["nifs"], hdr["tsamp"]) == (NCO, 8, 1, 781.25e-6)
        assert hdr["source_name"] == "beam%02d" % b and len(blob) - off == 2 * per * NCO
        if b == 1:                                      # the coherent beam: its block is in the npz
            beams, used = z["beams"], z["rows_used"]
            first, L = PR.planes(beams[:, :per], used[:, :per], 8)
            second, _ = PR.planes(beams[:, per:], used[:, per:], 8, L)              # batch 2 over the running level
            want = QR.quantise8(np.concatenate([first[0], second[0]]))
            got = np.frombuffer(blob[off:], np.uint8).reshape(2 * per, NCO)
            assert np.array_equal(got, want) and len(np.unique(got)) > 50
