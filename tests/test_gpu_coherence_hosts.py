"""Both hosts with -P 2 --coherence on a replayed dump: byte-identical .fil files and ring sinks, a SIGPROC header
with nifs 4, whole segments of AA, BB, CR, CI whose AA and BB are the -P 2 run's file and whose CR and CI are the
CPU reference's (tests/coherence_ref.py)."""
import importlib
import os

import numpy as np
import pytest

import coherence_ref as CR
from helpers import make_input
from test_native_exe import R, SEG, _argv, _dump, _run

pytestmark = pytest.mark.gpu

vdif = importlib.import_module("vlite-fast_amd.vdif")
sigproc = importlib.import_module("vlite-fast_amd.sigproc")
pbmod = importlib.import_module("vlite-fast_amd.process_baseband")
FILES = ("20160701_010000_muos_ea07.fil", "20160701_010000_muos_ea07_kur.fil", "co.bin", "out.bin")


def _host(who, d, dump, extra):
    d.mkdir()
    argv = _argv(d, dump, 8, extra)
    argv[argv.index("-P") + 1] = "2"
    if who == "py":
        assert pbmod.run(pbmod.build_parser().parse_args(argv)) == 0
    else:
        r = _run(argv)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    return {n: (d / n).read_bytes() for n in FILES}


def test_hosts_write_the_same_coherence_files(tmp_path, oracle):
    nsec = 4
    data = make_input(29, R, nsec * SEG)
    dump = str(tmp_path / "obs.uw")
    _dump(dump, data)
    outs = {who: _host(who, tmp_path / who, dump, ["--coherence"]) for who in ("py", "cxx")}
    p2 = _host("cxx", tmp_path / "p2", dump, [])
    for n in FILES:
        a, b = outs["py"][n], outs["cxx"][n]
        if n.endswith(".bin"):       # ring stand-ins: the header names the .fil file, whose directory differs here
            ha, hb = vdif.ascii_header_parse(a[:4096]), vdif.ascii_header_parse(b[:4096])
            assert ha["NPOL"] == "4" and hb["NPOL"] == "4", n
            ha["SIGPROC_FILE"], hb["SIGPROC_FILE"] = os.path.basename(ha["SIGPROC_FILE"]), os.path.basename(hb["SIGPROC_FILE"])
            assert ha == hb and list(ha) == list(hb), n
            a, b = a[4096:], b[4096:]
        assert a == b, n
    nseg = (nsec - 1) * SEG                    # the last second is not written (as the reference)
    trim = 4 * (R // 8) * 4096                 # code bytes per segment, 8 bit
    hdr = sigproc.sigproc_header(7, 0.8718, -0.72452, "B0833-45", 57570 + 3600 / 86400., 4, 8)
    hdr2 = sigproc.sigproc_header(7, 0.8718, -0.72452, "B0833-45", 57570 + 3600 / 86400., 2, 8)
    ref = CR.run(oracle, data[:nseg], R, 2, 8)
    for n, st in ((FILES[0], 0), (FILES[1], 1)):
        f = outs["cxx"][n]
        assert f[:len(hdr)] == hdr, n                          # nifs 4
        body = np.frombuffer(f[len(hdr):], np.uint8)
        assert body.size == nseg * trim, n                     # whole segments
        assert p2[n][:len(hdr2)] == hdr2
        body2 = np.frombuffer(p2[n][len(hdr2):], np.uint8)
        assert np.array_equal(body.reshape(-1, 4, 4096)[:, :2].ravel(), body2), n     # IFs 0, 1 = the -P 2 file
        assert np.array_equal(body, ref[st][0]), n             # CR, CI as the CPU reference
    co = np.frombuffer(outs["cxx"]["co.bin"][4096:], np.uint8)
    assert np.array_equal(co, ref[1][0])                       # the coadd ring carries the excised stream
