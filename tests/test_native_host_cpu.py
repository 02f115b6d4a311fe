"""The native host program's loop (vlite-fast_amd/csrc/process_baseband) without a GPU: its own sources, as the
Makefile lists them, linked against the stand-in for libpb_hip.so of tests/fake_pb and built with AddressSanitizer and
UBSan (runtimes linked statically into the program, so it needs nothing preloaded and does not mind what is; leak
detection on).  The stand-in deframes on the host and returns,
per segment, a fold of ALL its samples (fake_pb.cpp states it, _fold restates it), so a frame misplaced anywhere in a
second changes the files.  Every case is a --replay at --rows-per-seg 8 (2 MB per second of data) that ends through the
program's normal cleanup, and asserts the exact exit status and that nothing came out on stderr.

Cases: the smallest streams that reach each branch of the frame assembly (SecondReader: a short second swallowing the
head of the next one, invalid-bit marking, a duplicate frame once the block is full, truncation, a major skip), the -r
modes, two observations in one run, CMD_QUIT -- and the same streams through process_baseband.py's run() over a
stand-in with the same fold: both hosts must write the same bytes."""
import importlib
import os
import socket
import subprocess
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vlite-fast_amd", "csrc")
vdif = importlib.import_module("vlite-fast_amd.vdif")
sigproc = importlib.import_module("vlite-fast_amd.sigproc")
pbmod = importlib.import_module("vlite-fast_amd.process_baseband")

R, SEG = 8, 10
SEG_SAMP = R * 12500                   # samples per pol per segment
NS = SEG * SEG_SAMP                    # samples per pol per (shortened) second
FPS = NS // 5000                       # frames per thread per second = 200
TRIM = 2 * R * 4096 // 16              # 8-bit, npol 1
SEC0 = 3600
FIL, KUR = "20160701_010000_muos_ea07.fil", "20160701_010000_muos_ea07_kur.fil"
SP_HDR = sigproc.sigproc_header(7, 0.8718, -0.72452, "B0833-45", 57570 + SEC0 / 86400., 1, 8)
SAN = "-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the host program's sources (the Makefile's list) + tests/fake_pb/fake_pb.cpp under the sanitizers"""
    out = str(tmp_path_factory.mktemp("native_host") / "process_baseband")
    subprocess.run(["make", "-s", "-C", CSRC, "host-standin", "HOST_OUT=" + out, "HOST_CXXFLAGS=" + SAN], check=True)
    return out


@pytest.fixture(scope="module")
def samples():
    """[13 s][2 pols][NS] u8, never 0: zeros are what a missing frame leaves"""
    return np.random.default_rng(5).integers(1, 256, (13, 2, NS), dtype=np.uint8)


def _frames(samples, nsec, sec0=SEC0):
    """per second [2 * FPS][5032] frames in arrival order (frame 0 thread 0, frame 0 thread 1, frame 1 ...)"""
    return [vdif.frame_block(samples[s, 0], samples[s, 1], sec0 + s, 33, 7).reshape(2 * FPS, 5032).copy() for s in range(nsec)]


def _stream(frames):
    return b"".join(f.tobytes() for f in frames)


def _fold(x, trim=TRIM):
    """one pol of one second [NS] -> its SEG * trim output bytes: out[seg][j] = sum over i % trim == j of
    (2 * (i // trim) + 1) * x[seg][i], mod 256"""
    nrow = -(-SEG_SAMP // trim)
    pad = np.zeros((SEG, nrow * trim), np.uint32)
    pad[:, :SEG_SAMP] = x.reshape(SEG, SEG_SAMP)
    w = (2 * np.arange(nrow, dtype=np.uint32) + 1)[None, :, None]
    return ((pad.reshape(SEG, nrow, trim) * w).sum(axis=1) & 0xFF).astype(np.uint8).reshape(-1)


def _expected(kept, nout, sec0=SEC0):
    """the fold over vdif.deframe_block of the frames that were kept, seconds [0, nout): (raw payload, excised payload)"""
    raw, kur = [], []
    for s in range(nout):
        blk = np.zeros((2 * FPS, 5032), np.uint8)
        blk[:, 3] = 0x80                                    # (slots that no frame fills: invalid)
        blk[:len(kept[s])] = kept[s]
        d = vdif.deframe_block(blk.reshape(-1), sec0 + s, 0)
        raw.append(_fold(d[0]))
        kur.append(_fold(d[1]))
    return np.concatenate(raw).tobytes(), np.concatenate(kur).tobytes()


class FoldHandle(object):
    """Duck-typed PbHandle for process_baseband.py's run(): what fake_pb.cpp does, in numpy."""

    def __init__(self, nsets=2):
        self.trim, self.nsets, self.cur = TRIM, nsets, 0
        self.staged, self.done, self.unfetched = [None] * nsets, [None] * nsets, [False] * nsets

    def select_set(self, i):
        assert 0 <= i < self.nsets
        self.cur = i

    def reset_history(self, ant):
        pass

    def submit_vdif(self, ant, seg0, block, second=None, frame0=0):
        assert not self.unfetched[self.cur], "buffer set refilled before its output was fetched"
        self.staged[self.cur] = vdif.deframe_block(np.array(block, copy=True), second, frame0)

    def process(self, nseg, inject_now=0):
        self.done[self.cur], self.staged[self.cur], self.unfetched[self.cur] = self.staged[self.cur], None, True

    def fetch(self, ant, seg0, nseg, raw=True, kur=True, **kw):
        d = self.done[self.cur]
        assert d is not None and nseg == SEG
        self.unfetched[self.cur] = False
        return dict(raw=_fold(d[0]) if raw else None, kur=_fold(d[1]) if kur else None)

    def timers(self, reset=False):
        return {}

    def profile(self, on):
        pass

    def close(self):
        pass


def _write_dump(path, stream):
    hdr = vdif.ascii_header_format(vdif.writer_header(7, 0.8718, -0.72452, "B0833-45", 58000.0, "19A-331", 33, SEC0))
    with open(path, "wb") as f:
        f.write(hdr + stream)
    return str(path)


def _argv(d, dumps, extra=()):
    return ["-k", "40", "-K", "0", "-w", "2", "-b", "8", "-P", "1", "-r", "2", "-g", "0", "-p", "0", "--replay"] + list(dumps) + [
        "--datadir", str(d), "--logdir", str(d / "logs"), "--no-control", "--rows-per-seg", str(R),
        "--co-sink", str(d / "co.bin"), "--out-sink", str(d / "out.bin")] + list(extra)


def _native(exe, d, dumps, extra=(), status=0):
    """run the program; -> (files of the data directory by name, log text, the stand-in's call trace)"""
    env = dict(os.environ, FAKE_PB_TRACE=str(d / "trace.txt"))
    r = subprocess.run([exe] + _argv(d, dumps, extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert r.stderr == b"", r.stderr.decode()[-4000:]
    assert r.returncode == status
    return _outputs(d), _log(d), (d / "trace.txt").read_text().split("\n")[:-1]


def _outputs(d):
    return {p.name: p.read_bytes() for p in sorted(d.iterdir()) if p.suffix in (".fil", ".bin")}


def _log(d):
    return next((d / "logs").glob("*_process_*.log")).read_text()


def _python(d, dumps, extra=()):
    assert pbmod.run(pbmod.build_parser().parse_args(_argv(d, dumps, extra)), handle=FoldHandle()) == 0
    return _outputs(d)


def _same_outputs(a, b):
    """two hosts' files: .fil byte for byte; the sinks' payloads too, their headers but for the .fil file's directory"""
    assert sorted(a) == sorted(b)
    for n in a:
        x, y = a[n], b[n]
        if n.endswith(".bin"):
            hx, hy = vdif.ascii_header_parse(x[:4096]), vdif.ascii_header_parse(y[:4096])
            hx["SIGPROC_FILE"], hy["SIGPROC_FILE"] = os.path.basename(hx["SIGPROC_FILE"]), os.path.basename(hy["SIGPROC_FILE"])
            assert hx == hy and list(hx) == list(hy), n
            x, y = x[4096:], y[4096:]
        assert x == y, n


DROPS = {(1, 57), (2, 0), (2, 1), (5, 399)}     # mid-second; a second's very first frame, both threads; a last frame


def _dropped(samples):
    return [f[[i for i in range(2 * FPS) if (s, i) not in DROPS]] for s, f in enumerate(_frames(samples, 13))]


def _duplicated(samples):
    """5 s; second 1 carries frame slot 100 twice (the block fills one frame early, and the second's last frame then
    arrives where only a frame of the next second is expected); second 3 is whole and followed by its last frame again"""
    fr = _frames(samples, 5)
    fr[1] = np.concatenate([fr[1][:101], fr[1][100:]])
    fr[3] = np.concatenate([fr[3], fr[3][-1:]])
    return fr


def test_drops_12_s_out(tmp_path, exe, samples):
    kept = _dropped(samples)
    out, log, trace = _native(exe, tmp_path, [_write_dump(tmp_path / "obs.uw", _stream(kept))])
    raw, kur = _expected(kept, 12)                              # the last second is dropped
    assert sorted(out) == sorted([FIL, KUR, "co.bin", "out.bin"])
    assert out[FIL] == SP_HDR + raw
    assert out[KUR] == SP_HDR + kur
    ch = vdif.ascii_header_parse(out["co.bin"][:4096])
    assert ch["NCHAN"] == "4096" and ch["NBIT"] == "8" and ch["SIGPROC_FILE"].endswith("_muos_ea99_kur.fil")
    assert out["co.bin"][4096:] == kur
    assert len(out["out.bin"]) == 4096 + 12 * SEG * TRIM      # ten seconds in one write, then 1 s twice
    assert out["out.bin"][4096:] == kur
    # second k is queued before second k - 1 is collected, on alternating buffer sets
    assert trace[:9] == ["reset 0", "submit 0 3600 0", "process 0 10 0", "submit 1 3601 0", "process 1 10 0",
                         "fetch 0 0", "fetch 0 1", "submit 0 3602 0", "process 0 10 0"]
    assert [t for t in trace if t.startswith("submit")] == ["submit %d %d 0" % (k % 2, SEC0 + k) for k in range(12)]
    assert trace[-4:] == ["fetch 0 0", "fetch 0 1", "fetch 1 0", "fetch 1 1"]
    assert "Wrote 0.49 MB (0.09 s) to %s" % (tmp_path / FIL) in log     # (12 s of 8-row segments)


def test_major_skip(tmp_path, exe, samples):
    fr = _frames(samples, 3)
    late = vdif.frame_block(np.ones(NS, np.uint8), np.ones(NS, np.uint8), SEC0 + 5, 33, 7)
    out, log, _ = _native(exe, tmp_path, [_write_dump(tmp_path / "obs.uw", _stream(fr) + late.tobytes())], status=1)
    assert "ERR: Major data skip!  (3605 vs. 3602; thread = 0) Aborting this observation." in log
    assert out[FIL] == SP_HDR + _expected(fr, 2)[0]             # exactly the seconds queued before the skip
    assert out[KUR] == SP_HDR + _expected(fr, 2)[1]


def test_truncated_mid_frame(tmp_path, exe, samples):
    fr = _frames(samples, 3)
    out, log, _ = _native(exe, tmp_path, [_write_dump(tmp_path / "obs.uw", _stream(fr)[:-1000])])
    assert "Packet size=4032, expected 5032.  Aborting this observation." in log
    assert out[FIL] == SP_HDR + _expected(fr, 2)[0]             # the two complete seconds before the truncated one
    assert out[KUR] == SP_HDR + _expected(fr, 2)[1]


@pytest.mark.parametrize("case", ["drops", "duplicates"])
def test_hosts_agree(tmp_path, exe, samples, case):
    """the same stream through both hosts: same .fil files, same sink payloads.  The duplicate-frame expectation is
    the Python host's output, not a derivation: a frame that arrives twice mid-second costs the second its last frame
    (in both hosts), one that arrives again once the block is full costs nothing."""
    fr = _dropped(samples) if case == "drops" else _duplicated(samples)
    dump = _write_dump(tmp_path / "obs.uw", _stream(fr))
    for who in ("py", "cxx"):
        (tmp_path / who).mkdir()
    want = _python(tmp_path / "py", [dump])
    got, _, _ = _native(exe, tmp_path / "cxx", [dump])
    _same_outputs(want, got)
    assert len(got[FIL]) == len(SP_HDR) + (len(fr) - 1) * SEG * TRIM and sorted(got) == sorted([FIL, KUR, "co.bin", "out.bin"])
    if case == "duplicates":
        whole = _expected(_frames(samples, 5), 4)
        sec = SEG * TRIM
        for s in (0, 2, 3):                                     # the second followed by its own last frame is whole
            assert got[KUR][len(SP_HDR) + s * sec:][:sec] == whole[1][s * sec:][:sec], s


@pytest.mark.parametrize("rfi_mode", [0, 1])
def test_rfi_modes_0_and_1(tmp_path, exe, samples, rfi_mode):
    fr = _frames(samples, 13)
    out, _, trace = _native(exe, tmp_path, [_write_dump(tmp_path / "obs.uw", _stream(fr))], ["-r", str(rfi_mode)])
    stream = _expected(fr, 12)[rfi_mode]                        # -r 0: the raw stream everywhere; -r 1: the excised one
    fil = (FIL, KUR)[rfi_mode]
    assert sorted(out) == sorted([fil, "co.bin", "out.bin"])
    assert out[fil] == SP_HDR + stream
    assert out["co.bin"][4096:] == stream and out["out.bin"][4096:] == stream
    assert vdif.ascii_header_parse(out["co.bin"][:4096])["SIGPROC_FILE"].endswith(("_muos_ea99.fil", "_muos_ea99_kur.fil")[rfi_mode])
    assert vdif.ascii_header_parse(out["out.bin"][:4096])["SIGPROC_FILE"] == str(tmp_path / fil)
    assert set(t for t in trace if t.startswith("fetch")) == {"fetch 0 %d" % rfi_mode, "fetch 1 %d" % rfi_mode}


@pytest.mark.parametrize("single_pass", [False, True])
def test_two_observations_in_one_replay(tmp_path, exe, samples, single_pass):
    a, b = _frames(samples, 3), _frames(samples[3:], 3, sec0=SEC0 + 100)
    dumps = [_write_dump(tmp_path / "a.uw", _stream(a)), _write_dump(tmp_path / "b.uw", _stream(b))]
    out, log, trace = _native(exe, tmp_path, dumps, ["-s"] if single_pass else [])
    fil_b, kur_b = "20160701_010140_muos_ea07.fil", "20160701_010140_muos_ea07_kur.fil"
    want_a, want_b = _expected(a, 2), _expected(b, 2, sec0=SEC0 + 100)
    assert out[FIL] == SP_HDR + want_a[0] and out[KUR] == SP_HDR + want_a[1]

    def one(sec):
        return ["reset 0", "submit 0 %d 0" % sec, "process 0 10 0", "submit 1 %d 0" % (sec + 1), "process 1 10 0",
                "fetch 0 0", "fetch 0 1", "fetch 1 0", "fetch 1 1"]
    if single_pass:
        assert sorted(out) == sorted([FIL, KUR, "co.bin", "out.bin"])
        assert trace == one(SEC0) and log.count("Beginning new observation.") == 1
        return
    assert sorted(out) == sorted([FIL, KUR, fil_b, kur_b, "co.bin", "out.bin"])
    hdr_b = sigproc.sigproc_header(7, 0.8718, -0.72452, "B0833-45", 57570 + (SEC0 + 100) / 86400., 1, 8)
    assert out[fil_b] == hdr_b + want_b[0] and out[kur_b] == hdr_b + want_b[1]
    assert trace == one(SEC0) + one(SEC0 + 100)                 # the history is reset between the observations
    co = out["co.bin"]                                          # header, 2 s, header, 2 s
    assert len(co) == 2 * (4096 + 2 * SEG * TRIM)
    assert co[4096:][:2 * SEG * TRIM] == want_a[1] and co[2 * 4096 + 2 * SEG * TRIM:] == want_b[1]
    assert vdif.ascii_header_parse(co[4096 + 2 * SEG * TRIM:][:4096])["SIGPROC_FILE"].endswith("20160701_010140_muos_ea99_kur.fil")
    assert log.count("Beginning new observation.") == 2 and "Input ring closed.  Exiting." in log


def test_cmd_quit(tmp_path, exe, samples):
    """'Q' on the control socket (--control-port) while the stream arrives through a FIFO: status 0, the reference's log
    line, everything queued written.  The command is looked at once per second of data, when a second closes.  The
    writer's first 2.5 s have passed through the FIFO (64 KiB of them at most still in it) before the command is sent,
    so the program is reading second 2 by then, seconds 0 and 1 are queued, and the command is seen when second 2
    closes: exactly two seconds are written."""
    fr = _frames(samples, 6)
    dump = open(_write_dump(tmp_path / "obs.uw", _stream(fr)), "rb").read()
    fifo = str(tmp_path / "ring.fifo")
    os.mkfifo(fifo)
    probe = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    probe.bind(("127.0.0.1", 0))
    port = probe.getsockname()[1]
    probe.close()
    argv = [a for a in _argv(tmp_path, [fifo]) if a != "--no-control"] + ["--control-port", str(port)]
    proc = subprocess.Popen([exe] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE)

    def feed():
        cut = 4096 + 5 * FPS * 5032
        try:
            with open(fifo, "wb") as w:
                w.write(dump[:cut])
                w.flush()
                socket.socket(socket.AF_INET, socket.SOCK_DGRAM).sendto(b"xQ", ("127.0.0.1", port))
                w.write(dump[cut:])
        except BrokenPipeError:
            pass
    threading.Thread(target=feed, daemon=True).start()
    try:
        _, err = proc.communicate(timeout=120)
    finally:
        if proc.poll() is None:
            proc.kill()
    assert err == b"", err.decode()[-4000:]
    assert proc.returncode == 0
    assert "Received CMD_QUIT, indicating data taking is ceasing.  Exiting." in _log(tmp_path)
    out = _outputs(tmp_path)
    assert out[FIL] == SP_HDR + _expected(fr, 2)[0] and out[KUR] == SP_HDR + _expected(fr, 2)[1]
    assert out["co.bin"][4096:] == _expected(fr, 2)[1]
