"""Coherence output on the CPU: the ABI field, what pb_create refuses, both hosts' --coherence option and headers,
and the new kernels' compiled resources (no scratch)."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import synth  # noqa: F401  (tests/golden on the path, as the other host tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vlite-fast_amd", "csrc")
EXE = os.path.join(CSRC, "process_baseband")
lp = importlib.import_module("vlite-fast_amd.libpb")
vdif = importlib.import_module("vlite-fast_amd.vdif")
sigproc = importlib.import_module("vlite-fast_amd.sigproc")
pbmod = importlib.import_module("vlite-fast_amd.process_baseband")


def test_config_field_defaults_to_off():
    L = lp.load()
    cfg = lp.PbConfig()
    L.pb_config_default(C.byref(cfg))
    assert cfg.coherence == 0
    assert cfg.struct_size == C.sizeof(lp.PbConfig)
    assert lp.PbConfig._fields_[-1][0] == "coherence"


def test_config_of_the_previous_size_is_accepted_without_coherence():
    """a caller built before `coherence` was appended passes the shorter struct: pb_create takes it and reads nothing
    past it (here the bytes past it say coherence = 1 with npol = 1, which a full-size struct has refused)"""
    L = lp.load()
    cfg = lp.PbConfig()
    L.pb_config_default(C.byref(cfg))
    cfg.npol, cfg.rows_per_seg, cfg.max_seg, cfg.coherence = 1, 8, 1, 1
    h = C.c_void_p()
    assert L.pb_create(C.byref(cfg), C.byref(h)) == -22
    cfg.struct_size = lp.PbConfig.coherence.offset
    rc = L.pb_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        L.pb_destroy(h)
    assert rc != -22, L.pb_last_error(None).decode()      # 0 on a GPU box; without a device, "no HIP device"
    cfg.struct_size = lp.PbConfig.coherence.offset - 4
    assert L.pb_create(C.byref(cfg), C.byref(h)) == -22


@pytest.mark.parametrize("kw", [dict(npol=1), dict(npol=2, taps=4), dict(npol=2, fft_backend=lp.FFT_HIPFFT),
                                dict(npol=2, debug_keep=True)])
def test_unsupported_combinations_are_refused(kw):
    # refused by the argument checks, before any device is looked for
    with pytest.raises(ValueError):
        lp.PbHandle(coherence=True, rows_per_seg=8, max_seg=1, **kw)


def test_python_host_option():
    p = pbmod.build_parser()
    a = p.parse_args("-P 2 --coherence".split())
    pbmod.validate(a)
    assert a.coherence and pbmod.out_npol(a) == 4
    assert pbmod.out_npol(p.parse_args("-P 2".split())) == 2
    for bad in ("--coherence", "-P 1 --coherence", "-P 4", "-P 4 --coherence"):
        with pytest.raises(SystemExit):
            pbmod.validate(p.parse_args(bad.split()))


def _dump_headers(tmp_path, extra):
    if not os.access(EXE, os.X_OK):
        subprocess.run(["make", "-s", "-C", CSRC, "process_baseband"], check=False)
    inhdr = vdif.writer_header(7, 0.8718, -0.72452, "B0833-45", 58000.25, "19A-331", 33, 3600)
    frame = np.zeros(vdif.VD_FRM, np.uint8)
    frame[:32] = vdif.pack_header(3600, 33, 0, 7, 0).view(np.uint8)
    dump = tmp_path / "one.uw"
    dump.write_bytes(vdif.ascii_header_format(inhdr) + frame.tobytes())
    r = subprocess.run([EXE, "-b", "8", "-r", "2", "--replay", str(dump), "--datadir", "/data/x", "--logdir",
                        str(tmp_path), "--no-control", "--rows-per-seg", "8", "--dump-headers"] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return r, inhdr, frame


def test_native_host_option_and_headers(tmp_path):
    for bad in (["--coherence"], ["-P", "1", "--coherence"], ["-P", "4", "--coherence"]):
        r, _, _ = _dump_headers(tmp_path, bad)
        assert r.returncode == 1, bad
    r, inhdr, frame = _dump_headers(tmp_path, ["-P", "2", "--coherence"])
    assert r.returncode == 0, r.stderr
    out = dict(l.split(" ", 1) for l in r.stdout.decode().splitlines())
    vh = vdif.unpack_header(frame.tobytes())
    fps = 8 * 10 * 12500 // 5000
    want_sp = sigproc.sigproc_header(7, 0.8718, -0.72452, "B0833-45", vdif.frame_dmjd(vh, fps), 4, 8)
    assert bytes.fromhex(out["sigproc"].split()[1]) == want_sp
    assert b"nifs" in want_sp and want_sp[want_sp.index(b"nifs") + 4:want_sp.index(b"nifs") + 8] == np.int32(4).tobytes()
    # the psrdada headers of rings -K and -C: NPOL 4, and the bytes the Python host's encoder writes
    pin = vdif.ascii_header_parse(vdif.ascii_header_format(inhdr))
    t_unix = vdif.vdif_to_unixepoch(vh)
    fb, fbk, co, cok = sigproc.fb_names(t_unix, 7, "/data/x")
    assert out["files"].split() == [fb, fbk, co, cok]
    for key, f in (("out", fbk), ("co", cok)):
        n, hx = out[key].split()
        hx = bytes.fromhex(hx)
        assert re.search(rb"(^|\n)NPOL\s+4\s*\n", hx), key
        want = vdif.ascii_header_format(sigproc.psrdada_out_header(pin, vh, 4, 8, f, t_unix, vdif.frame_mjd(vh),
                                                                   vdif.frame_mjd_sec(vh)))
        assert int(n) == 4096 and hx == want, key


FLAGS = ("-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt "
         "-fno-gpu-flush-denormals-to-zero -I../../include -I. -w --cuda-device-only -S -o -").split()


def _usage(src):
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [src], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out, cur = {}, None
    for line in r.stdout.decode().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", line)
        if m and cur:
            out.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    return out


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_coherence_kernels_use_no_scratch():
    u = _usage("k_channelize.hip")
    chans = {k: v for k, v in u.items() if "k_coh_chan" in k}
    assert len(chans) == 2, sorted(u)
    for k, v in chans.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 2 and v["LDSByteSize"] <= 163840 // 2, (k, v)
    d = _usage("k_detect_coh.hip")
    det = {k: v for k, v in d.items() if "k_detect_coh" in k}
    assert len(det) == 18, sorted(d)
    assert all(v["ScratchSize"] == 0 for v in det.values()), det
