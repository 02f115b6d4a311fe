"""bench.py's plain run and its output dump, without a GPU: a plain run times exactly --steps steps (one region) and
leaves everything else to --full; --dump-outputs writes float32 .npy files, at most 64 MB in all, the same sample
of a larger output in every run."""
import os

import numpy as np


def _bench():
    import bench
    return bench


def test_plain_run_times_one_region_and_full_keeps_five():
    b = _bench()
    plain = b.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False and plain.regions == 1 and plain.dump_outputs is None
    full = b.parse_args(["--steps", "20", "--full"])
    assert full.full is True and full.regions == 5
    assert b.parse_args(["--coadd-selftest"]).regions == 5
    assert b.parse_args(["--regions", "3"]).regions == 3 and b.parse_args(["--full", "--regions", "2"]).regions == 2
    assert b.parse_args(["--dump-outputs", "out"]).dump_outputs == "out"


def test_write_outputs_float32_exact_when_it_fits(tmp_path):
    b = _bench()
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, (10, 524288), dtype=np.uint8)          # the headline step's size: 10 segments per stream
    kur = rng.integers(0, 256, (10, 524288), dtype=np.uint8)
    w = b.write_outputs(str(tmp_path), {"filterbank_raw_ant0": raw, "filterbank_kur_ant0": kur})
    assert w == {"filterbank_raw_ant0": ((10, 524288), False), "filterbank_kur_ant0": ((10, 524288), False)}
    for name, a in (("filterbank_raw_ant0", raw), ("filterbank_kur_ant0", kur)):
        got = np.load(os.path.join(str(tmp_path), name + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, a)
    assert sum(os.path.getsize(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))) <= 64_000_000


def test_write_outputs_samples_a_larger_output_the_same_way_every_time(tmp_path):
    b = _bench()
    # two antennas' streams (84 MB as float32): every file holds a sample, and each its own array's values
    arrays = {"filterbank_%s_ant%d" % (s, a): np.full((10, 524288), 7 * a + (s == "kur"), np.uint8)
              for a in range(2) for s in ("raw", "kur")}
    d1, d2 = tmp_path / "a", tmp_path / "b"
    w1 = b.write_outputs(str(d1), arrays)
    w2 = b.write_outputs(str(d2), arrays)
    assert w1 == w2 and all(sampled for _, sampled in w1.values())
    total = sum(os.path.getsize(os.path.join(str(d1), f)) for f in os.listdir(str(d1)))
    assert 60_000_000 < total <= 64_000_000
    for name in arrays:
        x, y = np.load(os.path.join(str(d1), name + ".npy")), np.load(os.path.join(str(d2), name + ".npy"))
        assert x.dtype == np.float32 and np.array_equal(x, y)
        assert set(np.unique(x)) <= set(np.unique(arrays[name]).astype(np.float32))
