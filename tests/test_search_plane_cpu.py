"""The fp32 entry of the streaming search without a GPU: the NumPy restatement of its quantiser (tests/search_plane_ref.py)
against the oracle's sel_and_dig_8b, the entry point's answer to a missing handle, and process_baseband's --search flags
(parsed by the search's own parser)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import search_plane_ref as PR
from helpers import CHANMIN, NCHAN, NCHANOUT, libpb

search = importlib.import_module("vlite-fast_amd.search")
host = importlib.import_module("vlite-fast_amd.process_baseband")


def oracle_codes(oracle, values):
    """values (float32, any length) through orc_sel_and_dig_8b at the oracle's [ntime][6251] layout: padded to whole rows
    of the 4096 output channels; the codes of the values themselves"""
    v = np.asarray(values, np.float32)
    ntime = -(-v.size // NCHANOUT)
    plane = np.zeros((ntime, NCHAN), np.float32)
    pad = np.zeros(ntime * NCHANOUT, np.float32)
    pad[:v.size] = v
    plane[:, CHANMIN:CHANMIN + NCHANOUT] = pad.reshape(ntime, NCHANOUT)
    return oracle.sel_and_dig(plane, 8 * ntime, npol=1, nbit=8)[:v.size]


def test_restatement_equals_the_oracle_on_noise(oracle):
    x = np.random.default_rng(11).normal(0, 1, 16 * NCHANOUT).astype(np.float32)
    q = PR.quantise8(x)
    assert np.array_equal(q, oracle_codes(oracle, x))
    assert q.min() < 40 and q.max() > 215 and len(np.unique(q)) > 150       # the codes are spread over the range
    # a scale is one binary32 product in front of the same rule
    for scale in (np.float32(1 / np.sqrt(2)), np.float32(1 / np.sqrt(3))):
        assert np.array_equal(PR.quantise8(x, scale), oracle_codes(oracle, x * scale))


def test_restatement_equals_the_oracle_at_every_cell_edge(oracle):
    e = PR.edges()
    assert e.size == 5 * 257 and e.dtype == np.float32
    q = PR.quantise8(e)
    assert np.array_equal(q, oracle_codes(oracle, e))
    # the edges are edges: around edge k only the codes k - 1 and k occur (at the ends: the clamped one), and over all
    # edges both sides are met
    per_edge = q.reshape(5, 257).astype(int)
    k = np.arange(257)
    assert ((per_edge == np.clip(k - 1, 0, 255)) | (per_edge == np.clip(k, 0, 255))).all()
    assert (per_edge == k - 1).any() and (per_edge[:, :256] == k[:256]).any()


def test_restatement_equals_the_oracle_on_zeros_and_infinities(oracle):
    q = PR.quantise8(PR.SPECIAL)
    assert np.array_equal(q, oracle_codes(oracle, PR.SPECIAL))
    assert q.tolist() == [127, 127, 255, 0, 255, 0]


def test_nan_gives_zero():
    # (the oracle's C cast of a NaN is undefined and is not consulted)
    x = np.array([np.nan, -np.nan, 0.5, np.nan], np.float32)
    assert PR.quantise8(x).tolist() == [0, 0, PR.quantise8(np.float32(0.5)), 0]
    assert PR.quantise8(x, np.float32(0.5))[0] == 0
    v = PR.test_values(5, 4096)
    assert np.isnan(v).any() and np.isinf(v).any() and (PR.quantise8(v)[np.isnan(v)] == 0).all()


def test_no_handle_is_refused_with_a_message():
    L = libpb().load()
    fill = C.c_int(7)
    plane = (C.c_float * 8)()
    assert L.pb_search_push_f32(None, plane, 0, 1, C.c_float(1.0), C.byref(fill)) == -22        # PB_EINVAL
    assert b"pb_search_push_f32" in L.pb_search_last_error(None) and b"no search handle" in L.pb_search_last_error(None)
    assert fill.value == 7


# ---------------------------------------------------------------------------------------------------------------------
# the host's flags

FLAGS = "-dm 0 6 -dm_step 2 -boxcar_max 4 -nsamps_gulp 128 -detect_thresh 1 -zap_chans 0 190 -zap_chans 3900 4096 -output_dir 'a b'"


def host_args(*argv):
    return host.build_parser().parse_args(list(argv))


def test_search_absent_gives_none():
    a = host_args("-b", "2")
    assert a.search is None and a.search_input == "plane"
    host.validate(a)
    assert host.search_flags(a) is None


def test_the_flag_string_goes_through_the_search_parser():
    a = host_args("-b", "2", "--search", FLAGS, "--search-input", "codes")
    host.validate(a)
    got = host.search_flags(a)
    want = search.parse_args(["-f", "x.fil", "-dm", "0", "6", "-dm_step", "2", "-boxcar_max", "4", "-nsamps_gulp", "128",
                              "-detect_thresh", "1", "-zap_chans", "0", "190", "-zap_chans", "3900", "4096", "-output_dir", "a b"])
    d = dict(vars(want))
    assert d.pop("fil") == "x.fil" and d.pop("stream_chunk") == 0
    assert vars(got) == d
    assert got.zap_chans == [[0, 190], [3900, 4096]] and got.output_dir == "a b" and a.search_input == "codes"
    # the checks between flags are the search's too
    assert host.search_flags(host_args("--search", "-detect_thresh 7")).cutout_thresh == 7.0
    # an empty string: the search's defaults
    e = host.search_flags(host_args("--search", ""))
    assert e.nsamps_gulp == search.HEIMDALL_GULP and e.dm == list(search.HEIMDALL_DM)


@pytest.mark.parametrize("argv", [("-P", "2", "--search", FLAGS),
                                  ("-P", "2", "--coherence", "--search", FLAGS),
                                  ("--search", "-no_such_flag 1"),
                                  ("--search", "-f some.fil"),
                                  ("--search", "-stream_chunk 80"),
                                  ("--search", "-cutouts"),                  # (needs -output_dir: the search's own check)
                                  ("--search", FLAGS, "--search-input", "floats")])
def test_what_the_host_refuses(argv, capsys):
    with pytest.raises(SystemExit) as e:
        host.validate(host_args(*argv))
    assert e.value.code not in (0, None)
    if "-P" in argv:
        assert "--search takes one" in str(e.value.code)
    capsys.readouterr()


def test_the_defaults_of_search_main_are_unchanged():
    a = vars(search.parse_args(["-f", "x.fil"]))
    assert a == dict(fil="x.fil", dm=[2.0, 1000.0], dm_tol=1.25, dm_step=0.0, boxcar_max=64, nsamps_gulp=30720, zap_chans=None,
                     detect_thresh=6.0, baseline_length=2.0, beam=1, coincidencer=None, gpu_id=0, rfi_clean=False,
                     rfi_tol=5.0, rfi_no_narrow=False, rfi_no_broad=False, output_dir=None, cutouts=False, cutout_thresh=6.0,
                     cutout_max=32, refine=False, refine_thresh=6.0, refine_max=32, giants=False, cand_sep_time=3,
                     cand_sep_dm=200, cand_sep_filter=3, max_giants=1 << 18, stream_chunk=0)
    assert list(a) == ["fil", "dm", "dm_tol", "dm_step", "boxcar_max", "nsamps_gulp", "zap_chans", "detect_thresh",
                       "baseline_length", "beam", "coincidencer", "gpu_id", "rfi_clean", "rfi_tol", "rfi_no_narrow",
                       "rfi_no_broad", "output_dir", "cutouts", "cutout_thresh", "cutout_max", "refine", "refine_thresh",
                       "refine_max", "giants", "cand_sep_time", "cand_sep_dm", "cand_sep_filter", "max_giants", "stream_chunk"]
    with pytest.raises(SystemExit):
        search.parse_args([])                                       # -f is still required
