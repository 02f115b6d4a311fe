"""Dedispersion + boxcar search on a filterbank block, and heimdall-style candidate lines.

Stands where the external `heimdall_stream` stands in the reference's chain
(/root/reference/scripts/start_heimdall_single_antenna:21; candidate line columns
`S/N, peak_idx, peak_time, tfilt, dmi, dm, ngiant, i0, i1` as parsed by src/candidate.py:8-18).
The GPU work is libpb_hip.so's pb_search_* (csrc/search_*.hip); this module only drives it and
groups the above-threshold samples into candidates on the host.  heimdall is third-party and not in
the image: its DM spacing, baseline removal and giant merging are not reproduced -- parity with its
candidate list is unpinned.

This module is the entry (`python -m vlite-fast_amd.search`) and the public name of all of it; it holds the command line,
the file writers, open_search and main.  The rest lives in searcher.py (Searcher: the ctypes surface), candidates.py (the
grouping on the host, the candidate line and the TCP leg) and gulp.py (GulpSearch) and is imported here by name.
"""
import argparse

import numpy as np

from . import sigproc as sig
from .candidates import (PERIODIC_BINS, candidate_line, candidates_from_giants, candidates_from_peaks,
                         candidates_from_periodic, candidates_from_subbands, find_candidates, group_points, harmonic_ratio,
                         overlap, periodic_octaves, subband_list)
from .gulp import GulpSearch, gulp_cuts
from .searcher import (CUTOUT_KEYS, FCH1, FOFF, HEIMDALL_BOXCAR_MAX, HEIMDALL_DM, HEIMDALL_GULP, HEIMDALL_ZAP,
                       POL_KEYS, TSAMP, Searcher, dedisp_dm_list)


def arg_parser(with_file=True):
    """the command line of main(): heimdall's flag names.  with_file=False: the flags that a host which feeds the search
    itself accepts (process_baseband --search) -- the same ones less -f and -stream_chunk."""
    ap = argparse.ArgumentParser(prog="search" if with_file else "--search", prefix_chars="-",
                                 epilog="with -f also: -pol [-pol_thresh S] [-pol_max N] [-rm LO HI] [-rm_step D] [-pol_off L G]: "
                                        "a nifs 4 filterbank (AA, BB, CR, CI); Stokes spectra and RM synthesis of the strongest "
                                        "candidates (pol_parser).  Also: -subbands N [-subband_thresh S] [-subband_send]: search N base "
                                        "sub-bands (2, 4, 8 or 16) and their staggered dyadic runs for band-limited bursts "
                                        "(subband_parser).  Also: -periodic P_LO P_HI [-periodic_bins B] [-periodic_thresh S] "
                                        "[-periodic_max N]: fold every trial DM's series at the periods P_LO .. P_HI seconds "
                                        "(periodic_parser)")
    if with_file:
        ap.add_argument("-f", dest="fil", required=True)
    ap.add_argument("-dm", nargs=2, type=float, default=list(HEIMDALL_DM))
    ap.add_argument("-dm_tol", type=float, default=1.25)
    ap.add_argument("-dm_step", type=float, default=0.0, help="> 0: linear grid instead of the tolerance-spaced list")
    ap.add_argument("-boxcar_max", type=int, default=HEIMDALL_BOXCAR_MAX)
    ap.add_argument("-nsamps_gulp", type=int, default=HEIMDALL_GULP)
    ap.add_argument("-zap_chans", nargs=2, type=int, action="append", default=None)
    ap.add_argument("-detect_thresh", type=float, default=6.0)
    ap.add_argument("-baseline_length", type=float, default=2.0, help="seconds")
    ap.add_argument("-beam", type=int, default=1)
    ap.add_argument("-coincidencer", default=None)
    ap.add_argument("-gpu_id", type=int, default=0)
    ap.add_argument("-rfi_clean", action="store_true", help="clean each gulp of RFI before dedispersion (narrow + broad)")
    ap.add_argument("-rfi_tol", type=float, default=5.0, help="with -rfi_clean: the cleaning's threshold")
    ap.add_argument("-rfi_no_narrow", action="store_true", help="with -rfi_clean: no per-channel outlier pass")
    ap.add_argument("-rfi_no_broad", action="store_true", help="with -rfi_clean: no zero-DM impulse pass")
    ap.add_argument("-output_dir", default=None, help="write each gulp's candidate lines to <UTC>_<beam>.cand there")
    ap.add_argument("-cutouts", action="store_true", help="with -output_dir: a .cutouts.npz beside each .cand file")
    ap.add_argument("-cutout_thresh", type=float, default=None, help="with -cutouts: lowest S/N cut out (default: -detect_thresh)")
    ap.add_argument("-cutout_max", type=int, default=32, help="with -cutouts: most cutouts per gulp")
    ap.add_argument("-refine", action="store_true", help="refine DM, width and S/N of the strongest candidates; with -output_dir a .refined file beside each .cand")
    ap.add_argument("-refine_thresh", type=float, default=None, help="with -refine: lowest S/N refined (default: -detect_thresh)")
    ap.add_argument("-refine_max", type=int, default=32, help="with -refine: most refinements per gulp")
    ap.add_argument("-giants", action="store_true", help="candidates from giants and clusters of giants made on the GPU instead of the host's grouping of points")
    ap.add_argument("-cand_sep_time", type=int, default=3, help="with -giants: samples between hot samples of one giant, and between linked giants (1..64)")
    ap.add_argument("-cand_sep_dm", type=int, default=200, help="with -giants: trial DMs between linked giants")
    ap.add_argument("-cand_sep_filter", type=int, default=3, help="with -giants: log2 boxcar widths between linked giants")
    ap.add_argument("-max_giants", type=int, default=1 << 18, help="with -giants: a gulp with more giants is given up")
    if with_file:
        ap.add_argument("-stream_chunk", type=int, default=0, help="> 0: read the file in pieces of this many samples and gather each gulp on the GPU; 8-, 4- and 2-bit files")
    return ap


def pol_parser():
    """the flags of -pol, parsed apart from arg_parser()'s: a command line without -pol gives the namespace it always gave"""
    ap = argparse.ArgumentParser(prog="search", prefix_chars="-", add_help=False, allow_abbrev=False)
    ap.add_argument("-pol", action="store_true", help="a nifs 4 filterbank (AA, BB, CR, CI): search total intensity; Stokes spectra and RM synthesis of the strongest candidates; with -output_dir a .pol and a .pol.npz file beside each .cand")
    ap.add_argument("-pol_thresh", type=float, default=None, help="with -pol: lowest S/N analysed (default: -detect_thresh)")
    ap.add_argument("-pol_max", type=int, default=32, help="with -pol: most candidates analysed per gulp")
    ap.add_argument("-rm", nargs=2, type=float, default=[-2000.0, 2000.0], help="with -pol: first and last trial RM in rad/m^2")
    ap.add_argument("-rm_step", type=float, default=2.0, help="with -pol: step of the trial RMs")
    ap.add_argument("-pol_off", nargs=2, type=int, default=[64, 8], help="with -pol: length of each off-pulse window and its guard from the on window, in samples")
    return ap


def subband_parser():
    """the flags of -subbands, parsed apart from arg_parser()'s like -pol's: a command line without them gives the namespace
    it always gave"""
    ap = argparse.ArgumentParser(prog="search", prefix_chars="-", add_help=False, allow_abbrev=False)
    ap.add_argument("-subbands", type=int, default=0, help="search N base sub-bands (2, 4, 8 or 16) and their staggered dyadic runs for band-limited bursts; 0: off; with -output_dir a .subband file beside each .cand")
    ap.add_argument("-subband_thresh", type=float, default=None, help="with -subbands: lowest sub-band S/N reported (default: -detect_thresh)")
    ap.add_argument("-subband_send", action="store_true", help="with -subbands: send the sub-band candidates to the coincidencer too")
    return ap


def periodic_parser():
    """the flags of -periodic, parsed apart from arg_parser()'s like -pol's: a command line without them gives the namespace
    it always gave"""
    ap = argparse.ArgumentParser(prog="search", prefix_chars="-", add_help=False, allow_abbrev=False)
    ap.add_argument("-periodic", nargs=2, type=float, default=None, metavar=("P_LO", "P_HI"), help="search every trial DM's series for periodic pulses with periods P_LO .. P_HI seconds by folding (FFA); with -output_dir a .periodic file beside each .cand")
    ap.add_argument("-periodic_bins", type=int, default=None, help="with -periodic: profiles of B .. 2B - 1 bins, B 32, 64 or 128 (default 64)")
    ap.add_argument("-periodic_thresh", type=float, default=None, help="with -periodic: lowest folded S/N reported (default 8.0)")
    ap.add_argument("-periodic_max", type=int, default=None, help="with -periodic: most periodicity candidates per gulp (default 64)")
    return ap


def rfichan_parser():
    """the flags of -rfi_chan, parsed apart from arg_parser()'s like -pol's: a command line without them gives the namespace
    it always gave"""
    ap = argparse.ArgumentParser(prog="search", prefix_chars="-", add_help=False, allow_abbrev=False)
    ap.add_argument("-rfi_chan", action="store_true", help="flag the channels that are noisy for a whole gulp and fill them with their mean before the rest of the cleaning; with -output_dir a .chans file beside each .cand")
    ap.add_argument("-rfi_chan_tol", type=float, default=None, help="with -rfi_chan: the outlier threshold in robust sigmas (default 4)")
    ap.add_argument("-rfi_chan_radius", type=int, default=None, help="with -rfi_chan: the largest lag in unzapped channels (default 0: a tenth of them)")
    return ap


def parse_flags(flags):
    """process_baseband's --search "<flags>": the string split as a shell would and parsed by the search's own parser
    (arg_parser(with_file=False) and parse_args' checks); an unknown flag, -f, -stream_chunk or -pol ends in SystemExit; -subbands,
    -periodic and -rfi_chan and their flags are taken"""
    import shlex
    return parse_args(shlex.split(flags), with_file=False)


def _rfichan_checks(ap, a, ca, argv, with_file):
    if (ca.rfi_chan_tol is not None or ca.rfi_chan_radius is not None) and not ca.rfi_chan:
        ap.error("-rfi_chan_tol, -rfi_chan_radius: only with -rfi_chan")
    if ca.rfi_chan:
        if ca.rfi_chan_tol is None:
            ca.rfi_chan_tol = 4.0
        if ca.rfi_chan_radius is None:
            ca.rfi_chan_radius = 0
        if not (ca.rfi_chan_tol > 0 and np.isfinite(ca.rfi_chan_tol)) or ca.rfi_chan_radius < 0:
            ap.error("-rfi_chan_tol must be > 0 and finite, -rfi_chan_radius >= 0")


def _subband_checks(ap, a, sa, argv, with_file):
    if sa.subbands not in (0, 2, 4, 8, 16):
        ap.error("-subbands must be 0, 2, 4, 8 or 16")
    if (sa.subband_thresh is not None or sa.subband_send) and not sa.subbands:
        ap.error("-subband_thresh, -subband_send: only with -subbands")
    if sa.subbands and sa.subband_thresh is None:
        sa.subband_thresh = a.detect_thresh


def _periodic_checks(ap, a, pa, argv, with_file):
    alone = [f for f in ("-periodic_bins", "-periodic_thresh", "-periodic_max") if getattr(pa, f[1:]) is not None]
    if alone and pa.periodic is None:
        ap.error("%s: only with -periodic" % ", ".join(alone))
    if pa.periodic is not None:
        if "-pol" in argv:
            ap.error("-periodic is not combined with -pol")
        for k, v in (("periodic_bins", 64), ("periodic_thresh", 8.0), ("periodic_max", 64)):
            if getattr(pa, k) is None:
                setattr(pa, k, v)
        if pa.periodic_bins not in PERIODIC_BINS:
            ap.error("-periodic_bins must be 32, 64 or 128")
        if not (0 < pa.periodic[0] <= pa.periodic[1]) or not np.isfinite(pa.periodic[1]):
            ap.error("-periodic P_LO P_HI: need 0 < P_LO <= P_HI, in seconds")
        if pa.periodic_thresh != pa.periodic_thresh or pa.periodic_max < 1:
            ap.error("-periodic_thresh must be a number, -periodic_max >= 1")


def _pol_checks(ap, a, pa, argv, with_file):
    alone = [f for f in ("-pol_thresh", "-pol_max", "-rm", "-rm_step", "-pol_off") if f in argv]
    if alone and not pa.pol:
        ap.error("%s: only with -pol" % ", ".join(alone))
    if pa.pol:
        if getattr(a, "subbands", 0):
            ap.error("-subbands is not combined with -pol")
        if not with_file:
            ap.error("-pol reads a nifs 4 file: a host that feeds the search itself feeds it one IF")
        if a.stream_chunk:
            ap.error("-pol reads whole gulps: not with -stream_chunk")
        if pa.pol_thresh is None:
            pa.pol_thresh = a.detect_thresh
        if pa.pol_max < 1:
            ap.error("-pol_max must be >= 1")
        if not pa.rm_step > 0 or pa.rm[1] < pa.rm[0] or rm_trials(pa.rm[0], pa.rm[1], pa.rm_step) > 8192:
            ap.error("-rm LO HI with LO <= HI and -rm_step > 0, at most 8192 trials")
        if not (1 <= pa.pol_off[0] <= 1024 and 0 <= pa.pol_off[1] <= 1024):
            ap.error("-pol_off L G: L in 1..1024, G in 0..1024")


# the flags parsed apart from arg_parser()'s: (their parser, the flag that switches them on, the checks between them)
_SIDE_FLAGS = ((rfichan_parser, "rfi_chan", _rfichan_checks), (subband_parser, "subbands", _subband_checks),
              (periodic_parser, "periodic", _periodic_checks), (pol_parser, "pol", _pol_checks))


def parse_args(argv=None, with_file=True):
    """arg_parser() plus the checks between flags"""
    import sys
    ap = arg_parser(with_file)
    argv = sys.argv[1:] if argv is None else list(argv)
    side, rest = [], argv
    for parser, _, _ in _SIDE_FLAGS:
        ns, rest = parser().parse_known_args(rest)
        side.append(ns)
    a = ap.parse_args(rest)
    if a.cutouts and not a.output_dir:
        ap.error("-cutouts needs -output_dir")
    if a.cutout_max < 1:
        ap.error("-cutout_max must be >= 1")
    if a.cutout_thresh is None:
        a.cutout_thresh = a.detect_thresh
    if a.refine_max < 1:
        ap.error("-refine_max must be >= 1")
    if a.refine_thresh is None:
        a.refine_thresh = a.detect_thresh
    if not 1 <= a.cand_sep_time <= 64:
        ap.error("-cand_sep_time must be in 1..64")
    if a.cand_sep_dm < 0 or a.cand_sep_filter < 0:
        ap.error("-cand_sep_dm and -cand_sep_filter must be >= 0")
    if not 1 <= a.max_giants <= 1 << 22:
        ap.error("-max_giants must be in 1..4194304")
    if with_file and a.stream_chunk < 0:
        ap.error("-stream_chunk must be >= 0")
    for (_, switch, checks), ns in zip(_SIDE_FLAGS, side):
        checks(ap, a, ns, argv, with_file)
        if getattr(ns, switch):                     # (only when switched on: without it the namespace is what it always was)
            for k, v in vars(ns).items():
                setattr(a, k, v)
    return a


def rm_trials(lo, hi, step):
    """how many trial RMs lo, lo + step, .. reach hi (a step that falls 1e-9 of itself short of hi still counts)"""
    return int(np.floor((hi - lo) / step + 1e-9)) + 1


def pol_numbers(p):
    """a candidate's "pol" entry -> (RM of the synthesis peak, L/I, V/I, position angle at lambda0 in degrees);
    uncalibrated (include/pb_hip.h, pb_search_set_pol), NaN where no channel had both windows"""
    k, sm = int(p["kbest"]), p["summary"]
    if k < 0:
        return (float("nan"),) * 4
    with np.errstate(divide="ignore", invalid="ignore"):
        return (float(sm[5]), float(sm[4] / sm[2]), float(sm[3] / sm[2]),
                float(np.degrees(0.5 * np.arctan2(p["F"][k, 1], p["F"][k, 0]))))


def pol_line(c):
    """a candidate's line followed by the RM of its synthesis peak, L/I, V/I and the position angle in degrees"""
    return "%s\t%.4f\t%.4f\t%.4f\t%.3f" % ((candidate_line(c),) + pol_numbers(c["pol"]))


def write_pol(path, cands, tsamp):
    """The polarised candidates of one gulp (those that carry a "pol" entry): path gets one pol_line each, path + ".npz"
    F, rms, on, non, off, noff, summary, kbest, freqs (pft, pft_hits, tscr of the first of them that were cut out too) and the candidates'
    nine columns as `cands` [n][9].  Returns how many were written (0: no files)."""
    cc = [c for c in cands if "pol" in c]
    if not cc:
        return 0
    with open(path, "w") as f:
        f.write("".join(pol_line(c) + "\n" for c in cc))
    d = {k: np.stack([c["pol"][k] for c in cc]) for k in POL_KEYS}
    d["rms"], d["freqs"] = cc[0]["pol"]["rms"], cc[0]["pol"]["freqs"]
    cp = [c for c in cc if "pft" in c["pol"]]       # the first of them: the images stop at the cutouts' max_cands
    if cp:
        for k in ("pft", "pft_hits"):
            d[k] = np.stack([c["pol"][k] for c in cp])
        d["tscr"] = np.array([c["pol"]["tscr"] for c in cp], np.int32)
    d["cands"] = np.array([[c["snr"], c["peak_idx"], c["peak_time"], c["tfilt"], c["dmi"], c["dm"], c["ngiant"], c["i0"], c["i1"]]
                           for c in cc], np.float64)
    d["tsamp"] = np.float64(tsamp)
    with open(path + ".npz", "wb") as f:
        np.savez(f, **d)
    return len(cc)


def write_cutouts_npz(path, cands, tsamp):
    """The cutouts of one gulp's candidates (those that carry one; the others are left out) as one .npz: ft, ft_hits
    [n][nsub][nt], dt, dt_hits [n][ndmrow][nt], dm_rows [n][ndmrow], sub_freqs [nsub], and per cutout peak_idx, dm, snr,
    tfilt, tscr; tsamp.  Returns how many were written (0: no file)."""
    cc = [c for c in cands if "cutout" in c]
    if not cc:
        return 0
    d = {k: np.stack([c["cutout"][k] for c in cc]) for k in CUTOUT_KEYS}
    d["sub_freqs"] = np.asarray(cc[0]["cutout"]["sub_freqs"], np.float64)
    d["peak_idx"] = np.array([c["peak_idx"] for c in cc], np.int64)
    d["dm"] = np.array([c["dm"] for c in cc], np.float64)
    d["snr"] = np.array([c["snr"] for c in cc], np.float32)
    d["tfilt"] = np.array([c["tfilt"] for c in cc], np.int32)
    d["tscr"] = np.array([c["cutout"]["tscr"] for c in cc], np.int32)
    d["tsamp"] = np.float64(tsamp)
    with open(path, "wb") as f:
        np.savez(f, **d)
    return len(cc)


def _write_lines(path, cc, line):
    """the body of write_refined / write_subbands: line(c) of every candidate in cc; no file for none"""
    if cc:
        with open(path, "w") as f:
            f.write("".join(line(c) + "\n" for c in cc))
    return len(cc)


def refined_line(c):
    """a candidate's line followed by its refined DM, S/N, width (samples) and peak sample (stream index)"""
    r = c["refined"]
    return "%s\t%.6f\t%.4f\t%d\t%d" % (candidate_line(c), r["dm"], r["snr"], r["width"], r["peak"])


def write_refined(path, cands):
    """The refined candidates of one gulp (those that carry a refinement), one refined_line each.  Returns how many were
    written (0: no file)."""
    return _write_lines(path, [c for c in cands if c.get("refined")], refined_line)


def subband_line(c):
    """a sub-band candidate's line followed by its band (first base sub-band, how many), the band's edges in MHz and the
    full-band S/N at its peak"""
    return "%s\t%d\t%d\t%.4f\t%.4f\t%.4f" % (candidate_line(c), c["band"][0], c["band"][1], c["f_lo"], c["f_hi"], c["snr_full"])


def write_subbands(path, cands):
    """The sub-band candidates of one gulp (those that carry `band`), one subband_line each.  Returns how many were written
    (0: no file)."""
    return _write_lines(path, [c for c in cands if "band" in c], subband_line)


def periodic_line(c):
    """a periodicity candidate's line: snr period_s dm width_s phase dmi k p i m nharm"""
    return "%.4f\t%.9f\t%.4f\t%.9f\t%.6f\t%d\t%d\t%d\t%d\t%d\t%s" % (c["snr"], c["period_s"], c["dm"], c["width_s"], c["phase"],
                                                                        c["dmi"], c["k"], c["p"], c["i"], c["m"], c["nharm"])


def write_periodic(path, cands):
    """The periodicity candidates of one gulp (those that carry `period_s`), one periodic_line each.  Returns how many were
    written (0: no file)."""
    return _write_lines(path, [c for c in cands if "period_s" in c], periodic_line)


def write_chans(path, info, s):
    """One gulp's channel mask (Searcher.rfi_chan_info): the line `# nflag nact radius tol`, then `channel S fill recv` for
    every flagged channel, ascending.  Written for every gulp searched with the channel stage on, flagged channels or not."""
    radius, tol = s._rfichan
    with open(path, "w") as f:
        f.write("# %d %d %d %g\n" % (info["nflag"], s.nact, radius, tol))
        for c in np.nonzero(info["mask"])[0]:
            f.write("%d %d %d %d\n" % (c, info["stat"][c], info["fill"][c], info["recv"][c]))


def gulp_stem(utc_start, first_sample, tsamp, beam):
    """<UTC of the gulp's first sample>_<beam, two digits>: the name heimdall gives a gulp's candidate file, as far as
    this project knows it (unpinned)"""
    import calendar
    import time as _time
    t0 = calendar.timegm(_time.strptime(utc_start, "%Y-%m-%d-%H:%M:%S"))
    return "%s_%02d" % (_time.strftime("%Y-%m-%d-%H:%M:%S", _time.gmtime(t0 + int(first_sample * tsamp))), beam)


def open_search(a, hdr, gulp, device=None, searcher=None):
    """What main() and a host that feeds the search itself (process_baseband --search) share: the Searcher and the
    GulpSearch that the flags `a` (parse_args) ask for, for a stream whose SIGPROC header is `hdr` (nchans, fch1, foff,
    tsamp, tstart), and the writer of a batch of candidates.  gulp: GulpSearch's (None: whole host gulps through push()).
    device: instead of -gpu_id.  searcher: one made by an earlier call with the same flags and band, used again (a host's
    next observation).  Returns (searcher, gulp_search, emit); emit(cands) prints the candidates' lines, writes the
    -output_dir files of the batch that gulp_search has just returned, and returns how many there were."""
    import os
    import time as _time
    nchan, tsamp = hdr["nchans"], hdr["tsamp"]
    maxs = a.nsamps_gulp + int(4.148808e3 * a.dm[1] * abs((hdr["fch1"] + (nchan - 1) * hdr["foff"]) ** -2
                                                         - hdr["fch1"] ** -2) / tsamp) + 64
    s = searcher
    if s is None:
        zap = tuple(tuple(z) for z in a.zap_chans) if a.zap_chans else ()
        dml = None if a.dm_step > 0 else dedisp_dm_list(a.dm[0], a.dm[1], tsamp, hdr["fch1"], hdr["foff"], nchan, a.dm_tol)
        kw = dict(device=a.gpu_id if device is None else device, nchan=nchan, fch1=hdr["fch1"], foff=hdr["foff"], tsamp=tsamp,
                  boxcar_max=a.boxcar_max, zap=zap)
        s = Searcher(max_samples=maxs, dm_list=dml, dm_min=a.dm[0], dm_max=a.dm[1], dm_step=a.dm_step or 2.0, **kw)
        s.set_baseline(int(a.baseline_length / tsamp))
        if a.rfi_clean:
            s.set_rfi(narrow=not a.rfi_no_narrow, broad=not a.rfi_no_broad, tol=a.rfi_tol)
        if getattr(a, "rfi_chan", False):
            s.set_rfi_chan(radius=a.rfi_chan_radius, tol=a.rfi_chan_tol)
    utc = _time.strftime("%Y-%m-%d-%H:%M:%S", _time.gmtime(round((hdr.get("tstart", 40587.0) - 40587.0) * 86400.0)))
    cut = None
    if a.cutouts:
        # the default geometry; fewer time bins where the blocks are too short for 256 bins of 64 samples, fewer
        # subbands where 64 does not divide the band
        s.set_cutouts(nsub=64 if nchan % 64 == 0 else 1, nt=min(256, (maxs // 64) & ~1), max_cands=a.cutout_max)
        cut = dict(thresh=a.cutout_thresh, max_per_gulp=a.cutout_max)
    ref = None
    if a.refine:
        # the default geometry; a shorter window where the blocks are too short for two of the default
        s.set_refine(half_window=max(64, min(128, (maxs // 4) & ~1)), max_cands=a.refine_max)
        ref = dict(thresh=a.refine_thresh, max_per_gulp=a.refine_max)
    pol = None
    if getattr(a, "pol", False):
        s.set_pol(off_len=a.pol_off[0], guard=a.pol_off[1], rm=(a.rm[0], a.rm_step, rm_trials(a.rm[0], a.rm[1], a.rm_step)),
                  max_cands=a.pol_max)
        pol = dict(thresh=a.pol_thresh, max_per_gulp=a.pol_max)
    sub = None
    if getattr(a, "subbands", 0):
        if nchan % a.subbands:
            raise SystemExit("search -subbands: %d does not divide the %d channels" % (a.subbands, nchan))
        s.set_subbands(nsb=a.subbands)
        sub = dict(thresh=a.subband_thresh, send=a.subband_send)
    per = None
    if getattr(a, "periodic", None):
        try:
            k_lo, k_hi = periodic_octaves(a.periodic[0], a.periodic[1], a.periodic_bins, tsamp)
            s.set_periodic(bins=a.periodic_bins, k_lo=k_lo, k_hi=k_hi)
        except ValueError as e:
            raise SystemExit("search -periodic: %s" % e)
        per = dict(thresh=a.periodic_thresh, max_per_gulp=a.periodic_max, p_range=tuple(a.periodic))
    gi = dict(sep_time=a.cand_sep_time, sep_dm=a.cand_sep_dm, sep_filter=a.cand_sep_filter,
              max_giants=a.max_giants) if a.giants else None
    g = GulpSearch(s, threshold=a.detect_thresh, coincidencer=a.coincidencer, utc_start=utc, beam=a.beam, cutouts=cut,
                   refine=ref, giants=gi, gulp=gulp, pol=pol, subbands=sub, periodic=per)
    if a.output_dir:
        os.makedirs(a.output_dir, exist_ok=True)
    stems = set()

    def new_stem(first):
        stem = gulp_stem(utc, first, tsamp, a.beam)
        if stem in stems:                           # gulps shorter than a second: keep the names apart
            stem = "%s.%d_%02d" % (stem[:-3], first, a.beam)
        stems.add(stem)
        return stem

    def emit(batch):
        cands = [c for c in batch if "band" not in c and "period_s" not in c]
        for c in cands:
            print(candidate_line(c))
        for c in batch:
            if "band" in c:
                print(subband_line(c))
        for c in batch:
            if "period_s" in c:
                print(periodic_line(c))
        stem = new_stem(g.last_first) if a.output_dir and batch else None
        if a.output_dir:                            # the channel masks of the gulps that the call searched
            for first, info in g.chan_log:                # (beside the batch's .cand where the gulp is the batch's)
                cstem = stem if stem and first == g.last_first else new_stem(first)
                write_chans(os.path.join(a.output_dir, cstem + ".chans"), info, s)
        if stem:
            if cands:
                with open(os.path.join(a.output_dir, stem + ".cand"), "w") as f:
                    f.write("".join(candidate_line(c) + "\n" for c in cands))
            if sub:
                write_subbands(os.path.join(a.output_dir, stem + ".subband"), batch)
            if per:
                write_periodic(os.path.join(a.output_dir, stem + ".periodic"), batch)
            if a.cutouts:
                write_cutouts_npz(os.path.join(a.output_dir, stem + ".cutouts.npz"), cands, tsamp)
            if a.refine:
                write_refined(os.path.join(a.output_dir, stem + ".refined"), cands)
            if pol:
                write_pol(os.path.join(a.output_dir, stem + ".pol"), cands, tsamp)
        return len(batch)

    return s, g, emit


def main(argv=None):
    """heimdall's place in the chain for a SIGPROC file: `python -m vlite-fast_amd.search -f obs_kur.fil
    -dm 2 1000 -boxcar_max 64 -nsamps_gulp 30720 -zap_chans 0 190 -zap_chans 3900 4096 -rfi_clean
    -giants -output_dir /mnt/ssd/cands -cutouts -coincidencer vlite-nrl:27555` (the flags of
    scripts/start_heimdall_single_antenna:21; that launch leaves heimdall's RFI cleaning on, which here is -rfi_clean).
    Prints heimdall-format candidate lines per gulp and, with -coincidencer, sends them there; with -output_dir each
    gulp that has candidates also gets a .cand file of the same lines, with -cutouts a .cutouts.npz beside it, with
    -refine a .refined file (the refined candidates' lines, each followed by refined DM, S/N, width and peak sample).
    -giants takes the candidates from the GPU's giants and clusters (heimdall's -cand_sep_time / -cand_sep_dm /
    -cand_sep_filter; this project's own definition) instead of the host's grouping of the point list.
    -pol takes a nifs 4 file (process_baseband -P 2 --coherence: AA, BB, CR, CI), searches its total intensity and gives
    the strongest candidates of each gulp Stokes spectra and an RM synthesis (-rm, -rm_step, -pol_off; uncalibrated:
    include/pb_hip.h, pb_search_set_pol); with -output_dir a .pol file (each line followed by RM, L/I, V/I, position angle
    in degrees) and a .pol.npz beside each .cand.
    -subbands N (2, 4, 8 or 16) follows each gulp's search with the sub-band search for band-limited bursts (include/pb_hip.h,
    pb_search_set_subbands; -subband_thresh, default -detect_thresh): the sub-band candidates are printed after the gulp's
    full-band lines, each as its nine columns followed by band_first band_count f_lo f_hi snr_full, and with -output_dir
    written to a .subband file beside .cand, which stays as it is; -subband_send also sends them to the coincidencer.
    -periodic P_LO P_HI follows each gulp's search with the periodicity search of every trial DM's series (include/pb_hip.h,
    pb_search_set_periodic; -periodic_bins, -periodic_thresh, -periodic_max): the candidates, grouped by harmonic ratio
    (candidates_from_periodic), are printed last as snr period_s dm width_s phase dmi k p i m nharm and with -output_dir
    written to a .periodic file beside .cand; nothing periodic goes to the coincidencer.
    -stream_chunk M reads the file in pieces of M samples and feeds them to GulpSearch(gulp=-nsamps_gulp): the same
    lines, gathered on the GPU as a host behind pb_process would gather them; on this path 4- and 2-bit files are
    accepted and fed packed."""
    a = parse_args(argv)
    use_pol = getattr(a, "pol", False)
    with open(a.fil, "rb") as f:
        hdr, off = sig.read_header(f.read(4096))
    nbits = hdr["nbits"]
    if a.stream_chunk:
        if nbits not in (8, 4, 2) or hdr.get("nifs", 1) != 1 or (hdr["nchans"] * nbits) % 8:
            raise SystemExit("search -stream_chunk: 8-, 4- or 2-bit single-IF filterbanks whose time samples fill whole bytes only")
    elif use_pol:
        if nbits != 8 or hdr.get("nifs", 1) != 4:
            raise SystemExit("search -pol: 8-bit filterbanks with nifs 4 (AA, BB, CR, CI) only")
    elif nbits != 8 or hdr.get("nifs", 1) != 1:
        raise SystemExit("search: 8-bit single-IF filterbanks only")
    s, g, emit = open_search(a, hdr, a.nsamps_gulp if a.stream_chunk else None)
    nchan, ntot = hdr["nchans"], 0
    nrow = nchan * (4 if use_pol else 1)              # bytes of a time sample on the whole-gulp path

    with open(a.fil, "rb") as f:
        f.seek(off)
        rowb = nchan * nbits // 8
        while a.stream_chunk:
            blk = np.frombuffer(f.read(a.stream_chunk * rowb), np.uint8)
            if blk.size < rowb:
                ntot += emit(g.flush())
                break
            ntot += emit(g.feed(blk[:blk.size // rowb * rowb], nbit=nbits))
        while not a.stream_chunk:
            blk = np.frombuffer(f.read(a.nsamps_gulp * nrow), np.uint8)
            if blk.size < nrow:
                break
            ntot += emit(g.push(blk[:blk.size // nrow * nrow].reshape(-1, nrow)))
    ntot += emit(g.finish())
    s.close()
    return ntot


if __name__ == "__main__":
    main()
