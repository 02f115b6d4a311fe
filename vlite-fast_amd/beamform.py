"""Coherent beams from the voltage dumps of a set of antennas.

The phased sums run on the GPU (include/pb_hip.h: pb_beamform, over the spectra that a coherence = 1 handle keeps);
everything in this module is host-side numpy on small arrays:

  read_beams(path, nant)           a text file of beams, one line of nant delays (samples) per beam
  loc_delays(path, nant)           the per-antenna delays that the localise tool measured (its fit_samples)
  one_hot(nant)                    the delays (0) and gains of the nant single-antenna beams
  ratio(series, incoherent)        a beam's summed power over that of the incoherent sum

Command line (offline; the dump files are those the hosts' --replay reads, read as the correlate tool reads them):

  python -m vlite-fast_amd.beamform --replay ant0.uw ant1.uw ... [--offsets n0 n1 ...] [--stream raw|kur]
         (--delays d0 d1 ... | --beams beams.txt | --loc loc.npz) [--phase-turns] [--dm DM] [--tscr N]
         [--rows-per-seg N] [--max-seg N] [--seconds N] [--null K [--null-min-ratio X] [--null-train ROW0 ROW1]]
         [--search "<search flags>" [--search-single]] [--fil DIR] [--level-alpha X] -o beams.npz
  (--rows-per-seg R --max-seg S: the handle's batch, 1024 x 10 rows = one second by default; a file's tail that does not
  fill a batch is left out.  Per batch the tool emits the output samples whose whole window -- in every channel, with
  the shift of --dm -- lies within the batch: the correlate tool's limit for its gates, and an output sample is never
  split between two calls)

A delay is the number of samples at 128 MS/s that the antenna is LATE (correlate's delay_samples, localise's
fit_samples and antenna_delays).  An antenna d samples late carries exp(-2 pi i k d / 12500), which the delay takes
off, and, where the delay lies in front of the sampler (geometry, cables), localise.phase_turns(d) = -384 MHz x delay
= -3 d turns on top; a shift of the sample stream, as --offsets makes, carries none.  pb_beamform adds psi to an
antenna's phase, so --phase-turns passes psi = -localise.phase_turns(delay), which takes that phase off again: the
same correction as localise.baseline_phase makes for the imager's PHASE mode (tests/test_array_conventions_cpu.py holds
the two to each other).  --dm makes the output samples follow a pulse of that dispersion measure:
shift = correlate.dm_row0(dm, 0, ...).  The tool always appends the nant single-antenna beams (one-hot gains, delay 0)
to the call; their sum is the incoherent beam.

--null K takes the K strongest directions per (pol, channel) out of the coherent beams (nulling.py; DESIGN.md section
13): per batch the tool correlates the batch's rows -- all of them, or the batch-relative rows ROW0 .. ROW1 - 1 of
--null-train, which can leave a pulse out -- in gates of at most one segment, as the correlate tool does, builds the
projectors (with --null-min-ratio X only in channels whose largest eigenvalue is at least X times the mean of the
others) and forms the coherent beams with pb_beamform_proj.  The single-antenna beams stay un-nulled, through
pb_beamform, so `incoherent` and `ratio` mean what they mean without --null.

--search "<flags>" searches every coherent beam for pulses where it lies on the GPU: per batch
pb_beam_planes turns the beams into zero-mean, unit-variance fp32 planes that stay in HBM, and each beam's plane is fed to
a search of its own (search.parse_flags and search.open_search, as process_baseband --search does; GulpSearch.feed_plane
quantises it to 8 bits with the reference's rule).  The flags are the search tool's less -f and -stream_chunk; -beam is set
by this tool: coherent beam b is beam b + 1, and with --search-single the nant single-antenna beams follow as beams
nbeam + 1 .. nbeam + nant (un-nulled, like `incoherent`).  The band in the search's header is the filterbank's own fch1 and
foff: plane channel c is FFT bin 2155 + c, the filterbank's channel c (tests/test_gpu_beam_planes.py holds the two planes
to each other), and tsamp = tscr * 12500 / 128e6 s.  The search dedisperses itself and the batches must tile time, so
--search refuses --dm and a --tscr that does not divide a batch's rows.  One searcher at the production flags holds
2.17 GB of device memory, which bounds the beams one card can search.
--fil DIR writes each searched beam's 8-bit SIGPROC filterbank, DIR/beamNN.fil: the bytes are those the search's quantiser
makes of the plane on the device (Searcher.push_plane into a searcher kept for that purpose, fetched and transposed); the
host has no quantiser of its own.  sigproc.sigproc_header writes the filterbank's 781.25 us sampling only, so --fil is
accepted at --tscr 8 alone.
The planes' level is a running one, kept on the host per (beam, channel): the first batch is divided by its own mean
(pb_beam_planes' level_out), later batches by run, updated as run += alpha * (level_out - run) where level_out > 0 (a
channel whose run is still 0 takes level_out as it is).  --level-alpha (default 0.25) is a host-side choice of this tool,
not tuned and not part of the library's definition.

beams.npz: beams float32 [nbeam][nout][4][4096] (the coherent beams' AA, BB, CR, CI dynamic spectra, tscr rows per
sample), sample_row int64 [nout] (the first row, counted from the start of the data, of each output sample in channel
0; channel c starts shift[c] rows later), shift int32 [4096], rows_used int32 [nbeam][nout][4096], incoherent float64
[nout][4][4096] (the single-antenna beams added), series float64 [nbeam][nout] and incoherent_series float64 [nout]
(AA + BB added over the band), ratio float64 [nbeam] (sum of series / sum of incoherent_series), delays float64
[nbeam][nant], phase_turns float64 [nbeam][nant] (the psi handed to pb_beamform, in turns: -localise.phase_turns(delays)
with --phase-turns, else 0), freqs_mhz [4096], tscr, options (JSON).  With --search also search_cands float64 [n][6]: beam number, S/N, peak sample
(counted from the start of the data, in output samples), log2 boxcar width, trial-DM index, DM of every candidate, in the
order the searches gave them.  With --null also null_count int64 [2][4096], the vectors nulled per (pol,
channel), added over the batches, and rows_used counts every antenna (pb_beamform_proj's).
"""
import argparse
import importlib
import json
import sys

import numpy as np

replay_batches = importlib.import_module("vlite-fast_amd.replay_batches")
NCHANOUT = 4096


def _corr():
    return importlib.import_module("vlite-fast_amd.correlate")


def read_beams(path, nant):
    """float64 [nbeam][nant] from a text file: one line of nant delays per beam, '#' starts a comment"""
    rows = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            words = line.split("#")[0].split()
            if not words:
                continue
            if len(words) != nant:
                raise ValueError("%s:%d: %d delays, %d antennas" % (path, n, len(words), nant))
            rows.append([float(w) for w in words])
    if not rows:
        raise ValueError("%s holds no beam" % path)
    return np.array(rows, np.float64)


def loc_delays(path, nant):
    """float64 [1][nant]: localise's fit_samples [2 slots][nant] (samples later than antenna 0), the slots averaged"""
    z = np.load(path)
    if "fit_samples" not in z.files:
        raise ValueError("%s holds no fit_samples" % path)
    fit = np.asarray(z["fit_samples"], np.float64)
    if fit.ndim != 2 or fit.shape[1] != nant:
        raise ValueError("%s: fit_samples is %s, %d antennas" % (path, fit.shape, nant))
    return fit.mean(axis=0)[None]


def one_hot(nant):
    """(delay float64 [nant][nant] = 0, gain float32 [nant][nant] = the unit matrix)"""
    return np.zeros((nant, nant), np.float64), np.eye(nant, dtype=np.float32)


def ratio(series, incoherent_series):
    """sum of a beam's series over the sum of the incoherent one; series [..][nout]"""
    return np.asarray(series, np.float64).sum(axis=-1) / float(np.sum(incoherent_series))


# ---------------------------------------------------------------------------------------------------------------
# the tool (its common arguments, the dump reader and the batch loop are shared with correlate.py: replay_batches.py)

def update_level(run, level_out, alpha):
    """the running level float32 [nbeam][4096] after a batch whose own level is level_out: level_out itself for the first
    batch (run None) and where run is still 0, else run + alpha * (level_out - run) where level_out > 0"""
    level_out = np.asarray(level_out, np.float32)
    if run is None:
        return level_out.copy()
    step = (run + np.float32(alpha) * (level_out - run)).astype(np.float32)
    return np.where(level_out > 0, np.where(run > 0, step, level_out), run).astype(np.float32)


def plane_header(tscr):
    """the SIGPROC fields that describe a beam plane: channel c is FFT bin 2155 + c -- the filterbank's own channel
    order, so its fch1 and foff --, sampled every tscr rows"""
    search = importlib.import_module("vlite-fast_amd.search")
    return dict(nchans=NCHANOUT, fch1=search.FCH1, foff=search.FOFF, tsamp=tscr * 12500 / 128e6, tstart=40587.0, nbits=8, nifs=1)


class PlaneSearch(object):
    """What --search and --fil do with a group of beams that one pb_beam_planes call forms: the running level, one
    GulpSearch per beam (--search) and one .fil file per beam (--fil), beam numbers first + 1 .. first + nbeam."""

    def __init__(self, args, nbeam, first, quantiser):
        self.nbeam, self.first, self.alpha, self.run = nbeam, first, args.level_alpha, None
        self.searches, self.files, self.quantiser, self.cands = [], [], quantiser, []
        if args.search is not None:
            import copy
            search = importlib.import_module("vlite-fast_amd.search")
            for b in range(nbeam):
                flags = copy.copy(args.search_flags)
                flags.beam = first + b + 1
                self.searches.append(search.open_search(flags, plane_header(args.tscr), flags.nsamps_gulp, device=args.device))
        if args.fil is not None:
            import os
            sigproc = importlib.import_module("vlite-fast_amd.sigproc")
            os.makedirs(args.fil, exist_ok=True)
            for b in range(nbeam):
                f = open(os.path.join(args.fil, "beam%02d.fil" % (first + b + 1)), "wb")
                f.write(sigproc.sigproc_header(0, 0.0, 0.0, "beam%02d" % (first + b + 1), 40587.0, 1, 8))
                self.files.append(f)

    def _took(self, b, batch, emit):
        emit(batch)
        self.cands += [(self.first + b + 1, c["snr"], c["peak_idx"], c["tfilt"], c["dmi"], c["dm"]) for c in batch if "band" not in c]

    def batch(self, h, stream, nseg, delay, psi, gain, proj, tscr, nout):
        """form the group's planes for the handle's current batch (shifts 0) and hand each beam's on, where it lies"""
        _, ptr, level_out = h.beam_planes(stream, nseg, delay, psi, gain, proj, None, tscr, nout, level=self.run, to_host=False)
        self.run = update_level(self.run, level_out, self.alpha)
        for b in range(self.nbeam):
            at = ptr + b * nout * NCHANOUT * 4
            if self.searches:
                _, g, emit = self.searches[b]
                self._took(b, g.feed_plane(device_ptr=at, nsamp=nout, scale=1.0), emit)
            if self.files:
                q = self.quantiser
                q.push_plane(device_ptr=at, nsamp=nout, scale=1.0)
                self.files[b].write(np.ascontiguousarray(q.gulp_fetch().T).tobytes())
                q.gulp_advance(0)

    def close(self):
        for b, (s, g, emit) in enumerate(self.searches):
            self._took(b, g.flush(), emit)
            self._took(b, g.finish(), emit)
            s.close()
        for f in self.files:
            f.close()


def make_parser():
    p = argparse.ArgumentParser(prog="beamform", description="coherent beams from voltage dumps")
    replay_batches.add_arguments(p)
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--delays", nargs="+", type=float, default=None, help="one beam: samples that each antenna is late")
    g.add_argument("--beams", default=None, help="text file, one line of delays per beam")
    g.add_argument("--loc", default=None, help="the localise tool's npz: its fit_samples")
    p.add_argument("--phase-turns", action="store_true",
                   help="take off the phase localise.phase_turns says a late antenna carries: psi = -phase_turns(delay)")
    p.add_argument("--dm", type=float, default=None, help="output samples follow a pulse of this DM")
    p.add_argument("--tscr", type=int, default=8, help="rows per output sample")
    p.add_argument("--null", type=int, default=None, metavar="K",
                   help="project the K strongest directions per (pol, channel) out of the coherent beams")
    p.add_argument("--null-min-ratio", type=float, default=None, metavar="X",
                   help="null only where the largest eigenvalue is at least X times the mean of the others")
    p.add_argument("--null-train", nargs=2, type=int, default=None, metavar=("ROW0", "ROW1"),
                   help="rows ROW0 .. ROW1 - 1 of each batch make the matrices (default: all)")
    p.add_argument("--search", default=None, metavar="FLAGS",
                   help="search every coherent beam on the GPU: the search tool's flags in one string (-beam is set here)")
    p.add_argument("--search-single", action="store_true", help="with --search or --fil: the single-antenna beams too")
    p.add_argument("--fil", default=None, metavar="DIR", help="write each searched beam's 8-bit filterbank to DIR/beamNN.fil (--tscr 8)")
    p.add_argument("--level-alpha", type=float, default=0.25,
                   help="weight of a batch's own level in the planes' running level (a host-side choice, not tuned)")
    return p


def parse_args(argv=None):
    p = make_parser()
    a = p.parse_args(argv)
    replay_batches.check_arguments(p, a)
    if a.delays is not None and len(a.delays) != len(a.replay):
        p.error("--delays: one value per --replay file")
    if a.delays is not None and not np.all(np.isfinite(a.delays)):
        p.error("--delays must be finite")
    if a.tscr <= 0 or a.tscr > a.rows_per_seg * a.max_seg or a.seconds < 0:
        p.error("--tscr must be 1 .. the %d rows of a batch, --seconds not negative" % (a.rows_per_seg * a.max_seg))
    if a.dm is not None and a.dm < 0:
        p.error("--dm must not be negative")
    if a.null is None and (a.null_min_ratio is not None or a.null_train is not None):
        p.error("--null-min-ratio and --null-train need --null")
    if a.null is not None and not 1 <= a.null <= len(a.replay) - 1:
        p.error("--null must be 1 .. the number of antennas less one")
    if a.null_min_ratio is not None and not a.null_min_ratio > 0:
        p.error("--null-min-ratio must be positive")
    if a.null_train is not None and not 0 <= a.null_train[0] < a.null_train[1] <= a.rows_per_seg * a.max_seg:
        p.error("--null-train: 0 <= ROW0 < ROW1 <= the %d rows of a batch" % (a.rows_per_seg * a.max_seg))
    a.search_flags = None
    if a.search is not None or a.fil is not None:
        if a.dm is not None:
            p.error("--search and --fil: not with --dm (the search dedisperses itself, and the shifts must be 0 so that batches tile time)")
        if (a.rows_per_seg * a.max_seg) % a.tscr:
            p.error("--search and --fil: --tscr must divide the %d rows of a batch" % (a.rows_per_seg * a.max_seg))
        if not 0 < a.level_alpha <= 1:
            p.error("--level-alpha must be in (0, 1]")
    elif a.search_single:
        p.error("--search-single needs --search or --fil")
    if a.fil is not None and a.tscr != 8:
        p.error("--fil: only at --tscr 8: the SIGPROC header this project writes (sigproc.sigproc_header) carries the "
                "filterbank's own sampling of 8 rows, 781.25 us, and no other")
    if a.search is not None:
        a.search_flags = importlib.import_module("vlite-fast_amd.search").parse_flags(a.search)
    return a


def beam_table(args):
    """the beams of the command line: (delay float64 [nbeam][nant], psi float64 [nbeam][nant] or None)"""
    nant = len(args.replay)
    if args.delays is not None:
        delay = np.array([args.delays], np.float64)
    elif args.beams is not None:
        delay = read_beams(args.beams, nant)
    else:
        delay = loc_delays(args.loc, nant)
    if delay.shape[0] + nant > 64:
        raise ValueError("at most %d beams beside the %d single-antenna ones" % (64 - nant, nant))
    psi = None
    if args.phase_turns:
        # pb_beamform ADDS psi to an antenna's phase: what takes off the phase_turns(d) that an antenna d late carries
        psi = -importlib.import_module("vlite-fast_amd.localise").phase_turns(delay)
    return delay, psi


def run(args):
    corr = _corr()
    nant = len(args.replay)
    R, S, tscr = args.rows_per_seg, args.max_seg, args.tscr
    T = R * S
    try:
        delay, psi = beam_table(args)
        shift = None
        if args.dm is not None:
            shift = corr.dm_row0(args.dm, 0, T - tscr + 1)
    except (ValueError, IOError) as e:
        raise SystemExit("beamform: %s" % e)
    nb = delay.shape[0]
    nout = (T - (0 if shift is None else int(shift.max()))) // tscr            # per batch
    # the call's beams: the coherent ones, then the single-antenna ones
    d1, g1 = one_hot(nant)
    all_delay = np.concatenate([delay, d1])
    all_psi = None if psi is None else np.concatenate([psi, np.zeros_like(d1)])
    all_gain = np.concatenate([np.ones(delay.shape, np.float32), g1])
    beams, used, incoherent, rows = [], [], [], []
    nulling = importlib.import_module("vlite-fast_amd.nulling") if args.null is not None else None
    null_count = np.zeros((2, NCHANOUT), np.int64)
    # --search / --fil: the coherent beams' planes, and with --search-single the single-antenna beams' (un-nulled)
    planes = args.search is not None or args.fil is not None
    coherent = single = quantiser = None
    for k, h, stream in replay_batches.batches(args, "beamform"):
        if planes and coherent is None:
            if args.fil is not None:
                searcher = importlib.import_module("vlite-fast_amd.searcher")
                quantiser = searcher.Searcher(device=args.device, nchan=NCHANOUT, max_samples=nout + 128, dm_min=0, dm_max=1,
                                              dm_step=1, boxcar_max=1, zap=())
                quantiser.set_gulp(1)
            coherent = PlaneSearch(args, nb, 0, quantiser)
            single = PlaneSearch(args, nant, nb, quantiser) if args.search_single else None
        if nulling is None:
            v, u = h.beamform(stream, S, all_delay, all_psi, all_gain, shift, tscr, nout)
            beams.append(v[:nb].copy())
            used.append(u[:nb].copy())
            incoherent.append(v[nb:].astype(np.float64).sum(axis=0))
        else:
            r0, r1 = args.null_train if args.null_train is not None else (0, T)
            cov = nulling.covariances(nulling.training_vis(h, stream, S, r0, r1), nant)
            proj, count = nulling.projectors(cov, args.null, args.null_min_ratio)
            null_count += count
            v, u = h.beamform_proj(stream, S, delay, proj, psi, None, shift, tscr, nout)
            beams.append(v)
            used.append(u)
            incoherent.append(h.beamform(stream, S, d1, None, g1, shift, tscr, nout)[0].astype(np.float64).sum(axis=0))
        rows.append(k * T + tscr * np.arange(nout, dtype=np.int64))
        if planes:                                              # (last: the planes live until the handle's next beam call)
            coherent.batch(h, stream, S, delay, psi, None, proj if nulling is not None else None, tscr, nout)
            if single is not None:
                single.batch(h, stream, S, d1, None, g1, None, tscr, nout)
    cands = []
    for group in (coherent, single):
        if group is not None:
            group.close()
            cands += group.cands
    if quantiser is not None:
        quantiser.close()
    beams = np.concatenate(beams, axis=1)
    incoherent = np.concatenate(incoherent, axis=0)
    series = beams[:, :, :2].astype(np.float64).sum(axis=(2, 3))
    inc_series = incoherent[:, :2].sum(axis=(1, 2))
    out = dict(beams=beams, sample_row=np.concatenate(rows),
               shift=np.zeros(NCHANOUT, np.int32) if shift is None else shift.astype(np.int32),
               rows_used=np.concatenate(used, axis=1), incoherent=incoherent, series=series, incoherent_series=inc_series,
               ratio=ratio(series, inc_series), delays=delay, phase_turns=np.zeros_like(delay) if psi is None else psi,
               freqs_mhz=corr.chan_freqs_mhz(), tscr=np.int64(tscr))
    if args.search is not None:
        out["search_cands"] = np.array(cands, np.float64).reshape(len(cands), 6)
    options = vars(args).copy()
    del options["search_flags"]
    if not planes:
        for name in ("search", "search_single", "fil", "level_alpha"):      # without them the file is what it was
            del options[name]
    if nulling is None:
        for name in ("null", "null_min_ratio", "null_train"):       # without --null the file is what it was
            del options[name]
    else:
        out["null_count"] = null_count
    out["options"] = np.array(json.dumps(options, sort_keys=True))
    np.savez(args.output, **out)
    return out


def main(argv=None):
    run(parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
