"""Visibilities and delays of a set of antennas from their voltage dumps.

The X step runs on the GPU (include/pb_hip.h: pb_correlate / pb_correlate_gated, over the spectra that a
coherence = 1 handle keeps); everything in this module is host-side numpy on its small outputs:

  baselines(nant)                    the (i, j) list in the library's baseline order
  dm_row0(dm, t0_row, nrows_total)   the per-channel first rows of a dedispersed gate
  lag_delays(vis, ...)               the reference's get_delays / get_delays_new (analysis/baseband.py:741, :723)
  fit_delays(delays)                 the reference's fit_delays (:773) as the linear least-squares problem it is

Command line (offline; the dump files are those the hosts' --replay reads):

  python -m vlite-fast_amd.correlate --replay ant0.uw ant1.uw ... [--offsets n0 n1 ...] [--stream raw|kur]
         [--int-rows N] [--seconds N] [--dm DM --t0 ROW --width ROWS [--off-gates K]]
         [--track --antennas ants.txt --centre RA_DEG DEC_DEG --time UNIX [--clock-ns c0 c1 ...] | --track-model m.txt]
         -o out.npz
  (--rows-per-seg R --max-seg S: the handle's batch, 1024 x 10 rows = one second by default; a file's tail that does not
  fill a batch is left out, and the gates of --dm must lie within one batch)

--track stops the fringes (pb_correlate_tracked): every antenna's spectra are turned, row by row, by a delay and a phase
that drift linearly, before the products are added -- for anything integrated longer than a few tens of milliseconds on
long baselines.  The model is localise.track_model's for the position --centre at --time, the time of the data's first
row (ants.txt as for localise), taken relative to antenna 0; or --track-model reads it: one line of delay0 delay_rate
psi0 psi_rate per antenna (samples late, samples per row, turns, turns per row).  Batch k is correlated with row_base =
k * S * R, the ungated sum and the --dm gates alike; out.npz then also holds track_model [nant][4] and track_row_base
[batches].  Without --track / --track-model nothing changes.

out.npz: vis complex128 [nbl][4][4096] (all gates added in double), rows_used int64 [nbl][4096], baselines [nbl][2],
freqs_mhz [4096], lag_cycles / lag_samples [2 pols][nant][nant] (pol products 0 and 3), fit_samples [2][nant] and
fit_model [2][nant][nant] (fit_delays of lag_samples, the reference's sign: lag[i][j] = m_i - m_j is positive when antenna
j is the later one), delay_samples = -fit_samples (how many samples later than antenna 0 each antenna sees the sky:
--offsets of these values lines the antennas up), rows (rows correlated), options (JSON).  With --dm also gate_vis complex64 [2 K + 1][nbl][4][4096] (K off-gates
before the on-gate, the on-gate, K after it, each --width rows long and dedispersed alike), gate_rows_used,
gate_row0 [2 K + 1][4096] (rows counted from the start of the data) and gate_on = K.
"""
import argparse
import collections
import importlib
import json
import sys

import numpy as np

replay_batches = importlib.import_module("vlite-fast_amd.replay_batches")
NFFT, NCHAN, CHANMIN, NCHANOUT = 12500, 6251, 2155, 4096
VLITE_RATE = 128000000
ROW_S = NFFT / float(VLITE_RATE)            # one FFT row: 97.65625 us, 10240 rows per second
DM_CONST = 4.15e-3                          # s GHz^2 cm^3 / pc: the injection's constant (src/pb_kernels.cu:344)


def baselines(nant):
    """[(i, j)] for i <= j in the library's order: bl = i * nant - i * (i - 1) / 2 + (j - i)"""
    return [(i, j) for i in range(nant) for j in range(i, nant)]


def chan_freqs_mhz():
    """channel c of the 4096 sits at 384 - (2155 + c) * 64 / 6251 MHz"""
    return 384.0 - (CHANMIN + np.arange(NCHANOUT)) * 64.0 / NCHAN


def dm_row0(dm, t0_row, nrows_total):
    """int32 [4096]: the first row of a gate that follows a dispersed pulse arriving in channel 0 (the top of the band) at
    row t0_row.  Delay of channel c = dm * 4.15e-3 s * (f_c^-2 - f_0^-2), f in GHz, rounded to rows of 12500 / 128e6 s.
    The constant is the one the front end's FRB injection uses (src/pb_kernels.cu:344: 4.15e-3, not the search's
    4.148808e-3), so that a gate made here lies on a pulse injected there.  ValueError when a first row leaves
    [0, nrows_total)."""
    f = chan_freqs_mhz() * 1e-3
    delay = float(dm) * DM_CONST * (f ** -2 - f[0] ** -2)
    rows = int(t0_row) + np.floor(delay / ROW_S + 0.5).astype(np.int64)
    if rows.min() < 0 or rows.max() >= nrows_total:
        raise ValueError("dm_row0: rows %d..%d leave [0, %d)" % (rows.min(), rows.max(), nrows_total))
    return rows.astype(np.int32)


LagDelays = collections.namedtuple("LagDelays", "cycles samples peak third")


def lag_delays(vis, used=None, mask=None, normalize=True):
    """The reference's crude delay estimate (get_delays; with a mask and normalize, get_delays_new).
    vis: complex [nbl][4][nchan] in baseline order (gates already added).  For pol products 0 and 3 and every baseline
    i < j: c = V_ij / sqrt(V_ii V_jj) (normalize), times the mask, numpy.fft.fft over the channels, the argmax of the
    modulus, fftfreq(nchan) there.  used (rows_used [nbl][nchan]): channels without a single used row are masked;
    mask: bool / float [nchan].
    -> LagDelays: cycles [2][nant][nant] in cycles per channel (antisymmetric), samples = cycles * 12500 (samples at
    128 MS/s), peak and third = the largest and third-largest modulus of each lag spectrum."""
    vis = np.asarray(vis)
    nbl, nchan = vis.shape[0], vis.shape[-1]
    nant = int(round((np.sqrt(8 * nbl + 1) - 1) / 2))
    bls = baselines(nant)
    assert len(bls) == nbl, "vis is not [nant (nant + 1) / 2][4][nchan]"
    index = dict((b, k) for k, b in enumerate(bls))
    m = np.ones(nchan) if mask is None else np.asarray(mask, float)
    freqs = np.fft.fftfreq(nchan)
    cycles = np.zeros((2, nant, nant))
    peak = np.zeros((2, nant, nant))
    third = np.zeros((2, nant, nant))
    for k, prod in enumerate((0, 3)):
        for (i, j), bl in index.items():
            if i == j:
                continue
            c = vis[bl, prod].astype(np.complex128)
            mm = m if used is None else m * (np.asarray(used)[bl] > 0)
            if normalize:
                d = np.sqrt(vis[index[(i, i)], prod].real.astype(float) * vis[index[(j, j)], prod].real.astype(float))
                c = np.where(d > 0, c / np.where(d > 0, d, 1.0), 0)
            y = np.abs(np.fft.fft(c * mm))
            a = int(np.argmax(y))
            cycles[k, i, j] = freqs[a]
            cycles[k, j, i] = -freqs[a]
            peak[k, i, j] = peak[k, j, i] = y[a]
            third[k, i, j] = third[k, j, i] = np.sort(y)[-3] if nchan >= 3 else 0.0
    return LagDelays(cycles, cycles * NFFT, peak, third)


def fit_delays(delays):
    """Per-antenna delays, antenna 0 at 0, that minimise the residuals of delays[i][j] = m_i - m_j over the baselines
    i < j: the reference's fit_delays as linear least squares.  -> (m [nant], model [nant][nant])"""
    delays = np.asarray(delays, float)
    nant = delays.shape[0]
    iu = np.triu_indices(nant, k=1)
    if nant == 1:
        return np.zeros(1), np.zeros((1, 1))
    design = np.zeros((len(iu[0]), nant - 1))
    for r, (i, j) in enumerate(zip(*iu)):
        if i > 0:
            design[r, i - 1] += 1.0
        design[r, j - 1] -= 1.0
    sol = np.linalg.lstsq(design, delays[iu], rcond=None)[0]
    m = np.append(0.0, sol)
    return m, m[:, None] - m[None, :]


# ---------------------------------------------------------------------------------------------------------------
# the tool (its common arguments, the dump reader and the batch loop are shared with beamform.py: replay_batches.py)

def make_parser():
    p = argparse.ArgumentParser(prog="correlate", description="visibilities and delays of voltage dumps")
    replay_batches.add_arguments(p)
    p.add_argument("--int-rows", type=int, default=1024, help="rows per gate of the ungated correlation")
    p.add_argument("--dm", type=float, default=None)
    p.add_argument("--t0", type=int, default=None, help="row (from the start of the data) of the pulse in channel 0")
    p.add_argument("--width", type=int, default=None, help="rows per on / off gate")
    p.add_argument("--off-gates", type=int, default=2, help="off gates before and after the on gate")
    p.add_argument("--track", action="store_true", help="stop the fringes with the geometric model of --centre at --time")
    p.add_argument("--antennas", help="`name X Y Z` per antenna, metres, Earth-fixed")
    p.add_argument("--centre", nargs=2, type=float, metavar=("RA_DEG", "DEC_DEG"))
    p.add_argument("--time", type=float, help="unix time of the data's first row")
    p.add_argument("--clock-ns", nargs="+", type=float, default=None, help="clock delay per antenna")
    p.add_argument("--track-model", help="stop the fringes with this model: delay0 delay_rate psi0 psi_rate per antenna")
    return p


def parse_args(argv=None):
    p = make_parser()
    a = p.parse_args(argv)
    replay_batches.check_arguments(p, a)
    if a.int_rows <= 0 or a.seconds < 0 or a.off_gates < 0:
        p.error("--int-rows must be positive, --seconds and --off-gates not negative")
    if (a.rows_per_seg * a.max_seg) % a.int_rows:
        p.error("--int-rows must divide the %d rows of a batch" % (a.rows_per_seg * a.max_seg))
    gate = (a.dm, a.t0, a.width)
    if any(v is not None for v in gate):
        if any(v is None for v in gate):
            p.error("--dm, --t0 and --width go together")
        if a.dm < 0 or a.t0 < 0 or a.width <= 0:
            p.error("--dm and --t0 must not be negative, --width must be positive")
    geometry = (a.antennas, a.centre, a.time)
    if a.track and a.track_model is not None:
        p.error("--track builds the model from geometry and --track-model reads it: give one of them")
    if a.track:
        if any(v is None for v in geometry):
            p.error("--track needs --antennas, --centre and --time")
        if not -90.0 <= a.centre[1] <= 90.0:
            p.error("--centre: the declination must lie within -90..90 degrees")
    elif any(v is not None for v in geometry) or a.clock_ns is not None:
        p.error("--antennas, --centre, --time and --clock-ns belong to --track")
    return a


def read_track_model(path, nant):
    """m.txt -> float64 [nant][4]; ValueError for a malformed line or a wrong count"""
    rows = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            w = line.split("#")[0].split()
            if not w:
                continue
            try:
                rows.append([float(v) for v in w])
            except ValueError:
                rows.append(None)
            if rows[-1] is None or len(w) != 4:
                raise ValueError("%s:%d: expected `delay0 delay_rate psi0 psi_rate`" % (path, ln))
    if len(rows) != nant:
        raise ValueError("%s: %d antennas, --replay has %d" % (path, len(rows), nant))
    return np.array(rows, np.float64)


def tracking_model(args):
    """the model of --track / --track-model, float64 [nant][4], or None"""
    nant = len(args.replay)
    try:
        if args.track_model is not None:
            return read_track_model(args.track_model, nant)
        if args.track:
            loc = importlib.import_module("vlite-fast_amd.localise")
            _, xyz = loc.read_antennas(args.antennas, nant)
            if args.clock_ns is not None and len(args.clock_ns) != nant:
                raise ValueError("--clock-ns: one value per antenna (%d)" % nant)
            m = loc.track_model(xyz, np.radians(args.centre[0]), np.radians(args.centre[1]), args.time, args.clock_ns)
            return m - m[0]            # what all antennas share leaves every product; the delays stay within the array's
    except (ValueError, IOError) as e:
        raise SystemExit("correlate: %s" % e)
    return None


def run(args):
    R, S = args.rows_per_seg, args.max_seg
    bls = baselines(len(args.replay))
    vis = np.zeros((len(bls), 4, NCHANOUT), np.complex128)
    rows_used = np.zeros((len(bls), NCHANOUT), np.int64)
    gates = None
    model, row_bases = tracking_model(args), []
    if args.dm is not None:
        K = args.off_gates
        starts = [args.t0 + (m - K) * args.width for m in range(2 * K + 1)]
        batch = args.t0 // (S * R)
        try:
            row0 = np.stack([dm_row0(args.dm, s - batch * S * R, S * R - args.width + 1) for s in starts])
        except ValueError as e:
            raise SystemExit("correlate: the gates must lie within one batch of %d rows (%s)" % (S * R, e))
        gates = dict(batch=batch, row0=row0)
    for k, h, stream in replay_batches.batches(args, "correlate"):
        if model is None:
            v, u = h.correlate(stream, S, args.int_rows)
        else:
            row_bases.append(k * S * R)
            v, u = h.correlate_tracked(stream, S, model, row_base=k * S * R, nrows=args.int_rows)
        vis += v.astype(np.complex128).sum(axis=0)
        rows_used += u.astype(np.int64).sum(axis=0)
        if gates is not None and gates["batch"] == k:
            if model is None:
                gates["vis"], gates["used"] = h.correlate_gated(stream, S, gates["row0"], args.width)
            else:
                gates["vis"], gates["used"] = h.correlate_tracked(stream, S, model, row_base=k * S * R, row0=gates["row0"],
                                                                  nrows=args.width)
        nsec = k + 1                             # batches done
    if gates is not None and "vis" not in gates:
        raise SystemExit("correlate: --t0 lies beyond the %d batches read" % nsec)
    lag = lag_delays(vis, used=rows_used)
    fits = [fit_delays(lag.samples[k]) for k in range(2)]
    out = dict(vis=vis, rows_used=rows_used, baselines=np.array(bls, np.int32), freqs_mhz=chan_freqs_mhz(),
               lag_cycles=lag.cycles, lag_samples=lag.samples, lag_peak=lag.peak, lag_third=lag.third,
               fit_samples=np.stack([f[0] for f in fits]), fit_model=np.stack([f[1] for f in fits]),
               delay_samples=-np.stack([f[0] for f in fits]),
               rows=np.int64(nsec * S * R), options=np.array(json.dumps(vars(args), sort_keys=True)))
    if model is not None:
        out.update(track_model=model, track_row_base=np.array(row_bases, np.int64))
    if gates is not None:
        out.update(gate_vis=gates["vis"], gate_rows_used=gates["used"],
                   gate_row0=gates["row0"].astype(np.int64) + gates["batch"] * S * R, gate_on=np.int64(args.off_gates))
    np.savez(args.output, **out)
    return out


def main(argv=None):
    run(parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
