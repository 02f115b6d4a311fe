"""Fine delays and a sky position from the gated visibilities of a voltage dump.

The hot path runs on the GPU (include/pb_hip.h: pb_imager_*, libpb.PbImager): for every hypothesis -- one delay, and
optionally one phase, per baseline -- rotate each baseline's 4096-channel visibility by the delay slope, add the
channels, combine the baselines.  Everything in this module is host-side numpy on small arrays:

  weighted_vis(gate_vis, gate_on, gate_rows_used, mask)   on-gate minus off-gates over sqrt(auto_i auto_j), cross baselines
  coarse_delays(u)                    whole-lag delays of weighted visibilities (the argmax of their lag spectrum)
  fine_delays(imager, coarse, ...)    the reference's fractional-delay scan and parabola (analysis/loc_step2.py:91-120)
  gmst_rad, precession_matrix, source_vector, antenna_delays, sky_grid     the geometry (see "Frame" below)
  antenna_delay_rates, track_model    the delays' drift as the Earth turns; the fringe-stopping model of correlate --track
  antenna_to_baseline, phase_turns, baseline_phase                         per-antenna values to per-baseline ones
  tdoa_rms_map(measured, clock, tau_grid, mask)                            the rms map of analysis/loc_step3.py:312-348

Signs.  d[a] is how many samples LATER antenna a sees the signal; a baseline (i, j) has dd = d[j] - d[i], and with the
correlator's V_ij = X_i conj(X_j) the sum over the channels of V_ij exp(-2 pi i k dd / 12500) peaks at the true dd.

Frame.  A J2000 position is precessed to the date (IAU 1976) and turned by the mean sidereal time into the Earth-fixed
frame of the antenna coordinates.  Nutation, aberration, UT1 - UTC and polar motion are left out: tens of arcseconds.
Positions are meant differentially, against a calibrator imaged the same way (analysis/beamforming.py:12-15).

Phase mode.  For a band sampled from 384 MHz downwards, an antenna tau seconds late carries the phase -384e6 tau turns
= -3 d turns on top of the delay slope (whole turns for whole samples).  Whether the array's signals arrive
fringe-stopped is not known from the reference, so DELAY mode, which adds moduli and needs no phase, is the default;
PHASE mode adds real parts after baseline_phase and holds only if the signals are as described here.

Command line (writes one npz):

  python -m vlite-fast_amd.localise --vis out.npz [--scan-only]
         [--antennas ants.txt --centre RA_DEG DEC_DEG --time UNIX [--clock-ns c0 c1 ...]
          [--half-width ARCMIN] [--npix N] [--mode delay|phase]] [--zap LO HI]... -o loc.npz

out.npz is what `python -m vlite-fast_amd.correlate` wrote: its gates (gate_vis, gate_on, gate_rows_used) where it has
them, else its summed visibilities as one on-gate without off-gates.  ants.txt: one `name X Y Z` line per antenna, metres,
Earth-fixed, in the order of the visibilities' antennas.  --zap LO HI masks the channels [LO, HI) of the 4096.
loc.npz: baselines, coarse_samples, scan_x, fine_samples / fine_peak / fine_err [2][nbl], fit_samples [2][nant] (how many
samples later than antenna 0), fit_model; unless --scan-only also grid_ra_deg / grid_dec_deg [N][N], image [N][N],
peak_pixel (row, column), peak_ra_deg, peak_dec_deg, tdoa_rms_ns [N][N], residual_samples [nbl] at the peak; options.
"""
import argparse
import importlib
import json
import sys

import numpy as np

NFFT, CHANMIN, NCHANOUT = 12500, 2155, 4096
VLITE_RATE = 128e6
C_M_S = 299792458.0
SCAN_SPAN, SCAN_STEP = 5.0, 0.1             # the reference's dom = linspace(-5, 5, 101), samples


def cross_baselines(nant):
    return [(i, j) for i in range(nant) for j in range(i + 1, nant)]


def _nant_of_cross(nbl):
    nant = int(round((1 + np.sqrt(1 + 8 * nbl)) / 2))
    if nant * (nant - 1) // 2 != nbl:
        raise ValueError("%d is not a number of cross baselines" % nbl)
    return nant


def weighted_vis(gate_vis, gate_on, gate_rows_used, mask=None):
    """gate_vis complex [ngate][nbl][4][4096] in the correlator's baseline order (autos included), gate_on the index of
    the on-gate, gate_rows_used [ngate][nbl][4096]; mask bool [4096], False = leave the channel out.
    For the cross baselines i < j and the products 0 and 3: (on-gate - mean of the off-gates) / sqrt(auto_i auto_j), the
    autos being those of the off-gates (the reference's get_delays normalisation), 0 where the on-gate used no row, the
    channel is masked or an auto is not positive.  With a single gate there is no off-gate: nothing is subtracted and the
    autos are the gate's own.  -> (u complex64 [ncross][2][4096], [(i, j)])"""
    corr = importlib.import_module("vlite-fast_amd.correlate")
    gate_vis = np.asarray(gate_vis)
    used = np.asarray(gate_rows_used)
    ngate, nbl = gate_vis.shape[:2]
    nant = int(round((np.sqrt(8 * nbl + 1) - 1) / 2))
    all_bls = corr.baselines(nant)
    if len(all_bls) != nbl or gate_vis.shape[2:] != (4, NCHANOUT) or used.shape != (ngate, nbl, NCHANOUT):
        raise ValueError("gate_vis must be [ngate][nant (nant + 1) / 2][4][4096] and gate_rows_used [ngate][nbl][4096]")
    if not 0 <= gate_on < ngate:
        raise ValueError("gate_on outside the gates")
    index = dict((b, k) for k, b in enumerate(all_bls))
    on = gate_vis[gate_on].astype(np.complex128)
    if ngate > 1:
        off = np.delete(gate_vis, gate_on, axis=0).astype(np.complex128).mean(axis=0)
        sig, norm = on - off, off
    else:
        sig, norm = on, on
    m = np.ones(NCHANOUT, bool) if mask is None else np.asarray(mask, bool)
    bls = cross_baselines(nant)
    u = np.zeros((len(bls), 2, NCHANOUT), np.complex64)
    for b, (i, j) in enumerate(bls):
        for s, prod in enumerate((0, 3)):
            d = norm[index[(i, i)], prod].real * norm[index[(j, j)], prod].real
            ok = m & (used[gate_on, index[(i, j)]] > 0) & (d > 0)
            u[b, s] = np.where(ok, sig[index[(i, j)], prod] / np.sqrt(np.where(d > 0, d, 1.0)), 0)
    return u, bls


def antenna_to_baseline(d_ant, bls):
    """d_ant [..][nant] -> d[j] - d[i] per baseline, [..][nbl]"""
    d_ant = np.asarray(d_ant, float)
    i = np.array([b[0] for b in bls])
    j = np.array([b[1] for b in bls])
    return d_ant[..., j] - d_ant[..., i]


def phase_turns(d_ant):
    """the phase in turns that an antenna d samples late carries on top of its delay slope: -384e6 tau = -3 d"""
    return -3.0 * np.asarray(d_ant, float)


def baseline_phase(d_ant, bls):
    """dpsi of PbImager.run for antenna delays d_ant: the phase of V_ij = X_i conj(X_j), phase_turns(d_i) -
    phase_turns(d_j), [..][nbl]"""
    return -antenna_to_baseline(phase_turns(d_ant), bls)


def coarse_delays(u):
    """u complex [nbl][2][4096] -> [nbl]: the lag, in samples, at which the two slots' lag spectra together are largest
    (resolution 12500 / 4096 samples); positive when the baseline's second antenna is the later one"""
    y = np.abs(np.fft.fft(np.asarray(u, np.complex128), axis=-1)).sum(axis=1)
    return np.fft.fftfreq(NCHANOUT)[np.argmax(y, axis=-1)] * NFFT


def parabola_peak(x, y):
    """the reference's three-point fit (loc_step2.py:108-117) around the largest y: (x0, peak, err)"""
    a = int(np.argmax(y))
    a = min(max(a, 1), len(y) - 2)
    p = np.polyfit(x[a - 1:a + 2], y[a - 1:a + 2], 2)
    if not p[0] < 0:
        return float(x[a]), float(y[a]), float("inf")
    fmax = -p[1] ** 2 / (4 * p[0]) + p[2]
    return float(-p[1] / p[0] * 0.5), float(fmax), float((-0.5 * fmax / p[0]) ** 0.5)


def fine_delays(imager, coarse_samples, span=SCAN_SPAN, step=SCAN_STEP, bls=None):
    """The scan of loc_step2.py:91-120 on the GPU: pixel p tries coarse[b] + x_p on every baseline at once, x from -span
    to span in steps of `step`; the parabola through the three points around each baseline's and slot's largest modulus
    gives its delay, peak and curvature width (the reference's err); correlate.fit_delays then gives per-antenna delays.
    imager: a PbImager whose visibilities are set.  bls: the baselines' (i, j); default all cross pairs in order.
    -> dict(x [npix], scan complex64 [npix][nbl][2], dd [npix][nbl], samples, peak, err [2][nbl],
            fit_samples [2][nant] (samples later than antenna 0), fit_model [2][nant][nant])"""
    corr = importlib.import_module("vlite-fast_amd.correlate")
    coarse = np.asarray(coarse_samples, float)
    nbl = coarse.shape[0]
    if bls is None:
        bls = cross_baselines(_nant_of_cross(nbl))
    nant = 1 + max(max(b) for b in bls)
    n = int(round(span / step))
    x = np.arange(-n, n + 1) * float(step)
    dd = coarse[None, :] + x[:, None]
    _, scan = imager.run(dd, per_baseline=True)
    mod = np.abs(scan.astype(np.complex128))
    samples, peak, err = np.zeros((2, nbl)), np.zeros((2, nbl)), np.zeros((2, nbl))
    for s in range(2):
        for b in range(nbl):
            x0, peak[s, b], err[s, b] = parabola_peak(x, mod[:, b, s])
            samples[s, b] = coarse[b] + x0
    fits = []
    for s in range(2):
        lag = np.zeros((nant, nant))
        for b, (i, j) in enumerate(bls):
            lag[i, j], lag[j, i] = samples[s, b], -samples[s, b]
        mfit, model = corr.fit_delays(lag)          # lag[i][j] = m_i - m_j = d_j - d_i: m = -d
        fits.append((-mfit, model))
    return dict(x=x, scan=scan, dd=dd, samples=samples, peak=peak, err=err,
                fit_samples=np.stack([f[0] for f in fits]), fit_model=np.stack([f[1] for f in fits]))


# ---------------------------------------------------------------------------------------------------------------
# geometry

def gmst_rad(unix):
    """Greenwich mean sidereal time: 18.697374558 + 24.06570982441908 (JD - 2451545.0) hours, JD = unix / 86400 +
    2440587.5 (UTC taken for UT1), in radians within [0, 2 pi)"""
    jd = np.asarray(unix, float) / 86400.0 + 2440587.5
    hours = 18.697374558 + 24.06570982441908 * (jd - 2451545.0)
    return np.mod(hours, 24.0) * (np.pi / 12.0)


def _r2(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])


def _r3(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


def precession_matrix(T):
    """IAU 1976 precession from J2000 to T Julian centuries after it: P = R3(-z) R2(theta) R3(-zeta)"""
    arcsec = np.pi / (180.0 * 3600.0)
    zeta = (2306.2181 * T + 0.30188 * T ** 2 + 0.017998 * T ** 3) * arcsec
    z = (2306.2181 * T + 1.09468 * T ** 2 + 0.018203 * T ** 3) * arcsec
    theta = (2004.3109 * T - 0.42665 * T ** 2 - 0.041833 * T ** 3) * arcsec
    return _r3(-z) @ _r2(theta) @ _r3(-zeta)


def source_vector(ra, dec, unix):
    """unit vector(s) towards the J2000 position (radians) in the Earth-fixed frame at `unix`: precessed to the date,
    then s = (cos d cos(a - GMST), cos d sin(a - GMST), sin d).  ra, dec scalars or arrays -> [..][3]"""
    ra, dec = np.asarray(ra, float), np.asarray(dec, float)
    T = (float(unix) / 86400.0 + 2440587.5 - 2451545.0) / 36525.0
    v = np.stack([np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)], axis=-1)
    return v @ (_r3(gmst_rad(unix)) @ precession_matrix(T)).T


def antenna_delays(xyz_m, s, clock_ns=None):
    """xyz_m [nant][3] Earth-fixed metres, s [..][3] -> samples LATE per antenna, [..][nant]: -(r . s) / c 128e6, plus
    the antenna's clock delay"""
    d = -(np.asarray(s, float) @ np.asarray(xyz_m, float).T) / C_M_S * VLITE_RATE
    if clock_ns is not None:
        d = d + np.asarray(clock_ns, float) * 1e-9 * VLITE_RATE
    return d


EARTH_RATE = 2.0 * np.pi * 1.00273790935 / 86400.0      # rad / s: the rate of gmst_rad
ROW_S = NFFT / VLITE_RATE                                # one FFT row, 97.65625 us


def antenna_delay_rates(xyz_m, s, unix=None):
    """the time derivative of antenna_delays(xyz_m, s) in samples per row of 12500 samples.  In the Earth-fixed frame
    ds/dt = EARTH_RATE (s_y, -s_x, 0): the sidereal angle.  Precession moves s 10^-7 as fast (50" a year); with `unix`,
    the time at which s = source_vector(.., unix) was taken, its term R3 dP/dt P^T R3^T s is added.
    xyz_m [nant][3], s [..][3] -> [..][nant]"""
    s = np.asarray(s, float)
    ds = EARTH_RATE * np.stack([s[..., 1], -s[..., 0], np.zeros_like(s[..., 0])], axis=-1)
    if unix is not None:
        T = (float(unix) / 86400.0 + 2440587.5 - 2451545.0) / 36525.0
        h = 1e-3                                         # centuries: P is a cubic in T, the difference exact to 10^-9 of it
        dP = (precession_matrix(T + h) - precession_matrix(T - h)) / (2 * h * 36525.0 * 86400.0)
        g = _r3(gmst_rad(unix))
        ds = ds + s @ (g @ dP @ precession_matrix(T).T @ g.T).T
    return antenna_delays(xyz_m, ds) * ROW_S


def track_model(xyz_m, ra, dec, unix, clock_ns=None):
    """The model of PbHandle.correlate_tracked for a J2000 position (radians) from `unix` on: float64 [nant][4] = delay0,
    delay_rate, psi0, psi_rate with row 0 at `unix`.  The delays are antenna_delays' and antenna_delay_rates'; the
    phases take the band as sampled from 384 MHz downwards, psi0 = -phase_turns(delay0) and psi_rate =
    -phase_turns(delay_rate), which stops the fringe only if the signals arrive as "Phase mode" above describes: the sign
    of that 384 MHz term is not known from the reference."""
    s = source_vector(ra, dec, unix)
    d0 = antenna_delays(xyz_m, s, clock_ns)
    d1 = antenna_delay_rates(xyz_m, s, unix)
    return np.stack([d0, d1, -phase_turns(d0), -phase_turns(d1)], axis=-1)


def sky_grid(ra0, dec0, half_width_arcmin, n):
    """gnomonic n x n grid around (ra0, dec0), radians: pixel iy * n + ix lies at tangent-plane offsets (l, m) =
    (east, north) = linspace(-hw, hw, n)[ix], [iy].  -> (ra [n n], dec [n n])"""
    hw = np.radians(half_width_arcmin / 60.0)
    off = np.linspace(-hw, hw, n) if n > 1 else np.zeros(1)
    m, l = np.meshgrid(off, off, indexing="ij")
    s0 = np.array([np.cos(dec0) * np.cos(ra0), np.cos(dec0) * np.sin(ra0), np.sin(dec0)])
    east = np.array([-np.sin(ra0), np.cos(ra0), 0.0])
    north = np.array([-np.sin(dec0) * np.cos(ra0), -np.sin(dec0) * np.sin(ra0), np.cos(dec0)])
    v = s0 + l.ravel()[:, None] * east + m.ravel()[:, None] * north
    v /= np.linalg.norm(v, axis=1)[:, None]
    return np.mod(np.arctan2(v[:, 1], v[:, 0]), 2 * np.pi), np.arcsin(v[:, 2])


def tdoa_rms_map(measured, clock, tau_grid, mask):
    """The rms map of loc_step3.py:312-348.  measured, clock [nbl] and tau_grid [..][nbl] in seconds, mask bool [nbl]:
    chi = measured 1e9 + clock 1e9 + tau_grid 1e9, rms over the masked baselines, in ns"""
    total = np.asarray(measured, float) * 1e9
    total = total + np.asarray(clock, float) * 1e9
    chi = total + np.asarray(tau_grid, float) * 1e9
    return (chi[..., np.asarray(mask, bool)] ** 2).mean(axis=-1) ** 0.5


# ---------------------------------------------------------------------------------------------------------------
# the tool

def read_antennas(path, nant):
    """ants.txt -> (names, xyz [nant][3]); ValueError for a malformed line or a wrong count"""
    names, xyz = [], []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.split("#")[0].strip()
            if not line:
                continue
            w = line.split()
            if len(w) != 4:
                raise ValueError("%s:%d: expected `name X Y Z`" % (path, ln))
            try:
                xyz.append([float(v) for v in w[1:]])
            except ValueError:
                raise ValueError("%s:%d: X Y Z must be numbers" % (path, ln))
            names.append(w[0])
    if len(names) != nant:
        raise ValueError("%s: %d antennas, the visibilities have %d" % (path, len(names), nant))
    return names, np.array(xyz)


def make_parser():
    p = argparse.ArgumentParser(prog="localise", description="fine delays and a sky position from gated visibilities")
    p.add_argument("--vis", required=True, help="the npz of `python -m vlite-fast_amd.correlate`")
    p.add_argument("--scan-only", action="store_true", help="fine delays only")
    p.add_argument("--antennas", help="`name X Y Z` per antenna, metres, Earth-fixed")
    p.add_argument("--centre", nargs=2, type=float, metavar=("RA_DEG", "DEC_DEG"))
    p.add_argument("--time", type=float, help="unix time of the pulse")
    p.add_argument("--clock-ns", nargs="+", type=float, default=None, help="clock delay per antenna")
    p.add_argument("--half-width", type=float, default=10.0, help="half width of the grid in arcmin")
    p.add_argument("--npix", type=int, default=201, help="pixels along a side of the grid")
    p.add_argument("--mode", choices=("delay", "phase"), default="delay")
    p.add_argument("--zap", nargs=2, type=int, action="append", default=[], metavar=("LO", "HI"))
    p.add_argument("-o", "--output", required=True)
    return p


def parse_args(argv=None):
    p = make_parser()
    a = p.parse_args(argv)
    if not a.scan_only:
        if a.antennas is None or a.centre is None or a.time is None:
            p.error("a position needs --antennas, --centre and --time (or give --scan-only)")
        if not -90.0 <= a.centre[1] <= 90.0:
            p.error("--centre: the declination must lie within -90..90 degrees")
        if a.npix < 1 or a.npix > 1024 or a.half_width <= 0:          # 1024^2 pixels: 32 MB per baseline on the device
            p.error("--npix must be 1..1024 and --half-width positive")
    for lo, hi in a.zap:
        if not 0 <= lo < hi <= NCHANOUT:
            p.error("--zap LO HI: 0 <= LO < HI <= %d" % NCHANOUT)
    return a


def load_gates(path):
    """the gates of a correlate npz: (gate_vis, gate_on, gate_rows_used)"""
    z = np.load(path)
    if "gate_vis" in z.files:
        return z["gate_vis"], int(z["gate_on"]), z["gate_rows_used"]
    if "vis" not in z.files or "rows_used" not in z.files:
        raise ValueError("%s holds neither gate_vis nor vis / rows_used" % path)
    return z["vis"][None], 0, z["rows_used"][None]


def run(args):
    lp = importlib.import_module("vlite-fast_amd.libpb")
    try:
        gate_vis, gate_on, gate_used = load_gates(args.vis)
        mask = np.ones(NCHANOUT, bool)
        for lo, hi in args.zap:
            mask[lo:hi] = False
        u, bls = weighted_vis(gate_vis, gate_on, gate_used, mask)
        if not bls:
            raise ValueError("%s holds one antenna: no baseline" % args.vis)
        nant = 1 + max(max(b) for b in bls)
        if not args.scan_only:
            names, xyz = read_antennas(args.antennas, nant)
            if args.clock_ns is not None and len(args.clock_ns) != nant:
                raise ValueError("--clock-ns: one value per antenna (%d)" % nant)
    except (ValueError, IOError) as e:
        raise SystemExit("localise: %s" % e)
    nscan = 2 * int(round(SCAN_SPAN / SCAN_STEP)) + 1
    npix = 0 if args.scan_only else args.npix * args.npix
    coarse = coarse_delays(u)
    out = dict(baselines=np.array(bls, np.int32), coarse_samples=coarse,
               options=np.array(json.dumps(vars(args), sort_keys=True)))
    with lp.PbImager(len(bls), max(nscan, npix)) as im:
        im.set_vis(u)
        fd = fine_delays(im, coarse, SCAN_SPAN, SCAN_STEP, bls=bls)
        out.update(scan_x=fd["x"], fine_samples=fd["samples"], fine_peak=fd["peak"], fine_err=fd["err"],
                   fit_samples=fd["fit_samples"], fit_model=fd["fit_model"])
        if not args.scan_only:
            n = args.npix
            ra, dec = sky_grid(np.radians(args.centre[0]), np.radians(args.centre[1]), args.half_width, n)
            d_ant = antenna_delays(xyz, source_vector(ra, dec, args.time), args.clock_ns)
            dd = antenna_to_baseline(d_ant, bls)
            dpsi = baseline_phase(d_ant, bls) if args.mode == "phase" else None
            image = im.run(dd, dpsi, mode=args.mode)
            ipix = int(np.argmax(image))
            measured = fd["samples"].mean(axis=0) / VLITE_RATE
            geom = antenna_to_baseline(antenna_delays(xyz, source_vector(ra, dec, args.time)), bls) / VLITE_RATE
            clock = np.zeros(len(bls)) if args.clock_ns is None else antenna_to_baseline(np.asarray(args.clock_ns) * 1e-9, bls)
            rms = tdoa_rms_map(measured, -clock, -geom, np.isfinite(fd["err"]).all(axis=0))
            out.update(antenna_names=np.array(names), grid_ra_deg=np.degrees(ra).reshape(n, n),
                       grid_dec_deg=np.degrees(dec).reshape(n, n), image=image.reshape(n, n),
                       peak_pixel=np.array([ipix // n, ipix % n]), peak_ra_deg=np.degrees(ra[ipix]),
                       peak_dec_deg=np.degrees(dec[ipix]), tdoa_rms_ns=rms.reshape(n, n),
                       residual_samples=fd["samples"].mean(axis=0) - dd[ipix])
    np.savez(args.output, **out)
    return out


def main(argv=None):
    run(parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
