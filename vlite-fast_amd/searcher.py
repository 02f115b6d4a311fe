"""Searcher: the ctypes surface of libpb_hip.so's pb_search_* (csrc/search_*.hip), one method per entry point, with the
constants of the reference's production launch and the trial-DM list.  search.py is the entry and the public name."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import libpb as _lp
from .candidates import subband_list

# heimdall flags of the reference's production launch
HEIMDALL_DM = (2.0, 1000.0)
HEIMDALL_BOXCAR_MAX = 64
HEIMDALL_GULP = 30720
HEIMDALL_ZAP = ((0, 190), (3900, 4096))
FCH1 = 384 + (2155 - 0.5) * (-64. / 6251)     # MHz, src/process_baseband.cu:261
FOFF = -64. / 6251
TSAMP = 12500.0 / 128e6 * 8


def dedisp_dm_list(dm_start, dm_end, tsamp, fch1, foff, nchan, tol=1.25, pulse_width_us=40.0):
    """Trial DMs spaced so that the smearing of a pulse at one DM by the next step stays within `tol`:
    the recursion of the dedisp library's generate_dm_list that heimdall runs on (-dm_tol 1.25,
    -dm_pulse_width 40 are heimdall's defaults; dedisp/heimdall are third party, unpinned forks in the
    reference's src/INSTALL and absent here: restated from the published algorithm, Barsdell et al. 2012
    / Levin 2012 eq. 4.6; the candidate list it leads to stays parity-unpinned).
        a = 8.3 df / f^3 (us per DM unit per channel, f = band centre in GHz, df in MHz)
        dm' = (b2 dm + sqrt(-a2 b2 dm^2 + (a2 + b2) k)) / (a2 + b2),
        a2 = a^2, b2 = a2 nchan^2 / 16, k = (dt^2 + w^2)(tol^2 - 1) + tol^2 a2 dm^2"""
    dt = tsamp * 1e6
    f = (fch1 + (nchan / 2 - 0.5) * foff) * 1e-3
    tol2 = tol * tol
    a = 8.3 * abs(foff) / (f * f * f)
    a2 = a * a
    b2 = a2 * (nchan * nchan / 16.0)
    c = (dt * dt + pulse_width_us * pulse_width_us) * (tol2 - 1.0)
    dms = [float(dm_start)]
    while dms[-1] < dm_end:
        prev = dms[-1]
        k = c + tol2 * a2 * prev * prev
        dms.append((b2 * prev + np.sqrt(-a2 * b2 * prev * prev + (a2 + b2) * k)) / (a2 + b2))
    return np.asarray(dms, np.float32)


# what a set_*() call has switched on (Searcher._cut, _ref, _gi, _pol, _sub, _rfichan; None while the stage is off)
Cut = namedtuple("Cut", "nsub nt ndmrow max_cands")
Ref = namedtuple("Ref", "nstep half_window wmax max_cands")
Gi = namedtuple("Gi", "sep_time sep_dm sep_filter max_giants")
Pol = namedtuple("Pol", "off_len guard rm max_cands")             # rm = (rm_lo, rm_step, nrm)
Sub = namedtuple("Sub", "nsb bands max_points")                   # bands = [(first, count), ..]
RfiChan = namedtuple("RfiChan", "radius tol")
Per = namedtuple("Per", "bins k_lo k_hi")
# attribute -> (the subject of "... not switched on", the call that switches it on)
STAGES = dict(_cut=("cutouts are", "set_cutouts"), _pol=("polarisation is", "set_pol"), _ref=("refinement is", "set_refine"),
              _sub=("the sub-band search is", "set_subbands"), _gi=("giants are", "set_giants"),
              _per=("the periodicity search is", "set_periodic"))
POL_KEYS = ("on", "non", "off", "noff", "F", "kbest", "summary")  # of Searcher.pol, one entry per request
CUTOUT_KEYS = ("ft", "ft_hits", "dt", "dt_hits", "dm_rows")       # of Searcher.cutouts, one entry per request


def block_arg(a, dtype, row, nbit, device_ptr, nsamp, what):
    """A block given as a host array or as a device address: (pointer, codes_on_device, nsamp, the flat host array that owns
    the bytes or None).  a: host array of dtype holding samples of nbit bits, `row` of them per time sample; nsamp None: as
    many time samples as it holds, fewer than an explicit nsamp is refused.  device_ptr needs nsamp."""
    if device_ptr is not None:
        if nsamp is None:
            raise ValueError("device_ptr needs nsamp")
        return C.c_void_p(device_ptr), 1, int(nsamp), None
    a = np.ascontiguousarray(a, dtype).ravel()
    per = a.itemsize * 8 // nbit
    if nsamp is None:
        nsamp = a.size * per // row
    elif a.size * per < int(nsamp) * row:
        raise ValueError("%s holds fewer than nsamp samples" % what)
    return a.ctypes.data_as(C.c_void_p), 0, int(nsamp), a


def requests(dtype, *cols):
    """request columns (scalars or equally long sequences) -> the contiguous [n][len(cols)] array the library reads"""
    return np.ascontiguousarray(np.stack(np.broadcast_arrays(*[np.atleast_1d(c) for c in cols]), axis=1), dtype)


def peak_dict(buf, n, tout, max_out):
    """the dict of peaks() / gulp_peaks() from the library's [max_out][4] list, its count and the planes' length"""
    b = buf[:min(n, max_out, 1 << 20)]             # (the device list holds 2^20 points)
    return dict(dmi=b[:, 0].copy(), t=b[:, 1].copy(), snr=b[:, 2].copy().view(np.float32), width_log2=b[:, 3].astype(np.uint8),
                total=n, tout=tout)


class Searcher(object):
    def __init__(self, device=0, nchan=4096, max_samples=HEIMDALL_GULP, fch1=FCH1, foff=FOFF, tsamp=TSAMP,
                 dm_min=HEIMDALL_DM[0], dm_max=HEIMDALL_DM[1], dm_step=2.0, boxcar_max=HEIMDALL_BOXCAR_MAX,
                 zap=HEIMDALL_ZAP, dm_list=None):
        """dm_list: explicit trial DMs (e.g. dedisp_dm_list(...)); default the linear grid dm_min..dm_max"""
        self._lp = _lp
        self._L = _lp.load()
        zr = (C.c_int * (2 * len(zap)))(*[v for pair in zap for v in pair])
        self._s = C.c_void_p()
        if dm_list is not None:
            dl = np.ascontiguousarray(dm_list, np.float32)
            rc = self._L.pb_search_create_list(device, nchan, max_samples, fch1, foff, tsamp,
                                               dl.ctypes.data_as(C.POINTER(C.c_float)), dl.size, boxcar_max, zr, len(zap),
                                               C.byref(self._s))
        else:
            rc = self._L.pb_search_create(device, nchan, max_samples, fch1, foff, tsamp, dm_min, dm_max, dm_step,
                                          boxcar_max, zr, len(zap), C.byref(self._s))
        self._check(rc, "pb_search_create", handle=False)
        ndm, nbox, md = C.c_int(), C.c_int(), C.c_int()
        self._L.pb_search_info(self._s, C.byref(ndm), C.byref(nbox), C.byref(md))
        self.ndm, self.nbox, self.max_delay = ndm.value, nbox.value, md.value
        self.nchan, self.tsamp = nchan, tsamp
        zapped = np.zeros(nchan, bool)
        for lo, hi in zap:
            zapped[max(lo, 0):max(hi, 0)] = True
        self.chans = np.nonzero(~zapped)[0]     # the unzapped channels, ascending
        self.nact = int(self.chans.size)
        self.max_samples = max_samples
        self.fch1, self.foff = fch1, foff
        self._cut = None                 # Cut(nsub, nt, ndmrow, max_cands) once set_cutouts has switched them on
        self._ref = None                 # Ref(nstep, half_window, wmax, max_cands) once set_refine has switched it on
        self._gi = None                  # Gi(sep_time, sep_dm, sep_filter, max_giants) once set_giants has switched it on
        self._pol = None                 # Pol(off_len, guard, (rm_lo, rm_step, nrm), max_cands) once set_pol has switched it on
        self._sub = None                 # Sub(nsb, [(first, count), ..], max_points) once set_subbands has switched it on
        self._rfichan = None             # RfiChan(radius, tol) once set_rfi_chan has switched the channel stage on
        self._per = None                 # Per(bins, k_lo, k_hi) once set_periodic has switched it on
        self.dms = dm_min + dm_step * np.arange(self.ndm) if dm_list is None else np.asarray(dm_list, np.float64)
        self._nsamp = 0
        self._tout = 0                   # output samples of the planes on the device (the last search's, or set_planes')
        self._tsearch = 0                # output samples of the last search: the length of its series

    def _check(self, rc, name, exc=None, handle=True):
        """raise for a non-zero return code: PbError("<name> failed (rc): <last error>"), or exc(<last error>)"""
        if rc != 0:
            err = self._L.pb_search_last_error(self._s if handle else None).decode()
            raise exc(err) if exc else self._lp.PbError("%s failed (%d): %s" % (name, rc, err))

    def _stage(self, attr):
        """the named state of a stage (STAGES), or PbError("<stage> not switched on: call set_<stage>() first")"""
        if getattr(self, attr) is None:
            raise self._lp.PbError("%s not switched on: call %s() first" % STAGES[attr])
        return getattr(self, attr)

    def _timers(self, entry, names, *more):
        """a *_timers getter: the device ms that the library's `entry` fills in, under `names`"""
        t = (C.c_float * len(names))()
        entry(self._s, t, *more)
        return dict(zip(names, [float(v) for v in t]))

    def _codes_arg(self, codes, nbit, device_ptr, nsamp):
        """block_arg for packed codes, rows of nchan (4 nchan with polarisation on) samples of nbit bits"""
        return block_arg(codes, np.uint8, self.nchan * self._nif(), nbit, device_ptr, nsamp, "codes")

    def _planes(self, tout, want_series):
        """the outputs of run() / gulp_run() for tout samples: (the dict's arrays, their pointers in the library's order)"""
        out = dict(snr=np.empty((self.ndm, tout), np.float32), width_log2=np.empty((self.ndm, tout), np.uint8),
                   stats=np.empty((self.ndm, 2), np.float32), series=np.empty((self.ndm, tout), np.uint32) if want_series else None)
        return out, (out["snr"].ctypes.data_as(C.POINTER(C.c_float)), out["width_log2"].ctypes.data_as(C.POINTER(C.c_uint8)),
                     out["series"].ctypes.data_as(C.POINTER(C.c_uint32)) if want_series else None,
                     out["stats"].ctypes.data_as(C.POINTER(C.c_float)))

    def close(self):
        if getattr(self, "_s", None):
            self._L.pb_search_destroy(self._s)
            self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_baseline(self, window_samples):
        """running baseline over this many samples (heimdall: 2 s = 2560); 0 = one clipped mean per series"""
        rc = self._L.pb_search_set_baseline(self._s, int(window_samples))
        if rc != 0:
            raise ValueError("baseline window must be >= 0")

    def set_rfi(self, narrow=True, broad=True, tol=5.0, boxcar_max=16):
        """RFI cleaning of every following block before dedispersion (heimdall's narrow and broad stages, this
        project's own definition: include/pb_hip.h, pb_search_set_rfi); set_rfi(False, False) switches it off"""
        rc = self._L.pb_search_set_rfi(self._s, int(bool(narrow)), int(bool(broad)), float(tol), int(boxcar_max))
        self._check(rc, None, ValueError)

    def rfi_info(self):
        """the last run's cleaning: narrow flags, broad time samples, device ms (0 when it was not cleaned)"""
        n, b, ms = C.c_uint64(), C.c_int(), C.c_float()
        self._L.pb_search_rfi_info(self._s, C.byref(n), C.byref(b), C.byref(ms))
        return dict(n_narrow=int(n.value), n_broad_samples=int(b.value), ms=float(ms.value))

    def set_rfi_chan(self, radius=0, tol=4.0):
        """the cleaning's channel stage (include/pb_hip.h, pb_search_set_rfi_chan): of every following block the channels
        whose spread is an outlier among their neighbours' (lags up to radius; 0: a tenth of the unzapped channels) are
        filled with their rounded mean before the narrow and broad passes; tol=0 switches it off"""
        rc = self._L.pb_search_set_rfi_chan(self._s, int(radius), float(tol))
        self._check(rc, None, ValueError)
        self._rfichan = RfiChan(int(radius), float(tol)) if tol > 0 else None

    def rfi_chan_info(self):
        """the last block's channel stage: dict(nflag, mask u8, sum, stat i64, recv, cast i32, fill u8 -- [nchan], file
        channel numbering, 0 for zapped channels --, ms); all zero when the block did not go through the stage"""
        n, ms = C.c_int(), C.c_float()
        out = dict(mask=np.zeros(self.nchan, np.uint8), sum=np.zeros(self.nchan, np.int64), stat=np.zeros(self.nchan, np.int64),
                   recv=np.zeros(self.nchan, np.int32), cast=np.zeros(self.nchan, np.int32), fill=np.zeros(self.nchan, np.uint8))
        i64p, i32p, u8p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        rc = self._L.pb_search_rfi_chan_info(self._s, C.byref(n), out["mask"].ctypes.data_as(u8p), out["sum"].ctypes.data_as(i64p),
                                             out["stat"].ctypes.data_as(i64p), out["recv"].ctypes.data_as(i32p),
                                             out["cast"].ctypes.data_as(i32p), out["fill"].ctypes.data_as(u8p), C.byref(ms))
        self._check(rc, "pb_search_rfi_chan_info")
        out.update(nflag=int(n.value), ms=float(ms.value))
        return out

    def fetch_clean(self):
        """the last run's channel-major block [nchan][nsamp] u8 as dedispersion read it (cleaned if cleaning was on)"""
        out = np.empty((self.nchan, self._nsamp), np.uint8)
        rc = self._L.pb_search_fetch_clean(self._s, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.nbytes)
        self._check(rc, "pb_search_fetch_clean")
        return out

    def set_cutouts(self, nsub=64, nt=256, ndmrow=64, max_cands=32):
        """per-candidate cutouts of the last block (include/pb_hip.h, pb_search_set_cutouts): nsub subbands, nt time
        bins, ndmrow DM rows, up to max_cands requests per cutouts() call; max_cands=0 switches them off"""
        rc = self._L.pb_search_set_cutouts(self._s, int(nsub), int(nt), int(ndmrow), int(max_cands))
        self._check(rc, None, ValueError)
        self._cut = Cut(int(nsub), int(nt), int(ndmrow), int(max_cands)) if max_cands else None

    def cutouts(self, dmi, t, tscr):
        """Cutouts of the last block searched, one per request (dmi, t, tscr: scalars or equally long sequences; t in
        block coordinates, tscr a power of two in 1..64).  Returns dict(ft, ft_hits [n][nsub][nt] u32, dt, dt_hits
        [n][ndmrow][nt] u32, dm_rows [n][ndmrow] the DM of each row (NaN outside the grid), sub_freqs [nsub] the centre
        frequency of each subband in MHz).  Bin j covers the samples t + (j - nt/2) tscr .. + tscr."""
        nsub, nt, nrow, _ = self._stage("_cut")
        req = requests(np.int32, dmi, t, tscr)
        n = req.shape[0]
        out = dict(ft=np.zeros((n, nsub, nt), np.uint32), ft_hits=np.zeros((n, nsub, nt), np.uint32),
                   dt=np.zeros((n, nrow, nt), np.uint32), dt_hits=np.zeros((n, nrow, nt), np.uint32))
        u32p = C.POINTER(C.c_uint32)
        rc = self._L.pb_search_cutouts(self._s, req.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                       *[out[k].ctypes.data_as(u32p) for k in ("ft", "ft_hits", "dt", "dt_hits")])
        self._check(rc, "pb_search_cutouts")
        rows = req[:, :1].astype(np.int64) - nrow // 2 + np.arange(nrow)[None, :]
        ok = (rows >= 0) & (rows < self.ndm)
        out["dm_rows"] = np.where(ok, np.asarray(self.dms, np.float64)[np.clip(rows, 0, self.ndm - 1)], np.nan)
        per = self.nchan // nsub
        out["sub_freqs"] = self.fch1 + self.foff * (np.arange(nsub) * per + (per - 1) / 2.0)
        return out

    def cutout_timers(self):
        """device ms of the last cutouts() call: the kernels; the kernels and the copy to the host"""
        return self._timers(self._L.pb_search_cutout_timers, ("kernels", "with_copy"))

    def set_pol(self, off_len=64, guard=8, rm=(-2000.0, 2.0, 2001), max_cands=32):
        """polarisation of candidates (include/pb_hip.h, pb_search_set_pol): from now on run() and peaks() take blocks of
        [nsamp][4][nchan] 8-bit codes (AA, BB, CR, CI: a nifs 4 filterbank's rows) and search the rounded mean of AA and
        BB; pol() then gives on- and off-pulse spectra (off windows of off_len samples, guard samples away from the on
        window) and an RM synthesis over the trials rm = (first, step, how many), up to max_cands requests per call.
        max_cands=0 switches it off and returns the search to 1-IF blocks."""
        lo, step, nrm = float(rm[0]), float(rm[1]), int(rm[2])
        rc = self._L.pb_search_set_pol(self._s, int(off_len), int(guard), nrm, lo, step, int(max_cands))
        self._check(rc, None, ValueError)
        self._pol = Pol(int(off_len), int(guard), (lo, step, nrm), int(max_cands)) if max_cands else None

    def _nif(self):
        """rows of nchan codes per time sample of a block: 4 with polarisation on"""
        return 4 if self._pol is not None else 1

    def pol(self, dmi, t, w):
        """pb_search_pol on the last block searched, one request per element (scalars or equally long sequences): trial-DM
        index, peak sample in block coordinates, on-window length w in 1..64.  Returns dict(on, off [n][4][nchan] i32, non,
        noff [n][nchan] i32, F [n][nrm][2] f64 (re, im), kbest [n], summary [n][6] = W, lambda0^2, mean i, mean v,
        |F[kbest]|, RM of kbest; rms [nrm] the trial grid, freqs [nchan] in MHz)."""
        lo, step, nrm = self._stage("_pol").rm
        req = requests(np.int32, dmi, t, w)
        n = req.shape[0]
        out = dict(on=np.zeros((n, 4, self.nchan), np.int32), non=np.zeros((n, self.nchan), np.int32),
                   off=np.zeros((n, 4, self.nchan), np.int32), noff=np.zeros((n, self.nchan), np.int32),
                   F=np.full((n, nrm, 2), np.nan), kbest=np.full(n, -1, np.int32), summary=np.full((n, 6), np.nan))
        i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        rc = self._L.pb_search_pol(self._s, req.ctypes.data_as(i32p), n, out["on"].ctypes.data_as(i32p),
                                   out["non"].ctypes.data_as(i32p), out["off"].ctypes.data_as(i32p),
                                   out["noff"].ctypes.data_as(i32p), out["F"].ctypes.data_as(f64p),
                                   out["kbest"].ctypes.data_as(i32p), out["summary"].ctypes.data_as(f64p))
        self._check(rc, "pb_search_pol")
        out["rms"] = lo + step * np.arange(nrm)
        out["freqs"] = float(np.float32(self.fch1)) + float(np.float32(self.foff)) * np.arange(self.nchan)
        return out

    def pol_cutouts(self, dmi, t, tscr):
        """the four products' frequency-time images of the last block (set_cutouts() and set_pol() both on), requests as
        for cutouts(): dict(pft [n][4][nsub][nt] u32, pft_hits [n][nsub][nt] u32)"""
        if self._pol is None or self._cut is None:
            raise self._lp.PbError("pol_cutouts needs set_cutouts() and set_pol()")
        nsub, nt = self._cut.nsub, self._cut.nt
        req = requests(np.int32, dmi, t, tscr)
        n = req.shape[0]
        out = dict(pft=np.zeros((n, 4, nsub, nt), np.uint32), pft_hits=np.zeros((n, nsub, nt), np.uint32))
        u32p = C.POINTER(C.c_uint32)
        rc = self._L.pb_search_pol_cutouts(self._s, req.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                           out["pft"].ctypes.data_as(u32p), out["pft_hits"].ctypes.data_as(u32p))
        self._check(rc, "pb_search_pol_cutouts")
        return out

    def pol_fetch(self, which):
        """plane `which` (0..3 = AA, BB, CR, CI) of the last block, [nchan][nsamp] u8 as the file held it"""
        out = np.empty((self.nchan, self._nsamp), np.uint8)
        rc = self._L.pb_search_pol_fetch(self._s, int(which), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.nbytes)
        self._check(rc, "pb_search_pol_fetch")
        return out

    def pol_timers(self):
        """device ms of the last transposition into the five planes, of the last pol() call's kernels, and of those with
        the copy to the host"""
        return self._timers(self._L.pb_search_pol_timers, ("transpose", "kernels", "with_copy"))

    def set_refine(self, nstep=32, half_window=128, wmax=32, max_cands=32):
        """refinement of candidates on the last block (include/pb_hip.h, pb_search_set_refine): nstep fine trial DMs per
        request, a window of half_window samples either side of the peak, the odd widths below wmax, up to max_cands
        requests per refine_raw() call; max_cands=0 switches it off"""
        rc = self._L.pb_search_set_refine(self._s, int(nstep), int(half_window), int(wmax), int(max_cands))
        self._check(rc, None, ValueError)
        self._ref = Ref(int(nstep), int(half_window), int(wmax), int(max_cands)) if max_cands else None

    def refine_raw(self, t, width, dm_lo, dm_step, want_series=False):
        """pb_search_refine on the last block searched, one request per element (scalars or equally long sequences): peak
        sample t in block coordinates, width in 1..wmax (an even one counts as width + 1), fine trial k at
        float32(dm_lo) + k float32(dm_step).  Returns dict(status [n], sn_dm [n][nstep] f64 (NaN: trial outside the DM
        grid), kbest [n], opt_sn [n][wmax/2] f64, opt_loc [n][wmax/2], widths [wmax/2], dm_lo, dm_step [n] as rounded to binary32, dms [n][nstep] the trials' DMs,
        series? [n][nstep][2 (half_window + wmax/2)] u32)."""
        nstep, H, wmax, _ = self._stage("_ref")
        nw = wmax // 2
        ri = requests(np.int32, t, width)
        n = ri.shape[0]
        rf = np.ascontiguousarray(np.broadcast_to(requests(np.float32, dm_lo, dm_step), (n, 2)))
        out = dict(status=np.zeros(n, np.int32), sn_dm=np.full((n, nstep), np.nan), kbest=np.full(n, -1, np.int32),
                   opt_sn=np.full((n, nw), np.nan), opt_loc=np.full((n, nw), -1, np.int32))
        ser = np.zeros((n, nstep, 2 * (H + nw)), np.uint32) if want_series else None
        i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        rc = self._L.pb_search_refine(self._s, ri.ctypes.data_as(i32p), rf.ctypes.data_as(C.POINTER(C.c_float)), n,
                                      out["status"].ctypes.data_as(i32p), out["sn_dm"].ctypes.data_as(f64p),
                                      out["kbest"].ctypes.data_as(i32p), out["opt_sn"].ctypes.data_as(f64p),
                                      out["opt_loc"].ctypes.data_as(i32p),
                                      ser.ctypes.data_as(C.POINTER(C.c_uint32)) if want_series else None)
        self._check(rc, "pb_search_refine")
        out["widths"] = 2 * np.arange(nw) + 1
        out["dm_lo"], out["dm_step"] = rf[:, 0].astype(np.float64), rf[:, 1].astype(np.float64)
        out["dms"] = rf[:, :1].astype(np.float64) + np.arange(nstep)[None, :] * rf[:, 1:].astype(np.float64)
        if want_series:
            out["series"] = ser
        return out

    def refine_plan(self, dmi, width_log2):
        """pass 1 of refine() for a candidate at trial DM index dmi with boxcar 2^width_log2: (width, dm_lo, dm_step).  The
        fine trials span the grid DM +- the larger gap to its neighbours in the grid; the width is the candidate's,
        at most wmax."""
        nstep, _, wmax, _ = self._ref
        dms = np.asarray(self.dms, np.float64)
        gaps = [abs(dms[j] - dms[dmi]) for j in (dmi - 1, dmi + 1) if 0 <= j < dms.size]
        span = max(gaps) if gaps else 1.0
        return min(1 << int(width_log2), wmax), dms[dmi] - span, 2.0 * span / max(nstep - 1, 1)

    def refine(self, dmi, t, width_log2):
        """The reference's refinement of a candidate (analysis/loc_step0.py: refine_dm coarse, refine_dm fine,
        optimize_pulse) on the block that is still on the device, in two refine_raw() calls.  dmi, t, width_log2: a
        candidate's trial DM index, peak sample in block coordinates and log2 boxcar width, scalars or equally long
        sequences.  Pass 1: refine_plan().  Pass 2: centred on pass 1's best trial, +- two pass-1 steps.  Per candidate
        dict(dm, snr, width, peak, trials=[(dms, sns), (dms, sns)], opt_sn, opt_loc): the best fine DM of pass 2 and its
        S/N; width, and peak (block coordinates), from the largest opt_sn of pass 2's width pass.  None for a candidate
        whose window is too short or whose trials all lie outside the DM grid.  A scalar request returns one entry, a
        sequence a list."""
        ref = self._stage("_ref")
        nstep, H = ref.nstep, ref.half_window
        scalar = np.ndim(dmi) == 0
        dmi, t, wl = [np.asarray(v, np.int64) for v in np.broadcast_arrays(np.atleast_1d(dmi), np.atleast_1d(t), np.atleast_1d(width_log2))]
        plan = [self.refine_plan(int(d), int(w)) for d, w in zip(dmi, wl)]
        width, lo1, st1 = [np.array(v) for v in zip(*plan)]
        p1 = self.refine_raw(t, width, lo1, st1)
        k1 = np.maximum(p1["kbest"], 0)
        st1 = p1["dm_step"]                                             # the binary32 step that was used
        lo2 = p1["dms"][np.arange(len(t)), k1] - 2.0 * st1
        p2 = self.refine_raw(t, width, lo2, 4.0 * st1 / max(nstep - 1, 1))
        out = []
        for i in range(len(t)):
            if p1["status"][i] or p1["kbest"][i] < 0 or p2["kbest"][i] < 0:
                out.append(None)
                continue
            k2, iw = int(p2["kbest"][i]), int(np.argmax(p2["opt_sn"][i]))
            out.append(dict(dm=float(p2["dms"][i, k2]), snr=float(p2["sn_dm"][i, k2]), width=int(p2["widths"][iw]),
                            peak=int(max(0, t[i] - H) + p2["opt_loc"][i, iw]),
                            trials=[(p1["dms"][i], p1["sn_dm"][i]), (p2["dms"][i], p2["sn_dm"][i])],
                            opt_sn=p2["opt_sn"][i], opt_loc=p2["opt_loc"][i]))
        return out[0] if scalar else out

    def refine_timers(self):
        """device ms of the last refine_raw() call: the kernels; the kernels and the copy to the host"""
        return self._timers(self._L.pb_search_refine_timers, ("kernels", "with_copy"))

    def set_subbands(self, nsb=8, bands=None, dm_chunk=0, max_points=1 << 18):
        """the sub-band search for band-limited bursts (include/pb_hip.h, pb_search_set_subbands): nsb base sub-bands (2, 4,
        8 or 16), bands a list of (first, count) runs of them (None: subband_list(nsb)), the trial DMs processed dm_chunk at
        a time (0: what keeps the stage within 1 GiB), up to max_points points per subbands() call; nsb=0 or an empty band
        list switches the stage off"""
        bands = subband_list(nsb) if (bands is None and nsb) else [(int(f), int(c)) for f, c in (bands or [])]
        if not nsb:
            bands = []
        b2 = np.ascontiguousarray(np.asarray(bands, np.int32).reshape(-1, 2))
        rc = self._L.pb_search_set_subbands(self._s, int(nsb), b2.ctypes.data_as(C.POINTER(C.c_int32)), len(bands),
                                            int(dm_chunk), int(max_points))
        self._check(rc, None, ValueError)
        self._sub = Sub(int(nsb), bands, int(max_points)) if bands else None

    def subbands(self, thresh, t_lo=0, t_hi=None):
        """pb_search_subbands on the block and planes of the last run() / peaks() / gulp search, samples [t_lo, t_hi) (t_hi
        None: to the end): the cells where a band's S/N is >= thresh and above the full band's.  Returns dict(dmi, t, snr f32,
        width_log2, band (index into the band list), snr_full f32 -- one entry per point, order unspecified --, npoints,
        overflow); after an overflow (npoints > max_points) the arrays hold the first max_points points that arrived."""
        cap = self._stage("_sub").max_points
        if t_hi is None:
            t_hi = self._tout
        buf = np.empty((cap, 6), np.int32)
        n, ov = C.c_int(), C.c_int()
        rc = self._L.pb_search_subbands(self._s, C.c_float(thresh), int(t_lo), int(t_hi), buf.ctypes.data_as(C.POINTER(C.c_int32)),
                                        cap, C.byref(n), C.byref(ov))
        self._check(rc, "pb_search_subbands")
        b = buf[:min(n.value, cap)]
        return dict(dmi=b[:, 0].copy(), t=b[:, 1].copy(), snr=b[:, 2].copy().view(np.float32), width_log2=b[:, 3].astype(np.uint8),
                    band=b[:, 4].copy(), snr_full=b[:, 5].copy().view(np.float32), npoints=n.value, overflow=bool(ov.value))

    def subband_dm(self, dmi):
        """one trial DM of the current block through the sub-band kernels (tests, diagnostics): dict(sub [nsb][tout] u32,
        band_snr f32, band_wid u8 [nbands][tout], band_stats [nbands][2], best_snr f32, best_wid, best_band u8 [tout])"""
        sub = self._stage("_sub")
        nsb, nb, tout = sub.nsb, len(sub.bands), self._tout
        out = dict(sub=np.zeros((nsb, tout), np.uint32), band_snr=np.zeros((nb, tout), np.float32),
                   band_wid=np.zeros((nb, tout), np.uint8), band_stats=np.zeros((nb, 2), np.float32),
                   best_snr=np.zeros(tout, np.float32), best_wid=np.zeros(tout, np.uint8), best_band=np.zeros(tout, np.uint8))
        fp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        rc = self._L.pb_search_subband_dm(self._s, int(dmi), out["sub"].ctypes.data_as(C.POINTER(C.c_uint32)),
                                          out["band_snr"].ctypes.data_as(fp), out["band_wid"].ctypes.data_as(u8p),
                                          out["band_stats"].ctypes.data_as(fp), out["best_snr"].ctypes.data_as(fp),
                                          out["best_wid"].ctypes.data_as(u8p), out["best_band"].ctypes.data_as(u8p))
        self._check(rc, "pb_search_subband_dm")
        return out

    def subband_timers(self):
        """device ms of the last subbands() call: the sub-band dedispersion; band sums, prefix sums and statistics; boxcars
        and best band; everything with the copy to the host"""
        return self._timers(self._L.pb_search_subband_timers, ("dedisperse", "stats", "boxcar", "with_copy"))

    def set_periodic(self, bins=64, k_lo=0, k_hi=0, dm_chunk=0):
        """the periodicity search (include/pb_hip.h, pb_search_set_periodic): profiles of bins .. 2 bins - 1 bins (bins 32, 64
        or 128) at the octaves k_lo .. k_hi (series summed in 2^k samples), the trial DMs processed dm_chunk at a time (0: what
        keeps the stage's scratch within 1 GiB); bins=0 switches the stage off"""
        rc = self._L.pb_search_set_periodic(self._s, int(bins), int(k_lo), int(k_hi), int(dm_chunk))
        self._check(rc, None, ValueError)
        self._per = Per(int(bins), int(k_lo), int(k_hi)) if bins else None

    def periodic_rows(self, k, p):
        """(m, M) of base period p at octave k for the last block searched: rows folded, and trials (0: skipped)"""
        m = (self._tsearch >> int(k)) // int(p)
        return m, (1 << int(m - 1).bit_length()) if m >= 2 else 0

    def periodic(self):
        """pb_search_periodic on the series of the last run() / peaks() / gulp search: the best trial of every trial DM,
        octave and base period.  Returns dict(snr f32, i, q, j i32, m, M i32, period_s f64 -- all [ndm][nk][bins], the entry
        of base period p at p - bins; octaves [nk], p [bins]).  A skipped base period has snr 0, i -1 and period_s NaN;
        m, M and period_s = (p + i / (M - 1)) 2^k tsamp are made on the host."""
        B, k_lo, k_hi = self._stage("_per")
        nk = k_hi - k_lo + 1
        buf = np.empty((self.ndm, nk, B, 4), np.int32)
        rc = self._L.pb_search_periodic(self._s, buf.ctypes.data_as(C.POINTER(C.c_int32)))
        self._check(rc, "pb_search_periodic")
        ks, ps = np.arange(k_lo, k_hi + 1), np.arange(B, 2 * B)
        mM = np.array([[self.periodic_rows(k, p) for p in ps] for k in ks], np.int32)
        m, M = [np.broadcast_to(mM[None, :, :, c], buf.shape[:3]).copy() for c in (0, 1)]
        i = buf[..., 1].copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            per = (ps[None, None, :] + i / (M - 1.0)) * (2.0 ** ks)[None, :, None] * self.tsamp
        return dict(snr=buf[..., 0].copy().view(np.float32), i=i, q=buf[..., 2].copy(), j=buf[..., 3].copy(), m=m, M=M,
                    period_s=np.where(i >= 0, per, np.nan), octaves=ks, p=ps)

    def periodic_fold(self, dmi, k, p):
        """one (trial DM, octave, base period) in full (tests; the profile of a candidate): dict(m, M, prof [M][p] u32, snr
        [M][Q + 1] f32, jbest [M][Q + 1] i32, widths [Q + 1]); a skipped base period gives M = 0 and empty arrays"""
        B = self._stage("_per").bins
        nq = int(B // 2).bit_length()
        m, Mo = C.c_int(), C.c_int()
        rc = self._L.pb_search_periodic_fold(self._s, int(dmi), int(k), int(p), None, None, None, C.byref(m), C.byref(Mo))
        self._check(rc, "pb_search_periodic_fold")             # (no output asked for: the sizes only, nothing launched)
        M = Mo.value
        out = dict(prof=np.zeros((M, int(p)), np.uint32), snr=np.zeros((M, nq), np.float32), jbest=np.zeros((M, nq), np.int32))
        rc = self._L.pb_search_periodic_fold(self._s, int(dmi), int(k), int(p), out["prof"].ctypes.data_as(C.POINTER(C.c_uint32)),
                                             out["snr"].ctypes.data_as(C.POINTER(C.c_float)),
                                             out["jbest"].ctypes.data_as(C.POINTER(C.c_int32)), C.byref(m), C.byref(Mo))
        self._check(rc, "pb_search_periodic_fold")
        return dict(out, m=m.value, M=M, widths=1 << np.arange(nq))

    def periodic_timers(self):
        """device ms of the last periodic() call: the folding; the last stage and the evaluation; everything with the copy"""
        return self._timers(self._L.pb_search_periodic_timers, ("fold", "eval", "with_copy"))

    def set_giants(self, sep_time=3, sep_dm=200, sep_filter=3, max_giants=1 << 18):
        """giants and clusters of giants on the device (include/pb_hip.h, pb_search_set_giants): hot samples of a series
        at most sep_time apart make a giant, giants within sep_dm trial DMs, sep_filter in log2 width and sep_time in time
        are linked, up to max_giants giants per giants() call; max_giants=0 switches the stage off"""
        rc = self._L.pb_search_set_giants(self._s, int(sep_time), int(sep_dm), int(sep_filter), int(max_giants))
        self._check(rc, None, ValueError)
        self._gi = Gi(int(sep_time), int(sep_dm), int(sep_filter), int(max_giants)) if max_giants else None

    def set_planes(self, snr, width_log2):
        """replace the S/N and log2-width planes on the device with host planes [ndm][tout] (stored planes clustered
        again; hand-made patterns for tests); giants() then acts on them"""
        snr = np.ascontiguousarray(snr, np.float32)
        wl = np.ascontiguousarray(width_log2, np.uint8)
        if snr.ndim != 2 or snr.shape[0] != self.ndm or wl.shape != snr.shape:
            raise ValueError("set_planes: both planes must be [ndm][tout]")
        rc = self._L.pb_search_set_planes(self._s, snr.ctypes.data_as(C.POINTER(C.c_float)),
                                          wl.ctypes.data_as(C.POINTER(C.c_uint8)), snr.shape[1])
        self._check(rc, None, ValueError)
        self._tout = snr.shape[1]

    def giants(self, thresh, t_lo=0, t_hi=None, want_list=False):
        """pb_search_giants on the planes of the last run()/peaks() (or set_planes()), samples [t_lo, t_hi) (t_hi None: to
        the planes' end).  Returns dict(snr f32, peak, tfilt, dmi, members, npoints, i0, i1 -- one entry per cluster, in
        label order --, ngiants, overflow; with want_list also giant_list = dict(dmi, begin, end, npts, peak, snr, tfilt,
        label), ascending (dmi, begin)).  After an overflow (ngiants > max_giants) every array is empty."""
        cap = self._stage("_gi").max_giants
        if t_hi is None:
            t_hi = self._tout
        i32p, ip = C.POINTER(C.c_int32), C.POINTER(C.c_int)
        nc, ng, ov = C.c_int(), C.c_int(), C.c_int()
        buf = np.empty((cap, 8), np.int32)
        rc = self._L.pb_search_giants(self._s, C.c_float(thresh), int(t_lo), int(t_hi), buf.ctypes.data_as(i32p), cap,
                                      C.byref(nc), C.byref(ng), C.byref(ov))
        self._check(rc, "pb_search_giants")
        b = buf[:nc.value]
        out = dict(snr=b[:, 0].copy().view(np.float32), peak=b[:, 1].copy(), tfilt=b[:, 2].copy(), dmi=b[:, 3].copy(),
                   members=b[:, 4].copy(), npoints=b[:, 5].copy(), i0=b[:, 6].copy(), i1=b[:, 7].copy(),
                   ngiants=ng.value, overflow=bool(ov.value))
        if want_list:
            n = C.c_int()
            g = np.empty((0 if ov.value else ng.value, 8), np.int32)
            rc = self._L.pb_search_giant_list(self._s, g.ctypes.data_as(i32p), g.shape[0], C.byref(n))
            self._check(rc, "pb_search_giant_list")
            out["giant_list"] = dict(dmi=g[:, 0].copy(), begin=g[:, 1].copy(), end=g[:, 2].copy(), npts=g[:, 3].copy(),
                                     peak=g[:, 4].copy(), snr=g[:, 5].copy().view(np.float32), tfilt=g[:, 6].copy(),
                                     label=g[:, 7].copy())
        return out

    def giant_timers(self):
        """the last giants() call: device ms of the giant pass, of the labelling and merge, of everything with the copy;
        and the labelling's sweeps"""
        n = C.c_int()
        return dict(self._timers(self._L.pb_search_giant_timers, ("giants", "label", "with_copy"), C.byref(n)), sweeps=int(n.value))

    def timers(self):
        """device ms of the last run's stages"""
        return self._timers(self._L.pb_search_timers, ("h2d", "transpose", "dedisperse", "stats", "boxcar", "d2h"))

    def peaks(self, codes, threshold, nbit=8, device_ptr=None, nsamp=None, max_out=1 << 18):
        """Search one block and return only the (DM, sample) points with S/N >= threshold:
        dict(dmi, t, snr, width_log2, total).  codes: host uint8 array, or device_ptr + nsamp for codes that
        are already on the GPU (e.g. PbHandle.output_dev)."""
        # (a host array counts as long as it is, whatever nsamp says)
        ptr, on_dev, nsamp, keep = self._codes_arg(codes, nbit, device_ptr, nsamp if device_ptr is not None else None)
        buf = np.empty((max_out, 4), np.int32)
        n, t = C.c_int(), C.c_int()
        rc = self._L.pb_search_peaks(self._s, ptr, on_dev, nsamp, nbit, C.c_float(threshold),
                                     buf.ctypes.data_as(C.POINTER(C.c_int32)), max_out, C.byref(n), C.byref(t))
        self._check(rc, "pb_search_peaks")
        self._nsamp = nsamp
        self._tout = self._tsearch = t.value
        return peak_dict(buf, n.value, t.value, max_out)

    def set_gulp(self, keep_max):
        """streaming (include/pb_hip.h, pb_search_set_gulp): pieces pushed with push() accumulate in the search's block on
        the device, gulp_peaks() / gulp_run() search what has accumulated, gulp_advance(keep) hands its last keep <=
        keep_max samples on to the next gulp without leaving the device; keep_max=0 switches the stage off"""
        rc = self._L.pb_search_set_gulp(self._s, int(keep_max))
        self._check(rc, None, ValueError)

    def push(self, codes=None, nbit=8, device_ptr=None, nsamp=None):
        """append a piece to the accumulated block: a host uint8 array of nsamp x nchan samples of nbit bits (SIGPROC
        order), or device_ptr + nsamp for bytes that are already on the GPU (the contract of run()).  Returns the
        block's new length in samples."""
        ptr, on_dev, nsamp, keep = self._codes_arg(codes, nbit, device_ptr, nsamp)
        fill = C.c_int()
        rc = self._L.pb_search_push(self._s, ptr, on_dev, nsamp, int(nbit), C.byref(fill))
        self._check(rc, "pb_search_push")
        return fill.value

    def push_plane(self, plane=None, device_ptr=None, nsamp=None, scale=1.0):
        """append a piece of an fp32 plane [nsamp][nchan], quantised to 8 bits with the reference's rule on the device
        (include/pb_hip.h, pb_search_push_f32: q = trunc(float(double(x * scale) / 0.02957 + 127.5)) clamped to 0..255,
        NaN -> 0): a host float32 array, or device_ptr + nsamp for floats that are already on the GPU (PbHandle.output_dev's
        `ave` with keep_ave, a coadder's sum with scale = float32(1 / sqrt(N)); the contract of run(), the address a
        multiple of 4).  Returns the block's new length in samples."""
        ptr, on_dev, nsamp, keep = block_arg(plane, np.float32, self.nchan, 32, device_ptr, nsamp, "plane")
        fill = C.c_int()
        rc = self._L.pb_search_push_f32(self._s, ptr, on_dev, nsamp, C.c_float(float(scale)), C.byref(fill))
        self._check(rc, "pb_search_push_f32")
        return fill.value

    def gulp_peaks(self, threshold, max_out=1 << 18):
        """peaks() on the accumulated block: the same dict"""
        buf = np.empty((max_out, 4), np.int32)
        n, t = C.c_int(), C.c_int()
        rc = self._L.pb_search_gulp_peaks(self._s, C.c_float(threshold), buf.ctypes.data_as(C.POINTER(C.c_int32)), max_out,
                                          C.byref(n), C.byref(t))
        self._check(rc, "pb_search_gulp_peaks")
        self._nsamp = t.value + self.max_delay
        self._tout = self._tsearch = t.value
        return peak_dict(buf, n.value, t.value, max_out)

    def gulp_run(self, want_series=False):
        """run() on the accumulated block: the same dict"""
        fill = self.gulp_fill()
        out, ptrs = self._planes(max(fill - self.max_delay, 1), want_series)
        t = C.c_int()
        rc = self._L.pb_search_gulp_run(self._s, *ptrs, C.byref(t))
        self._check(rc, "pb_search_gulp_run")
        self._nsamp = fill
        self._tout = self._tsearch = t.value
        return dict(out, tout=t.value)

    def gulp_fill(self):
        """samples per channel in the accumulated block"""
        fill = C.c_int()
        rc = self._L.pb_search_push(self._s, None, 0, 0, 8, C.byref(fill))
        self._check(rc, "pb_search_push")
        return fill.value

    def gulp_advance(self, keep):
        """the last `keep` raw samples of the accumulated block become its first, the rest is dropped"""
        rc = self._L.pb_search_gulp_advance(self._s, int(keep))
        self._check(rc, "pb_search_gulp_advance")

    def gulp_fetch(self):
        """the raw accumulated block [nchan][fill] u8"""
        out = np.empty((self.nchan, self.gulp_fill()), np.uint8)
        fill = C.c_int()
        rc = self._L.pb_search_gulp_fetch(self._s, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.nbytes, C.byref(fill))
        self._check(rc, "pb_search_gulp_fetch")
        return out

    def gulp_timers(self):
        """device ms of the last push(): copy to the device, append; and of the last gulp_advance()"""
        return self._timers(self._L.pb_search_gulp_timers, ("copy", "append", "advance"))

    def run(self, codes, nbit=8, want_series=False, device_ptr=None, nsamp=None):
        """codes: uint8 array holding nsamp x nchan samples of nbit bits (SIGPROC order; with set_pol() on nsamp x 4 x nchan
        8-bit codes, and nsamp counts 4 nchan bytes per sample), or device_ptr + nsamp for
        codes that are already on the GPU (e.g. PbHandle.output_dev; the contract is under pb_search_run in
        include/pb_hip.h: the producer's stream synchronised, any byte address, valid until this returns).
        Returns dict(snr [ndm][tout] f32, width_log2 [ndm][tout] u8, stats [ndm][2], series?)."""
        # (a host array counts as long as it is, whatever nsamp says)
        ptr, on_dev, nsamp, keep = self._codes_arg(codes, nbit, device_ptr, nsamp if device_ptr is not None else None)
        tout = nsamp - self.max_delay
        if tout < 64:
            raise ValueError("block shorter than the largest dispersion delay (%d samples)" % self.max_delay)
        out, ptrs = self._planes(tout, want_series)
        t = C.c_int()
        rc = self._L.pb_search_run(self._s, ptr, on_dev, nsamp, nbit, *ptrs, C.byref(t))
        self._check(rc, "pb_search_run")
        self._nsamp = nsamp
        self._tout = self._tsearch = tout
        return dict(out, tout=tout)

