"""Dedispersion + boxcar search on a filterbank block, and heimdall-style candidate lines.

Stands where the external `heimdall_stream` stands in the reference's chain
(/root/reference/scripts/start_heimdall_single_antenna:21; candidate line columns
`S/N, peak_idx, peak_time, tfilt, dmi, dm, ngiant, i0, i1` as parsed by src/candidate.py:8-18).
The GPU work is libpb_hip.so's pb_search_* (csrc/search_*.hip); this module only drives it and
groups the above-threshold samples into candidates on the host.  heimdall is third-party and not in
the image: its DM spacing, baseline removal and giant merging are not reproduced -- parity with its
candidate list is unpinned.
"""
import ctypes as C
import importlib

import numpy as np

_pkg = __package__ or "vlite-fast_amd"

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


class Searcher(object):
    def __init__(self, device=0, nchan=4096, max_samples=HEIMDALL_GULP, fch1=FCH1, foff=FOFF, tsamp=TSAMP,
                 dm_min=HEIMDALL_DM[0], dm_max=HEIMDALL_DM[1], dm_step=2.0, boxcar_max=HEIMDALL_BOXCAR_MAX,
                 zap=HEIMDALL_ZAP, dm_list=None):
        """dm_list: explicit trial DMs (e.g. dedisp_dm_list(...)); default the linear grid dm_min..dm_max"""
        lp = importlib.import_module(_pkg + ".libpb")
        self._lp = lp
        self._L = lp.load()
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
        self._cut = None                 # (nsub, nt, ndmrow, max_cands) once set_cutouts has switched them on
        self._ref = None                 # (nstep, half_window, wmax, max_cands) once set_refine has switched it on
        self._gi = None                  # (sep_time, sep_dm, sep_filter, max_giants) once set_giants has switched it on
        self._pol = None                 # (off_len, guard, (rm_lo, rm_step, nrm), max_cands) once set_pol has switched it on
        self._sub = None                 # (nsb, [(first, count), ..], max_points) once set_subbands has switched it on
        self._rfichan = None             # (radius, tol) once set_rfi_chan has switched the channel stage on
        self.dms = dm_min + dm_step * np.arange(self.ndm) if dm_list is None else np.asarray(dm_list, np.float64)
        self._nsamp = 0
        self._tout = 0

    def _check(self, rc, name, exc=None, handle=True):
        """raise for a non-zero return code: PbError("<name> failed (rc): <last error>"), or exc(<last error>)"""
        if rc != 0:
            err = self._L.pb_search_last_error(self._s if handle else None).decode()
            raise exc(err) if exc else self._lp.PbError("%s failed (%d): %s" % (name, rc, err))

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
        self._rfichan = (int(radius), float(tol)) if tol > 0 else None

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
        self._cut = (int(nsub), int(nt), int(ndmrow), int(max_cands)) if max_cands else None

    def cutouts(self, dmi, t, tscr):
        """Cutouts of the last block searched, one per request (dmi, t, tscr: scalars or equally long sequences; t in
        block coordinates, tscr a power of two in 1..64).  Returns dict(ft, ft_hits [n][nsub][nt] u32, dt, dt_hits
        [n][ndmrow][nt] u32, dm_rows [n][ndmrow] the DM of each row (NaN outside the grid), sub_freqs [nsub] the centre
        frequency of each subband in MHz).  Bin j covers the samples t + (j - nt/2) tscr .. + tscr."""
        if self._cut is None:
            raise self._lp.PbError("cutouts are not switched on: call set_cutouts() first")
        nsub, nt, nrow, _ = self._cut
        req = np.stack(np.broadcast_arrays(np.atleast_1d(dmi), np.atleast_1d(t), np.atleast_1d(tscr)), axis=1)
        req = np.ascontiguousarray(req, np.int32)
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
        t = (C.c_float * 2)()
        self._L.pb_search_cutout_timers(self._s, t)
        return dict(kernels=float(t[0]), with_copy=float(t[1]))

    def set_pol(self, off_len=64, guard=8, rm=(-2000.0, 2.0, 2001), max_cands=32):
        """polarisation of candidates (include/pb_hip.h, pb_search_set_pol): from now on run() and peaks() take blocks of
        [nsamp][4][nchan] 8-bit codes (AA, BB, CR, CI: a nifs 4 filterbank's rows) and search the rounded mean of AA and
        BB; pol() then gives on- and off-pulse spectra (off windows of off_len samples, guard samples away from the on
        window) and an RM synthesis over the trials rm = (first, step, how many), up to max_cands requests per call.
        max_cands=0 switches it off and returns the search to 1-IF blocks."""
        lo, step, nrm = float(rm[0]), float(rm[1]), int(rm[2])
        rc = self._L.pb_search_set_pol(self._s, int(off_len), int(guard), nrm, lo, step, int(max_cands))
        self._check(rc, None, ValueError)
        self._pol = (int(off_len), int(guard), (lo, step, nrm), int(max_cands)) if max_cands else None

    def _nif(self):
        """rows of nchan codes per time sample of a block: 4 with polarisation on"""
        return 4 if self._pol is not None else 1

    def pol(self, dmi, t, w):
        """pb_search_pol on the last block searched, one request per element (scalars or equally long sequences): trial-DM
        index, peak sample in block coordinates, on-window length w in 1..64.  Returns dict(on, off [n][4][nchan] i32, non,
        noff [n][nchan] i32, F [n][nrm][2] f64 (re, im), kbest [n], summary [n][6] = W, lambda0^2, mean i, mean v,
        |F[kbest]|, RM of kbest; rms [nrm] the trial grid, freqs [nchan] in MHz)."""
        if self._pol is None:
            raise self._lp.PbError("polarisation is not switched on: call set_pol() first")
        lo, step, nrm = self._pol[2]
        req = np.stack(np.broadcast_arrays(np.atleast_1d(dmi), np.atleast_1d(t), np.atleast_1d(w)), axis=1)
        req = np.ascontiguousarray(req, np.int32)
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
        nsub, nt, _, _ = self._cut
        req = np.stack(np.broadcast_arrays(np.atleast_1d(dmi), np.atleast_1d(t), np.atleast_1d(tscr)), axis=1)
        req = np.ascontiguousarray(req, np.int32)
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
        t = (C.c_float * 3)()
        self._L.pb_search_pol_timers(self._s, t)
        return dict(transpose=float(t[0]), kernels=float(t[1]), with_copy=float(t[2]))

    def set_refine(self, nstep=32, half_window=128, wmax=32, max_cands=32):
        """refinement of candidates on the last block (include/pb_hip.h, pb_search_set_refine): nstep fine trial DMs per
        request, a window of half_window samples either side of the peak, the odd widths below wmax, up to max_cands
        requests per refine_raw() call; max_cands=0 switches it off"""
        rc = self._L.pb_search_set_refine(self._s, int(nstep), int(half_window), int(wmax), int(max_cands))
        self._check(rc, None, ValueError)
        self._ref = (int(nstep), int(half_window), int(wmax), int(max_cands)) if max_cands else None

    def refine_raw(self, t, width, dm_lo, dm_step, want_series=False):
        """pb_search_refine on the last block searched, one request per element (scalars or equally long sequences): peak
        sample t in block coordinates, width in 1..wmax (an even one counts as width + 1), fine trial k at
        float32(dm_lo) + k float32(dm_step).  Returns dict(status [n], sn_dm [n][nstep] f64 (NaN: trial outside the DM
        grid), kbest [n], opt_sn [n][wmax/2] f64, opt_loc [n][wmax/2], widths [wmax/2], dm_lo, dm_step [n] as rounded to binary32, dms [n][nstep] the trials' DMs,
        series? [n][nstep][2 (half_window + wmax/2)] u32)."""
        if self._ref is None:
            raise self._lp.PbError("refinement is not switched on: call set_refine() first")
        nstep, H, wmax, _ = self._ref
        nw = wmax // 2
        ri = np.stack(np.broadcast_arrays(np.atleast_1d(t), np.atleast_1d(width)), axis=1)
        ri = np.ascontiguousarray(ri, np.int32)
        n = ri.shape[0]
        rf = np.stack(np.broadcast_arrays(np.atleast_1d(dm_lo), np.atleast_1d(dm_step)), axis=1)
        rf = np.ascontiguousarray(np.broadcast_to(rf, (n, 2)), np.float32)
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
        if self._ref is None:
            raise self._lp.PbError("refinement is not switched on: call set_refine() first")
        nstep, H, _, _ = self._ref
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
        t = (C.c_float * 2)()
        self._L.pb_search_refine_timers(self._s, t)
        return dict(kernels=float(t[0]), with_copy=float(t[1]))

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
        self._sub = (int(nsb), bands, int(max_points)) if bands else None

    def subbands(self, thresh, t_lo=0, t_hi=None):
        """pb_search_subbands on the block and planes of the last run() / peaks() / gulp search, samples [t_lo, t_hi) (t_hi
        None: to the end): the cells where a band's S/N is >= thresh and above the full band's.  Returns dict(dmi, t, snr f32,
        width_log2, band (index into the band list), snr_full f32 -- one entry per point, order unspecified --, npoints,
        overflow); after an overflow (npoints > max_points) the arrays hold the first max_points points that arrived."""
        if self._sub is None:
            raise self._lp.PbError("the sub-band search is not switched on: call set_subbands() first")
        if t_hi is None:
            t_hi = self._tout
        cap = self._sub[2]
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
        if self._sub is None:
            raise self._lp.PbError("the sub-band search is not switched on: call set_subbands() first")
        nsb, nb, tout = self._sub[0], len(self._sub[1]), self._tout
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
        t = (C.c_float * 4)()
        self._L.pb_search_subband_timers(self._s, t)
        return dict(zip(("dedisperse", "stats", "boxcar", "with_copy"), [float(v) for v in t]))

    def set_giants(self, sep_time=3, sep_dm=200, sep_filter=3, max_giants=1 << 18):
        """giants and clusters of giants on the device (include/pb_hip.h, pb_search_set_giants): hot samples of a series
        at most sep_time apart make a giant, giants within sep_dm trial DMs, sep_filter in log2 width and sep_time in time
        are linked, up to max_giants giants per giants() call; max_giants=0 switches the stage off"""
        rc = self._L.pb_search_set_giants(self._s, int(sep_time), int(sep_dm), int(sep_filter), int(max_giants))
        self._check(rc, None, ValueError)
        self._gi = (int(sep_time), int(sep_dm), int(sep_filter), int(max_giants)) if max_giants else None

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
        if self._gi is None:
            raise self._lp.PbError("giants are not switched on: call set_giants() first")
        if t_hi is None:
            t_hi = self._tout
        cap = self._gi[3]
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
        t, n = (C.c_float * 3)(), C.c_int()
        self._L.pb_search_giant_timers(self._s, t, C.byref(n))
        return dict(giants=float(t[0]), label=float(t[1]), with_copy=float(t[2]), sweeps=int(n.value))

    def timers(self):
        """device ms of the last run's stages"""
        t = (C.c_float * 6)()
        self._L.pb_search_timers(self._s, t)
        return dict(zip(("h2d", "transpose", "dedisperse", "stats", "boxcar", "d2h"), [float(v) for v in t]))

    def peaks(self, codes, threshold, nbit=8, device_ptr=None, nsamp=None, max_out=1 << 18):
        """Search one block and return only the (DM, sample) points with S/N >= threshold:
        dict(dmi, t, snr, width_log2, total).  codes: host uint8 array, or device_ptr + nsamp for codes that
        are already on the GPU (e.g. PbHandle.output_dev)."""
        if device_ptr is None:
            codes = np.ascontiguousarray(codes, np.uint8).ravel()
            nsamp = codes.size * (8 // nbit) // (self.nchan * self._nif())
            ptr, on_dev = codes.ctypes.data_as(C.c_void_p), 0
        else:
            if nsamp is None:
                raise ValueError("device_ptr needs nsamp")
            nsamp = int(nsamp)
            ptr, on_dev = C.c_void_p(device_ptr), 1
        buf = np.empty((max_out, 4), np.int32)
        n, t = C.c_int(), C.c_int()
        rc = self._L.pb_search_peaks(self._s, ptr, on_dev, nsamp, nbit, C.c_float(threshold),
                                     buf.ctypes.data_as(C.POINTER(C.c_int32)), max_out, C.byref(n), C.byref(t))
        self._check(rc, "pb_search_peaks")
        self._nsamp = nsamp
        self._tout = t.value
        k = min(n.value, max_out, 1 << 20)        # (the device list holds 2^20 points)
        b = buf[:k]
        return dict(dmi=b[:, 0].copy(), t=b[:, 1].copy(), snr=b[:, 2].copy().view(np.float32), width_log2=b[:, 3].astype(np.uint8),
                    total=n.value, tout=t.value)

    def set_gulp(self, keep_max):
        """streaming (include/pb_hip.h, pb_search_set_gulp): pieces pushed with push() accumulate in the search's block on
        the device, gulp_peaks() / gulp_run() search what has accumulated, gulp_advance(keep) hands its last keep <=
        keep_max samples on to the next gulp without leaving the device; keep_max=0 switches the stage off"""
        rc = self._L.pb_search_set_gulp(self._s, int(keep_max))
        self._check(rc, None, ValueError)

    def _codes_arg(self, codes, nbit, device_ptr, nsamp):
        """(pointer, codes_on_device, nsamp, what keeps the host bytes alive) of a host array or a device address"""
        if device_ptr is None:
            codes = np.ascontiguousarray(codes, np.uint8).ravel()
            if nsamp is None:
                nsamp = codes.size * 8 // (nbit * self.nchan) if nbit in (8, 4, 2) else 0
            elif codes.size * 8 < int(nsamp) * self.nchan * nbit:
                raise ValueError("codes holds fewer than nsamp samples")
            return codes.ctypes.data_as(C.c_void_p), 0, int(nsamp), codes
        if nsamp is None:
            raise ValueError("device_ptr needs nsamp")
        return C.c_void_p(device_ptr), 1, int(nsamp), None

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
        if device_ptr is None:
            plane = np.ascontiguousarray(plane, np.float32).ravel()
            if nsamp is None:
                nsamp = plane.size // self.nchan
            elif plane.size < int(nsamp) * self.nchan:
                raise ValueError("plane holds fewer than nsamp samples")
            ptr, on_dev = plane.ctypes.data_as(C.c_void_p), 0
        else:
            if nsamp is None:
                raise ValueError("device_ptr needs nsamp")
            ptr, on_dev = C.c_void_p(device_ptr), 1
        fill = C.c_int()
        rc = self._L.pb_search_push_f32(self._s, ptr, on_dev, int(nsamp), C.c_float(float(scale)), C.byref(fill))
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
        self._tout = t.value
        b = buf[:min(n.value, max_out, 1 << 20)]
        return dict(dmi=b[:, 0].copy(), t=b[:, 1].copy(), snr=b[:, 2].copy().view(np.float32), width_log2=b[:, 3].astype(np.uint8),
                    total=n.value, tout=t.value)

    def gulp_run(self, want_series=False):
        """run() on the accumulated block: the same dict"""
        fill = self.gulp_fill()
        tout = max(fill - self.max_delay, 1)
        snr = np.empty((self.ndm, tout), np.float32)
        wid = np.empty((self.ndm, tout), np.uint8)
        stats = np.empty((self.ndm, 2), np.float32)
        series = np.empty((self.ndm, tout), np.uint32) if want_series else None
        t = C.c_int()
        rc = self._L.pb_search_gulp_run(self._s, snr.ctypes.data_as(C.POINTER(C.c_float)), wid.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        series.ctypes.data_as(C.POINTER(C.c_uint32)) if want_series else None,
                                        stats.ctypes.data_as(C.POINTER(C.c_float)), C.byref(t))
        self._check(rc, "pb_search_gulp_run")
        self._nsamp = fill
        self._tout = t.value
        return dict(snr=snr, width_log2=wid, stats=stats, series=series, tout=t.value)

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
        t = (C.c_float * 3)()
        self._L.pb_search_gulp_timers(self._s, t)
        return dict(copy=float(t[0]), append=float(t[1]), advance=float(t[2]))

    def run(self, codes, nbit=8, want_series=False, device_ptr=None, nsamp=None):
        """codes: uint8 array holding nsamp x nchan samples of nbit bits (SIGPROC order; with set_pol() on nsamp x 4 x nchan
        8-bit codes, and nsamp counts 4 nchan bytes per sample), or device_ptr + nsamp for
        codes that are already on the GPU (e.g. PbHandle.output_dev; the contract is under pb_search_run in
        include/pb_hip.h: the producer's stream synchronised, any byte address, valid until this returns).
        Returns dict(snr [ndm][tout] f32, width_log2 [ndm][tout] u8, stats [ndm][2], series?)."""
        if device_ptr is None:
            codes = np.ascontiguousarray(codes, np.uint8).ravel()
            nsamp = codes.size * (8 // nbit) // (self.nchan * self._nif())
            ptr, on_dev = codes.ctypes.data_as(C.c_void_p), 0
        else:
            if nsamp is None:
                raise ValueError("device_ptr needs nsamp")
            nsamp = int(nsamp)
            ptr, on_dev = C.c_void_p(device_ptr), 1
        tout = nsamp - self.max_delay
        if tout < 64:
            raise ValueError("block shorter than the largest dispersion delay (%d samples)" % self.max_delay)
        snr = np.empty((self.ndm, tout), np.float32)
        wid = np.empty((self.ndm, tout), np.uint8)
        stats = np.empty((self.ndm, 2), np.float32)
        series = np.empty((self.ndm, tout), np.uint32) if want_series else None
        t = C.c_int()
        rc = self._L.pb_search_run(self._s, ptr, on_dev, nsamp, nbit,
                                   snr.ctypes.data_as(C.POINTER(C.c_float)), wid.ctypes.data_as(C.POINTER(C.c_uint8)),
                                   series.ctypes.data_as(C.POINTER(C.c_uint32)) if want_series else None,
                                   stats.ctypes.data_as(C.POINTER(C.c_float)), C.byref(t))
        self._check(rc, "pb_search_run")
        self._nsamp = nsamp
        self._tout = tout
        return dict(snr=snr, width_log2=wid, stats=stats, series=series, tout=tout)


def overlap(c, o, delta_dm=0.1, delta_w=3):
    """The reference coincidencer's test for "the same event" between two candidates, src/candidate.py:49-65:
    DMs within delta_dm (fractional, relative to the other's DM), widths (i1 - i0) within a factor delta_w, and the
    sample ranges [i0, i1) overlapping.  c, o: dicts with dm, i0, i1.  delta_w None: no width test."""
    if o["dm"] == 0 or abs(c["dm"] / o["dm"] - 1) > delta_dm:
        if not (o["dm"] == 0 and c["dm"] == 0):
            return False
    if delta_w is not None:
        w1, w2 = float(c["i1"] - c["i0"]), float(o["i1"] - o["i0"])
        if min(w1, w2) <= 0 or max(w1, w2) / min(w1, w2) > delta_w:
            return False
    if c["i0"] < o["i0"]:
        return o["i0"] < c["i1"]
    return c["i0"] < o["i1"]


def group_points(idm, it, sn, w, dms, tsamp, dm_tol=0.1, delta_w=None, sample0=0):
    """Above-threshold (DM index, sample, S/N, boxcar width) points of ONE beam's search -> candidates: strongest
    first, a candidate absorbs every point that overlaps it in time and lies within dm_tol (fractional) of its DM.
    This clustering is this framework's own (heimdall's, which the reference runs at this place, is third-party and
    absent: unpinned).  It uses the time and DM tests of the reference's cross-beam coincidencer (src/candidate.py:
    53-54, 64-66) but by default NOT its width-ratio test (:57-63, delta_w = 3): the points of one series are boxcar
    trials of the same samples, a pulse shows up at every width from 1 to 64, and splitting them by width would
    report one pulse several times.  delta_w (e.g. 3) applies that test as well, for like-for-like experiments.
    Ties in S/N are broken by (DM index, sample, width): the GPU appends points in arrival order, which differs from run
    to run, and the grouping depends on the order.  Returns dicts with heimdall's nine columns."""
    idm, it, w = np.asarray(idm, np.int64), np.asarray(it, np.int64), np.asarray(w, np.int64)
    sn = np.asarray(sn)
    if idm.size == 0:
        return []
    order = np.lexsort((w, it, idm, -sn.astype(np.float64)))
    idm, it, sn, w = idm[order], it[order], sn[order], w[order]
    pdm = np.asarray(dms)[idm]
    taken = np.zeros(idm.size, bool)
    cands = []
    for k in range(idm.size):
        if taken[k]:
            continue
        i0, i1, dm = it[k], it[k] + w[k], pdm[k]
        near = (~taken) & (it < i1) & (it + w > i0) & (np.abs(pdm - dm) <= dm_tol * max(dm, 1.0) + 1e-9)
        if delta_w is not None:
            near &= (np.maximum(w, w[k]) <= delta_w * np.minimum(w, w[k]))
        taken |= near
        cands.append(dict(snr=float(sn[k]), peak_idx=int(sample0 + it[k]), peak_time=float((sample0 + it[k]) * tsamp),
                          tfilt=int(np.log2(w[k])), dmi=int(idm[k]), dm=float(dm), ngiant=int(near.sum()),
                          i0=int(sample0 + it[near].min()), i1=int(sample0 + (it[near] + w[near]).max())))
    return cands


def find_candidates(snr, width_log2, dms, tsamp, threshold=6.0, dm_tol=0.1, sample0=0, delta_w=None):
    """group_points on full S/N planes (Searcher.run): every (DM, sample) at or above the threshold"""
    idm, it = np.nonzero(snr >= threshold)
    return group_points(idm, it, snr[idm, it], 1 << width_log2[idm, it].astype(np.int64), dms, tsamp, dm_tol, delta_w, sample0)


def candidates_from_peaks(pk, dms, tsamp, dm_tol=0.1, sample0=0, delta_w=None):
    """group_points on a peak list (Searcher.peaks) instead of full S/N planes"""
    return group_points(pk["dmi"], pk["t"], pk["snr"], 1 << pk["width_log2"].astype(np.int64), dms, tsamp, dm_tol, delta_w, sample0)


def candidates_from_giants(res, dms, tsamp, sample0=0):
    """Searcher.giants' clusters as candidates: the dicts of group_points (ngiant = the cluster's giants) plus npoints,
    strongest first, ties broken by (DM index, peak).  The clustering is the device's (include/pb_hip.h,
    pb_search_set_giants), connected components of linked giants: exact and independent of any arrival order."""
    if len(res["snr"]) == 0:
        return []
    sn = np.asarray(res["snr"], np.float32)
    order = np.lexsort((res["peak"], res["dmi"], -sn.astype(np.float64)))
    dms = np.asarray(dms)
    return [dict(snr=float(sn[k]), peak_idx=int(sample0 + res["peak"][k]), peak_time=float((sample0 + res["peak"][k]) * tsamp),
                 tfilt=int(res["tfilt"][k]), dmi=int(res["dmi"][k]), dm=float(dms[res["dmi"][k]]),
                 ngiant=int(res["members"][k]), i0=int(sample0 + res["i0"][k]), i1=int(sample0 + res["i1"][k]),
                 npoints=int(res["npoints"][k])) for k in order]


def subband_list(nsb):
    """the default band list of the sub-band search (include/pb_hip.h, pb_search_set_subbands, rule 2): runs (first, count)
    of the nsb base sub-bands, staggered dyadic, widest first -- for c = nsb/2, nsb/4, .. 1 the bands (k max(c/2, 1), c),
    k = 0, 1, .. while they fit: 2, 7, 18, 41 bands for nsb 2, 4, 8, 16"""
    if nsb not in (2, 4, 8, 16):
        raise ValueError("subband_list: nsb must be 2, 4, 8 or 16")
    out, c = [], nsb // 2
    while c >= 1:
        step = max(c // 2, 1)
        out += [(k * step, c) for k in range((nsb - c) // step + 1)]
        c //= 2
    return out


def candidates_from_subbands(res, dms, tsamp, bands, nsb, fch1, foff, nchan, sample0=0):
    """Searcher.subbands' points as candidates: one group_points call over all of them, whatever their band; each dict also
    gets band = (first, count) and snr_full of the point at the candidate's (dmi, peak) -- there is one point per cell --
    and f_lo, f_hi in MHz, the outer edges of the band's channels [first nchan/nsb, (first + count) nchan/nsb)."""
    cands = group_points(res["dmi"], res["t"], res["snr"], 1 << np.asarray(res["width_log2"], np.int64), dms, tsamp, sample0=sample0)
    at = {(int(d), int(t)): i for i, (d, t) in enumerate(zip(res["dmi"], res["t"]))}
    per = nchan // nsb
    for c in cands:
        i = at[(c["dmi"], c["peak_idx"] - sample0)]
        first, count = bands[int(res["band"][i])]
        edges = [fch1 + (first * per - 0.5) * foff, fch1 + ((first + count) * per - 0.5) * foff]
        c.update(band=(int(first), int(count)), f_lo=float(min(edges)), f_hi=float(max(edges)), snr_full=float(res["snr_full"][i]))
    return cands


def gulp_cuts(since, nsamp, gulp):
    """Where a piece of nsamp samples is cut when `since` samples (0 <= since < gulp) have accumulated since the last
    fire and a fire is due every `gulp` new samples: a list of (first sample of the part within the piece, its length,
    whether a fire follows it).  Every part is non-empty, the parts tile the piece in order, a fire follows exactly the
    parts that complete a gulp -- so a piece that ends where a gulp ends has its fire and no empty part after it, and an
    empty piece gives []."""
    since, nsamp, gulp = int(since), int(nsamp), int(gulp)
    if gulp < 1 or not 0 <= since < gulp or nsamp < 0:
        raise ValueError("gulp_cuts: gulp >= 1, 0 <= since < gulp, nsamp >= 0")
    out, off = [], 0
    while off < nsamp:
        k = min(gulp - since, nsamp - off)
        since += k
        out.append((off, k, since == gulp))
        off += k
        if since == gulp:
            since = 0
    return out


class GulpSearch(object):
    """The search over a stream of filterbank samples in gulps, as heimdall runs it (-nsamps_gulp 30720,
    scripts/start_heimdall_single_antenna:21): every gulp is searched together with the last
    max_delay + widest_boxcar - 1 samples of the stream before it, and of a gulp's output samples only those for
    which EVERY boxcar width fits inside the gulp are emitted (k_boxcar stops at the end of the block: the last
    widest - 1 samples have only been tried with the narrow widths); the rest are produced by the next gulp.  So
    each output sample is produced exactly once, with all widths, and neither a pulse whose sweep straddles a gulp
    boundary nor a wide one that starts just before it is lost.  push() returns the candidates of the samples that
    became complete; finish() those of the stream's last widest - 1 samples (narrow widths only: there is no more
    data); sample indices count from the start of the stream.  With RFI cleaning on (Searcher.set_rfi) every block is
    cleaned with its own statistics, as heimdall cleans per gulp: the carried-over tail is cleaned again inside the
    next block.  With the channel stage on (Searcher.set_rfi_chan) every block also gets its own channel mask, and
    chan_log holds (first sample, Searcher.rfi_chan_info()) of each block that the latest push() / feed() / finish() searched.
    cutouts=dict(thresh=..., max_per_gulp=...) (the searcher's set_cutouts() must be on): of each push()'s or
    finish()'s candidates those at or above thresh, strongest first, at most max_per_gulp (and at most the searcher's
    max_cands), get a "cutout" entry -- dict(ft, ft_hits, dt, dt_hits, dm_rows, sub_freqs, tscr) of Searcher.cutouts
    with tscr = max(1, width / 2) -- cut from the block that is still on the device.  Nothing else changes.
    refine=dict(thresh=..., max_per_gulp=...) (the searcher's set_refine() must be on): the same selection gets a
    "refined" entry -- Searcher.refine's dict for the candidate, with `peak` counted from the start of the stream like
    peak_idx (None where Searcher.refine gives None) -- in the same push() / finish().  Printed and sent lines stay as
    they are.
    giants=dict(sep_time=..., sep_dm=..., sep_filter=..., max_giants=...) (any subset; {} for the defaults): the
    candidates come from the device's giants and clusters (Searcher.set_giants / giants, candidates_from_giants) instead
    of the point list and group_points; the point list is not pulled at all.  A gulp with more than max_giants giants
    yields no candidates and one log line.  A run of hot samples cut by the end of a gulp's complete samples is two
    giants, one in each gulp's call.
    gulp=N: the stream arrives through feed() in pieces of any length, 8, 4 or 2 bits, host or device memory, and is
    gathered on the device (Searcher.set_gulp / push): every N new samples the accumulated block is searched as push()
    searches a block of N new samples, and its last max_delay + widest - 1 raw samples are handed on without leaving the
    device.  feed(p1) .. feed(pk) + finish() return, in order, the candidates of push(b1) .. push(bm) + finish() over
    the same stream cut into blocks of N, the remainder last (tests/test_gpu_search_stream.py).  feed_plane() takes a
    piece as an fp32 plane instead, quantised to 8 bits on the device (Searcher.push_plane), and may alternate with
    feed().  gulp=None (default): push() only.
    pol=dict(thresh=..., max_per_gulp=...) (the searcher's set_pol() must be on; push() only, not with gulp=N): the blocks
    are [nsamp][4 nchan] (AA, BB, CR, CI rows per sample) and the same selection gets a "pol" entry -- the candidate's slice
    of Searcher.pol for the request (dmi, peak in block coordinates, min(2^tfilt, 64)): on, non, off, noff, F, kbest, summary,
    rms, freqs; with cutouts also on the strongest of them, as many as the cutouts' max_cands, also carry pft, pft_hits and
    tscr of Searcher.pol_cutouts.  feed() and feed_plane() raise.
    subbands=dict(thresh=..., send=False) (the searcher's set_subbands() must be on; not with pol=): every search is followed
    by the sub-band search of the same block (Searcher.subbands, candidates_from_subbands) and push(), feed() and finish()
    return the full-band candidates as before, followed by the sub-band candidates -- the ones that carry `band` -- of the
    same samples.  Cutouts, refinement and the coincidencer see the full-band candidates only; with send=True the sub-band
    candidates go to the coincidencer as well, as ordinary lines.  A gulp whose points exceed the searcher's max_points
    yields no sub-band candidates and one log line."""

    def __init__(self, searcher, threshold=6.0, nbit=8, coincidencer=None, utc_start="1970-01-01-00:00:00", beam=1,
                 cutouts=None, refine=None, giants=None, gulp=None, pol=None, subbands=None):
        self.s, self.threshold, self.nbit = searcher, threshold, nbit
        self.sub = None
        if subbands is not None:
            if searcher._sub is None:
                raise ValueError("GulpSearch(subbands=...): call the searcher's set_subbands() first")
            if pol is not None:
                raise ValueError("GulpSearch(subbands=...): not together with pol=")
            self.sub = (float(subbands.get("thresh", threshold)), bool(subbands.get("send", False)))
        self.chan_log = []               # (first sample, rfi_chan_info()) per block that the latest call searched (channel stage on)
        self.pending_sub = None          # sub-band points of the latest gulp's last `ov` output samples (for finish())
        self.pol = None
        if pol is not None:
            if searcher._pol is None:
                raise ValueError("GulpSearch(pol=...): call the searcher's set_pol() first")
            if gulp is not None:
                raise ValueError("GulpSearch(pol=...): four-product blocks are not streamed (gulp=N)")
            self.pol = (float(pol.get("thresh", threshold)), min(int(pol.get("max_per_gulp", 32)), searcher._pol[3]))
        self.nif = searcher._nif()
        self.gulp = None
        if gulp is not None:
            if int(gulp) < 1:
                raise ValueError("GulpSearch(gulp=...): at least one sample")
            self.gulp = int(gulp)
            self.since = 0               # samples fed since the last fire
            self.early = None            # finish()'s candidates where the latest fire had to make them (_fire)
        self.gi = giants is not None
        if self.gi:
            searcher.set_giants(**giants)
        self.ref = None
        if refine is not None:
            if searcher._ref is None:
                raise ValueError("GulpSearch(refine=...): call the searcher's set_refine() first")
            self.ref = (float(refine.get("thresh", threshold)), min(int(refine.get("max_per_gulp", 32)), searcher._ref[3]))
        self.cut = None
        if cutouts is not None:
            if searcher._cut is None:
                raise ValueError("GulpSearch(cutouts=...): call the searcher's set_cutouts() first")
            self.cut = (float(cutouts.get("thresh", threshold)), min(int(cutouts.get("max_per_gulp", 32)), searcher._cut[3]))
        self.last_first = 0              # stream index of the first sample of the latest push()'s / finish()'s batch
        self.tail = np.zeros((0, self.nif * searcher.nchan), np.uint8)
        self.done = 0                    # output samples produced so far = stream index of the next block's first output
        self.ov = (1 << (searcher.nbox - 1)) - 1        # widest boxcar - 1
        self.pending = None              # peaks of the latest gulp's last `ov` output samples (for finish())
        self.coincidencer, self.utc_start, self.beam = coincidencer, utc_start, beam
        if self.gulp is not None:
            searcher.set_gulp(min(searcher.max_delay + self.ov, searcher.max_samples))
            self.fill = 0

    def _send(self, cands, first, nsamps):
        if self.coincidencer:
            cmod = importlib.import_module(_pkg + ".candidates")
            host, port = cmod.parse_coincidencer(self.coincidencer)
            cmod.send_candidates(host, port, self.utc_start, self.beam, cands, first_sample=first, nsamps=nsamps)

    def _cutouts(self, cands, sample0):
        """attach cutouts to the strongest candidates (group_points returns them strongest first, ties broken);
        sample0: stream index of the current block's first output sample"""
        if self.cut is None:
            return
        thresh, most = self.cut
        sel = [c for c in cands if c["snr"] >= thresh][:most]
        if not sel:
            return
        tscr = [max(1, (1 << c["tfilt"]) // 2) for c in sel]
        r = self.s.cutouts([c["dmi"] for c in sel], [c["peak_idx"] - sample0 for c in sel], tscr)
        for i, c in enumerate(sel):
            c["cutout"] = dict(ft=r["ft"][i], ft_hits=r["ft_hits"][i], dt=r["dt"][i], dt_hits=r["dt_hits"][i],
                               dm_rows=r["dm_rows"][i], sub_freqs=r["sub_freqs"], tscr=tscr[i])

    def _refine(self, cands, sample0):
        """attach the refinement to the strongest candidates; sample0 as in _cutouts"""
        if self.ref is None:
            return
        thresh, most = self.ref
        sel = [c for c in cands if c["snr"] >= thresh][:most]
        if not sel:
            return
        r = self.s.refine([c["dmi"] for c in sel], [c["peak_idx"] - sample0 for c in sel], [c["tfilt"] for c in sel])
        for c, e in zip(sel, r):
            c["refined"] = None if e is None else dict(e, peak=e["peak"] + sample0)

    def _pol(self, cands, sample0):
        """attach the polarisation products to the strongest candidates; sample0 as in _cutouts"""
        if self.pol is None:
            return
        thresh, most = self.pol
        sel = [c for c in cands if c["snr"] >= thresh][:most]
        if not sel:
            return
        dmi, tpk = [c["dmi"] for c in sel], [c["peak_idx"] - sample0 for c in sel]
        r = self.s.pol(dmi, tpk, [min(1 << c["tfilt"], 64) for c in sel])
        for i, c in enumerate(sel):
            c["pol"] = dict({k: r[k][i] for k in POL_KEYS}, rms=r["rms"], freqs=r["freqs"])
        if self.s._cut is not None:
            # the images of as many of them, strongest first, as the cutouts' max_cands allows
            ncut = min(len(sel), self.s._cut[3])
            tscr = [max(1, (1 << c["tfilt"]) // 2) for c in sel[:ncut]]
            pc = self.s.pol_cutouts(dmi[:ncut], tpk[:ncut], tscr)
            for i, c in enumerate(sel[:ncut]):
                c["pol"].update(pft=pc["pft"][i], pft_hits=pc["pft_hits"][i], tscr=tscr[i])

    def _giants(self, t_lo, t_hi, sample0):
        """the candidates of the current block's samples [t_lo, t_hi) from the device's giants"""
        res = self.s.giants(self.threshold, t_lo, t_hi)
        if res["overflow"]:
            import sys
            sys.stderr.write("search: gulp at sample %d given up: %d giants exceed max_giants %d\n"
                             % (sample0 + t_lo, res["ngiants"], self.s._gi[3]))
            return []
        return candidates_from_giants(res, self.s.dms, self.s.tsamp, sample0=sample0)

    def _sub_cands(self, res, sel, sample0):
        """the sub-band candidates of the points `sel` of a subbands() result (None: the gulp was given up)"""
        if res is None:
            return []
        s = self.s
        sub = {k: res[k][sel] for k in ("dmi", "t", "snr", "width_log2", "band", "snr_full")}
        return candidates_from_subbands(sub, s.dms, s.tsamp, s._sub[1], s._sub[0], s.fch1, s.foff, s.nchan, sample0=sample0)

    def _sub_search(self, nout, tout, sample0):
        """the sub-band search of the current block: the candidates of its samples [0, nout); the points of [nout, tout)
        are kept for finish()"""
        res = self.s.subbands(self.sub[0], 0, tout)
        if res["overflow"]:
            import sys
            sys.stderr.write("search: sub-bands of the gulp at sample %d given up: %d points exceed max_points %d\n"
                             % (sample0, res["npoints"], self.s._sub[2]))
            res = None
        self.pending_sub = (res, sample0, nout)
        return self._sub_cands(res, res["t"] < nout, sample0) if res is not None else []

    def _out(self, cands, sub, first, nsamps):
        """send a batch (the sub-band candidates only with send=True) and return it, the sub-band candidates last"""
        self._send(cands + sub if (sub and self.sub[1]) else cands, first, nsamps)
        return cands + sub

    @staticmethod
    def _subset(pk, sel):
        return dict(dmi=pk["dmi"][sel], t=pk["t"][sel], snr=pk["snr"][sel], width_log2=pk["width_log2"][sel])

    def push(self, block):
        """block: uint8 [nsamp][nchan] (8-bit codes) of NEW samples; [nsamp][4 nchan] with the searcher's set_pol() on"""
        if self.nbit != 8:
            raise ValueError("GulpSearch takes unpacked 8-bit samples")
        block = np.asarray(block, np.uint8).reshape(-1, self.nif * self.s.nchan)
        self.chan_log = []
        data = np.concatenate([self.tail, block]) if self.tail.size else block
        if data.shape[0] - self.s.max_delay < 64 + self.ov:
            self.tail = data                          # not enough yet for one output block
            return []
        cands, sub, first, nout = self._search_block(data, data.shape[0])
        keep = min(self.s.max_delay + self.ov, data.shape[0])
        self.tail = data[data.shape[0] - keep:].copy()
        return self._out(cands, sub, first, nout)

    def _search_block(self, data, fill):
        """push()'s work from the search on: the block is `data` (host, [fill][nchan]) or, with data None, the `fill`
        samples accumulated on the device.  Returns (candidates, sub-band candidates, first, nout)."""
        if self.gi:
            # the same entry with a threshold no sample reaches: the block is searched, no point comes back
            pk = self.s.peaks(data, float("inf"), nbit=8, max_out=1) if data is not None else self.s.gulp_peaks(float("inf"), max_out=1)
            nout = pk["tout"] - self.ov
            cands = self._giants(0, nout, self.done)
            self.pending = (nout, self.done, pk["tout"])
        else:
            pk = self.s.peaks(data, self.threshold, nbit=8) if data is not None else self.s.gulp_peaks(self.threshold)
            nout = pk["tout"] - self.ov                   # samples with every width tried
            full = pk["t"] < nout
            cands = candidates_from_peaks(self._subset(pk, full), self.s.dms, self.s.tsamp, sample0=self.done)
            self.pending = (self._subset(pk, ~full), self.done, pk["tout"])
        first = self.last_first = self.done
        if self.s._rfichan is not None:
            self.chan_log.append((first, self.s.rfi_chan_info()))
        self._cutouts(cands, first)
        self._refine(cands, first)
        self._pol(cands, first)
        sub = self._sub_search(nout, pk["tout"], first) if self.sub else []
        self.done += nout
        return cands, sub, first, nout

    def _fire(self):
        """the accumulated block searched as push() searches tail + block, then its tail handed on"""
        self.since = 0
        fill = self.fill
        if fill - self.s.max_delay < 64 + self.ov:
            return []                                 # not enough yet for one output block: nothing is dropped
        cands, sub, first, nout = self._search_block(None, fill)
        # finish() cuts out and refines its candidates from the block of the latest search, which the advance below
        # and the pieces after it overwrite: where either is asked for, they are made now and kept for finish()
        self.early = self._pending_cands() if (self.cut or self.ref) else None
        out = self._out(cands, sub, first, nout)
        self.s.gulp_advance(min(self.s.max_delay + self.ov, fill))
        self.fill = min(self.s.max_delay + self.ov, fill)
        return out

    def feed(self, codes=None, nbit=8, device_ptr=None, nsamp=None):
        """GulpSearch(gulp=N): a piece of the stream, any number of samples of nbit bits in SIGPROC order -- a host uint8
        array (packed as in a file), or device_ptr + nsamp for bytes on the GPU (Searcher.run's contract).  Returns the
        candidates of the gulps that the piece completed (often none)."""
        if self.gulp is None or self.nif != 1:
            raise ValueError("feed() needs GulpSearch(gulp=N), and a searcher without set_pol()")
        nchan = self.s.nchan
        if nbit not in (8, 4, 2) or (nchan * nbit) % 8:
            raise ValueError("feed: nbit 8, 4 or 2, and a time sample must fill whole bytes (nchan x nbit a multiple of 8)")
        rowb = nchan * nbit // 8
        if device_ptr is None:
            codes = np.ascontiguousarray(codes, np.uint8).ravel()
            if nsamp is None:
                nsamp = codes.size // rowb
            if codes.size < nsamp * rowb:
                raise ValueError("codes holds fewer than nsamp samples")
        elif nsamp is None:
            raise ValueError("device_ptr needs nsamp")
        if device_ptr is None:
            return self._feed(nsamp, lambda off, n: self.s.push(codes[off * rowb:(off + n) * rowb], nbit=nbit, nsamp=n))
        return self._feed(nsamp, lambda off, n: self.s.push(nbit=nbit, device_ptr=device_ptr + off * rowb, nsamp=n))

    def feed_plane(self, plane=None, device_ptr=None, nsamp=None, scale=1.0):
        """feed() for a piece of an fp32 plane [nsamp][nchan] (Searcher.push_plane: quantised to 8 bits on the device) --
        a host float32 array, or device_ptr + nsamp.  The same cuts, fires and returns; feed() and feed_plane() may
        alternate on one stream."""
        if self.gulp is None or self.nif != 1:
            raise ValueError("feed_plane() needs GulpSearch(gulp=N), and a searcher without set_pol()")
        nchan = self.s.nchan
        if device_ptr is None:
            plane = np.ascontiguousarray(plane, np.float32).ravel()
            if nsamp is None:
                nsamp = plane.size // nchan
            if plane.size < nsamp * nchan:
                raise ValueError("plane holds fewer than nsamp samples")
            return self._feed(nsamp, lambda off, n: self.s.push_plane(plane[off * nchan:(off + n) * nchan], nsamp=n, scale=scale))
        if nsamp is None:
            raise ValueError("device_ptr needs nsamp")
        return self._feed(nsamp, lambda off, n: self.s.push_plane(device_ptr=device_ptr + 4 * off * nchan, nsamp=n, scale=scale))

    def _feed(self, nsamp, push):
        """a piece of nsamp samples cut where the gulps end: push(first sample, length) appends a part and returns the
        block's new length; a fire follows each part that completes a gulp"""
        out, self.chan_log = [], []
        for off, n, fire in gulp_cuts(self.since, nsamp, self.gulp):
            self.fill = push(off, n)
            self.since += n
            if fire:
                out += self._fire()
        return out

    def finish(self):
        """end of the stream: candidates of the last widest - 1 output samples; with gulp=N first those of the samples
        fed since the last fire (returned together, the partial gulp's first)"""
        return self.flush() + self._finish()

    def flush(self):
        """GulpSearch(gulp=N): search the partial gulp fed since the last fire now (finish() does it first; a caller that
        wants the two batches apart, each with its own last_first, calls flush() and then finish())"""
        self.chan_log = []
        return self._fire() if self.gulp is not None and self.since > 0 else []

    def _pending_cands(self):
        """the candidates of the latest search's last widest - 1 output samples, from the block that is still the
        searcher's current one"""
        pk, sample0, tout = self.pending
        if self.gi:                                # pk: the first sample of the block that push() left out
            cands = self._giants(pk, tout, sample0) if pk < tout else []
        else:
            cands = candidates_from_peaks(pk, self.s.dms, self.s.tsamp, sample0=sample0)
        self._cutouts(cands, sample0)
        self._refine(cands, sample0)
        self._pol(cands, sample0)
        return cands

    def _pending_sub(self):
        """the sub-band candidates of the same samples, from the points that the latest search kept (no device work)"""
        if not self.sub or self.pending_sub is None:
            return []
        res, sample0, nout = self.pending_sub
        self.pending_sub = None
        return self._sub_cands(res, res["t"] >= nout, sample0) if res is not None else []

    def _finish(self):
        if self.pending is None:
            return []
        early = getattr(self, "early", None)
        cands = early if early is not None else self._pending_cands()
        sub = self._pending_sub()
        _, sample0, tout = self.pending
        self.pending = None
        self.last_first = self.done
        first, self.done = self.done, sample0 + tout
        return self._out(cands, sub, first, tout - (first - sample0))


def candidate_line(c):
    """One heimdall-format text line (columns of src/candidate.py:8-18); see candidates.py for the TCP leg."""
    import importlib
    return importlib.import_module((__package__ or "vlite-fast_amd") + ".candidates").candidate_line(c)


def arg_parser(with_file=True):
    """the command line of main(): heimdall's flag names.  with_file=False: the flags that a host which feeds the search
    itself accepts (process_baseband --search) -- the same ones less -f and -stream_chunk."""
    import argparse
    ap = argparse.ArgumentParser(prog="search" if with_file else "--search", prefix_chars="-",
                                 epilog="with -f also: -pol [-pol_thresh S] [-pol_max N] [-rm LO HI] [-rm_step D] [-pol_off L G]: "
                                        "a nifs 4 filterbank (AA, BB, CR, CI); Stokes spectra and RM synthesis of the strongest "
                                        "candidates (pol_parser).  Also: -subbands N [-subband_thresh S] [-subband_send]: search N base "
                                        "sub-bands (2, 4, 8 or 16) and their staggered dyadic runs for band-limited bursts "
                                        "(subband_parser)")
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
    import argparse
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
    import argparse
    ap = argparse.ArgumentParser(prog="search", prefix_chars="-", add_help=False, allow_abbrev=False)
    ap.add_argument("-subbands", type=int, default=0, help="search N base sub-bands (2, 4, 8 or 16) and their staggered dyadic runs for band-limited bursts; 0: off; with -output_dir a .subband file beside each .cand")
    ap.add_argument("-subband_thresh", type=float, default=None, help="with -subbands: lowest sub-band S/N reported (default: -detect_thresh)")
    ap.add_argument("-subband_send", action="store_true", help="with -subbands: send the sub-band candidates to the coincidencer too")
    return ap


def rfichan_parser():
    """the flags of -rfi_chan, parsed apart from arg_parser()'s like -pol's: a command line without them gives the namespace
    it always gave"""
    import argparse
    ap = argparse.ArgumentParser(prog="search", prefix_chars="-", add_help=False, allow_abbrev=False)
    ap.add_argument("-rfi_chan", action="store_true", help="flag the channels that are noisy for a whole gulp and fill them with their mean before the rest of the cleaning; with -output_dir a .chans file beside each .cand")
    ap.add_argument("-rfi_chan_tol", type=float, default=None, help="with -rfi_chan: the outlier threshold in robust sigmas (default 4)")
    ap.add_argument("-rfi_chan_radius", type=int, default=None, help="with -rfi_chan: the largest lag in unzapped channels (default 0: a tenth of them)")
    return ap


def parse_flags(flags):
    """process_baseband's --search "<flags>": the string split as a shell would and parsed by the search's own parser
    (arg_parser(with_file=False) and parse_args' checks); an unknown flag, -f, -stream_chunk or -pol ends in SystemExit; -subbands
    and -rfi_chan and their flags are taken"""
    import shlex
    return parse_args(shlex.split(flags), with_file=False)


def parse_args(argv=None, with_file=True):
    """arg_parser() plus the checks between flags"""
    import sys
    ap = arg_parser(with_file)
    argv = sys.argv[1:] if argv is None else list(argv)
    pa, rest = pol_parser().parse_known_args(argv)
    sa, rest = subband_parser().parse_known_args(rest)
    ca, rest = rfichan_parser().parse_known_args(rest)
    a = ap.parse_args(rest)
    alone = [f for f in ("-pol_thresh", "-pol_max", "-rm", "-rm_step", "-pol_off") if f in argv]
    if alone and not pa.pol:
        ap.error("%s: only with -pol" % ", ".join(alone))
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
    if (ca.rfi_chan_tol is not None or ca.rfi_chan_radius is not None) and not ca.rfi_chan:
        ap.error("-rfi_chan_tol, -rfi_chan_radius: only with -rfi_chan")
    if ca.rfi_chan:
        if ca.rfi_chan_tol is None:
            ca.rfi_chan_tol = 4.0
        if ca.rfi_chan_radius is None:
            ca.rfi_chan_radius = 0
        if not (ca.rfi_chan_tol > 0 and np.isfinite(ca.rfi_chan_tol)) or ca.rfi_chan_radius < 0:
            ap.error("-rfi_chan_tol must be > 0 and finite, -rfi_chan_radius >= 0")
        for k, v in vars(ca).items():               # (only with -rfi_chan: without it the namespace is what it always was)
            setattr(a, k, v)
    if sa.subbands not in (0, 2, 4, 8, 16):
        ap.error("-subbands must be 0, 2, 4, 8 or 16")
    if (sa.subband_thresh is not None or sa.subband_send) and not sa.subbands:
        ap.error("-subband_thresh, -subband_send: only with -subbands")
    if sa.subbands:
        if pa.pol:
            ap.error("-subbands is not combined with -pol")
        if sa.subband_thresh is None:
            sa.subband_thresh = a.detect_thresh
        for k, v in vars(sa).items():               # (only with -subbands: without it the namespace is what it always was)
            setattr(a, k, v)
    if with_file and a.stream_chunk < 0:
        ap.error("-stream_chunk must be >= 0")
    if pa.pol:
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
        for k, v in vars(pa).items():               # (only with -pol: without it the namespace is what it always was)
            setattr(a, k, v)
    return a


def rm_trials(lo, hi, step):
    """how many trial RMs lo, lo + step, .. reach hi (a step that falls 1e-9 of itself short of hi still counts)"""
    return int(np.floor((hi - lo) / step + 1e-9)) + 1


POL_KEYS = ("on", "non", "off", "noff", "F", "kbest", "summary")


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


CUTOUT_KEYS = ("ft", "ft_hits", "dt", "dt_hits", "dm_rows")


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


def refined_line(c):
    """a candidate's line followed by its refined DM, S/N, width (samples) and peak sample (stream index)"""
    r = c["refined"]
    return "%s\t%.6f\t%.4f\t%d\t%d" % (candidate_line(c), r["dm"], r["snr"], r["width"], r["peak"])


def write_refined(path, cands):
    """The refined candidates of one gulp (those that carry a refinement), one refined_line each.  Returns how many were
    written (0: no file)."""
    cc = [c for c in cands if c.get("refined")]
    if cc:
        with open(path, "w") as f:
            f.write("".join(refined_line(c) + "\n" for c in cc))
    return len(cc)


def subband_line(c):
    """a sub-band candidate's line followed by its band (first base sub-band, how many), the band's edges in MHz and the
    full-band S/N at its peak"""
    return "%s\t%d\t%d\t%.4f\t%.4f\t%.4f" % (candidate_line(c), c["band"][0], c["band"][1], c["f_lo"], c["f_hi"], c["snr_full"])


def write_subbands(path, cands):
    """The sub-band candidates of one gulp (those that carry `band`), one subband_line each.  Returns how many were written
    (0: no file)."""
    cc = [c for c in cands if "band" in c]
    if cc:
        with open(path, "w") as f:
            f.write("".join(subband_line(c) + "\n" for c in cc))
    return len(cc)


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
    gi = dict(sep_time=a.cand_sep_time, sep_dm=a.cand_sep_dm, sep_filter=a.cand_sep_filter,
              max_giants=a.max_giants) if a.giants else None
    g = GulpSearch(s, threshold=a.detect_thresh, coincidencer=a.coincidencer, utc_start=utc, beam=a.beam, cutouts=cut,
                   refine=ref, giants=gi, gulp=gulp, pol=pol, subbands=sub)
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
        cands = [c for c in batch if "band" not in c]
        for c in cands:
            print(candidate_line(c))
        for c in batch:
            if "band" in c:
                print(subband_line(c))
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
    -stream_chunk M reads the file in pieces of M samples and feeds them to GulpSearch(gulp=-nsamps_gulp): the same
    lines, gathered on the GPU as a host behind pb_process would gather them; on this path 4- and 2-bit files are
    accepted and fed packed."""
    sig = importlib.import_module(_pkg + ".sigproc")
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
