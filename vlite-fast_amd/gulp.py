"""GulpSearch: a Searcher driven over a stream of filterbank samples in gulps, and gulp_cuts, where a piece of the stream is
cut.  search.py is the entry and the public name."""
import sys

import numpy as np

from .candidates import (candidates_from_giants, candidates_from_peaks, candidates_from_periodic, candidates_from_subbands,
                         parse_coincidencer, send_candidates)
from .searcher import CUTOUT_KEYS, POL_KEYS, block_arg


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
    yields no sub-band candidates and one log line.
    periodic=dict(thresh=8.0, max_per_gulp=64, p_range=None) (the searcher's set_periodic() must be on): every search is
    followed by the periodicity search of the same block's series (Searcher.periodic, candidates_from_periodic) and push(),
    feed() and flush() return its candidates -- the ones that carry `period_s` -- after all the others.  They describe the
    whole block, the samples it shares with the block before it included, and never go to the coincidencer, whose wire
    format has no period."""

    def __init__(self, searcher, threshold=6.0, nbit=8, coincidencer=None, utc_start="1970-01-01-00:00:00", beam=1,
                 cutouts=None, refine=None, giants=None, gulp=None, pol=None, subbands=None, periodic=None):
        self.s, self.threshold, self.nbit = searcher, threshold, nbit
        self.per = None
        self.per_cands = []              # the periodicity candidates of the latest search, until _out() hands them on
        if periodic is not None:
            if searcher._per is None:
                raise ValueError("GulpSearch(periodic=...): call the searcher's set_periodic() first")
            self.per = (float(periodic.get("thresh", 8.0)), int(periodic.get("max_per_gulp", 64)), periodic.get("p_range"))
        self.sub = None
        if subbands is not None:
            if searcher._sub is None:
                raise ValueError("GulpSearch(subbands=...): call the searcher's set_subbands() first")
            if pol is not None:
                raise ValueError("GulpSearch(subbands=...): not together with pol=")
            self.sub = (float(subbands.get("thresh", threshold)), bool(subbands.get("send", False)))
        self.chan_log = []               # (first sample, rfi_chan_info()) per block that the latest call searched (channel stage on)
        self.pending_sub = None          # sub-band points of the latest gulp's last `ov` output samples (for finish())
        self.pol = self._selection("pol", pol, searcher._pol)
        if pol is not None and gulp is not None:
            raise ValueError("GulpSearch(pol=...): four-product blocks are not streamed (gulp=N)")
        self.nif = searcher._nif()
        self.gulp = None
        self.early = None                # finish()'s candidates where the latest fire had to make them (_fire)
        if gulp is not None:
            if int(gulp) < 1:
                raise ValueError("GulpSearch(gulp=...): at least one sample")
            self.gulp = int(gulp)
            self.since = 0               # samples fed since the last fire
        self.gi = giants is not None
        if self.gi:
            searcher.set_giants(**giants)
        self.ref = self._selection("refine", refine, searcher._ref)
        self.cut = self._selection("cutouts", cutouts, searcher._cut)
        self.last_first = 0              # stream index of the first sample of the latest push()'s / finish()'s batch
        self.tail = np.zeros((0, self.nif * searcher.nchan), np.uint8)
        self.done = 0                    # output samples produced so far = stream index of the next block's first output
        self.ov = (1 << (searcher.nbox - 1)) - 1        # widest boxcar - 1
        self.pending = None              # peaks of the latest gulp's last `ov` output samples (for finish())
        self.coincidencer, self.utc_start, self.beam = coincidencer, utc_start, beam
        if self.gulp is not None:
            searcher.set_gulp(min(searcher.max_delay + self.ov, searcher.max_samples))
            self.fill = 0

    def _selection(self, name, opts, stage):
        """the constructor's cutouts= / refine= / pol=: None, or (lowest S/N, most per gulp) of the candidates that get the
        entry; `stage` is the searcher's state of the stage that makes it and must be switched on"""
        if opts is None:
            return None
        if stage is None:
            raise ValueError("GulpSearch(%s=...): call the searcher's set_%s() first" % (name, name))
        return float(opts.get("thresh", self.threshold)), min(int(opts.get("max_per_gulp", 32)), stage.max_cands)

    def _send(self, cands, first, nsamps):
        if self.coincidencer:
            host, port = parse_coincidencer(self.coincidencer)
            send_candidates(host, port, self.utc_start, self.beam, cands, first_sample=first, nsamps=nsamps)

    @staticmethod
    def _select(cands, selection, sample0):
        """the candidates a selection (_selection) takes -- those at or above its S/N, strongest first (group_points
        returns them so, ties broken), at most as many as it allows -- with their trial-DM indices and their peaks in
        block coordinates; sample0: stream index of the current block's first output sample"""
        sel = [c for c in cands if c["snr"] >= selection[0]][:selection[1]] if selection else []
        return sel, [c["dmi"] for c in sel], [c["peak_idx"] - sample0 for c in sel]

    def _attach(self, cands, sample0):
        """attach cutouts, the refinement and the polarisation products, each to the strongest candidates of its selection,
        from the block that is still the searcher's current one; sample0 as in _select"""
        sel, dmi, tpk = self._select(cands, self.cut, sample0)
        if sel:
            tscr = [max(1, (1 << c["tfilt"]) // 2) for c in sel]
            r = self.s.cutouts(dmi, tpk, tscr)
            for i, c in enumerate(sel):
                c["cutout"] = dict({k: r[k][i] for k in CUTOUT_KEYS}, sub_freqs=r["sub_freqs"], tscr=tscr[i])
        sel, dmi, tpk = self._select(cands, self.ref, sample0)
        if sel:
            for c, e in zip(sel, self.s.refine(dmi, tpk, [c["tfilt"] for c in sel])):
                c["refined"] = None if e is None else dict(e, peak=e["peak"] + sample0)
        sel, dmi, tpk = self._select(cands, self.pol, sample0)
        if sel:
            r = self.s.pol(dmi, tpk, [min(1 << c["tfilt"], 64) for c in sel])
            for i, c in enumerate(sel):
                c["pol"] = dict({k: r[k][i] for k in POL_KEYS}, rms=r["rms"], freqs=r["freqs"])
            if self.s._cut is not None:
                # the images of as many of them, strongest first, as the cutouts' max_cands allows
                ncut = min(len(sel), self.s._cut.max_cands)
                tscr = [max(1, (1 << c["tfilt"]) // 2) for c in sel[:ncut]]
                pc = self.s.pol_cutouts(dmi[:ncut], tpk[:ncut], tscr)
                for i, c in enumerate(sel[:ncut]):
                    c["pol"].update(pft=pc["pft"][i], pft_hits=pc["pft_hits"][i], tscr=tscr[i])

    @staticmethod
    def _given_up(what, sample, n, things, most):
        sys.stderr.write("search: %s at sample %d given up: %d %s exceed max_%s %d\n" % (what, sample, n, things, things, most))

    def _giants(self, t_lo, t_hi, sample0):
        """the candidates of the current block's samples [t_lo, t_hi) from the device's giants"""
        res = self.s.giants(self.threshold, t_lo, t_hi)
        if res["overflow"]:
            self._given_up("gulp", sample0 + t_lo, res["ngiants"], "giants", self.s._gi.max_giants)
            return []
        return candidates_from_giants(res, self.s.dms, self.s.tsamp, sample0=sample0)

    def _sub_cands(self, res, sel, sample0):
        """the sub-band candidates of the points `sel` of a subbands() result (None: the gulp was given up)"""
        if res is None:
            return []
        s = self.s
        sub = {k: res[k][sel] for k in ("dmi", "t", "snr", "width_log2", "band", "snr_full")}
        return candidates_from_subbands(sub, s.dms, s.tsamp, s._sub.bands, s._sub.nsb, s.fch1, s.foff, s.nchan, sample0=sample0)

    def _sub_search(self, nout, tout, sample0):
        """the sub-band search of the current block: the candidates of its samples [0, nout); the points of [nout, tout)
        are kept for finish()"""
        res = self.s.subbands(self.sub[0], 0, tout)
        if res["overflow"]:
            self._given_up("sub-bands of the gulp", sample0, res["npoints"], "points", self.s._sub.max_points)
            res = None
        self.pending_sub = (res, sample0, nout)
        return self._sub_cands(res, res["t"] < nout, sample0) if res is not None else []

    def _out(self, cands, sub, first, nsamps):
        """send a batch (the sub-band candidates only with send=True, the periodicity candidates never) and return it, the
        sub-band candidates after the full-band ones, the periodicity candidates last"""
        self._send(cands + sub if (sub and self.sub[1]) else cands, first, nsamps)
        per, self.per_cands = self.per_cands, []
        return cands + sub + per

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
        if self.per:
            self.per_cands = candidates_from_periodic(self.s.periodic(), self.s.dms, self.s.tsamp, self.per[0], self.per[1],
                                                      p_range=self.per[2])
        self._attach(cands, first)
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
        _, _, nsamp, codes = block_arg(codes, np.uint8, nchan, nbit, device_ptr, nsamp, "codes")
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
        _, _, nsamp, plane = block_arg(plane, np.float32, nchan, 32, device_ptr, nsamp, "plane")
        if device_ptr is None:
            return self._feed(nsamp, lambda off, n: self.s.push_plane(plane[off * nchan:(off + n) * nchan], nsamp=n, scale=scale))
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
        self._attach(cands, sample0)
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
        cands = self.early if self.early is not None else self._pending_cands()
        sub = self._pending_sub()
        _, sample0, tout = self.pending
        self.pending = None
        self.last_first = self.done
        first, self.done = self.done, sample0 + tout
        return self._out(cands, sub, first, tout - (first - sample0))

