"""CPU reference of the taps = 4 streaming chain (the 4-tap Hamming WOLA window, k_channelize_pfb.hip's header comment,
DESIGN.md section 4.3b) for every RFI mode, one or two output pols, 8 / 4 / 2 bits, restarts and the injected pulse.

The oracle's exported kernels do everything the reference's GPU path has (convertarray, kurtosis, compute_dagostino,
orc_rfft, orc_inject_frb, detect_and_normalize2 / 3, pscrunch(_weights), tscrunch(_weights), sel_and_dig), called in
orc_segment's order (oracle/pb_oracle.c); the parts the reference has no kernel for are restated here in numpy, one
IEEE binary32 operation per numpy operation:

* the FIR: products, then left-to-right adds, over the rows g-3 .. g; rows before the stream (or before a restart)
  are zeros;
* excision: the flagged 500-sample blocks of every contributing row are zeroed before the window;
* the row weight: the unflagged share of the window's energy, float sums in tap-then-block order; an absent row counts
  as flagged, a window without any flag gets exactly 1.

tests/test_pfb_ref_cpu.py holds this module to the two composers of tests/test_gpu_pfb.py (which the kernels are pinned
to at their shapes) and to float64 restatements of the spectra and of the weights."""
import ctypes as C
import types

import numpy as np

NFFT, NCHAN, NBLK, NKURTO = 12500, 6251, 25, 500
F = np.float32
SCALE = F((12500.0 / 128000000 * 8) / 1.0)          # bp_scale of orc_segment
FRB_AMP = F(1.05)


def taps32(oracle):
    """float32 FIR taps [4][12500] as pb_create builds them (sequential double sums for the norms)"""
    win = oracle.hamming_sym(4 * NFFT)
    norms = [1. / np.cumsum(win[j * NFFT:(j + 1) * NFFT] ** 2)[-1] for j in range(4)]
    return np.stack([(win[j * NFFT:(j + 1) * NFFT] * norms[0] * (norms[j] if j else 1.0)).astype(F) for j in range(4)])


def tap_energy(t):
    """E[j][b] as pb_create evaluates it (a sequential double sum of t*t over the block, rounded to float) and the
    float sum of all hundred in tap-then-block order"""
    E = np.empty((4, NBLK), F)
    for j in range(4):
        for b in range(NBLK):
            sq = t[j, b * NKURTO:(b + 1) * NKURTO].astype(np.float64) ** 2
            E[j, b] = F(np.cumsum(sq)[-1])
    tot = F(0)
    for v in E.ravel():
        tot = F(tot + v)
    return E, tot


def frb_width(R):
    """frb_width of orc_segment: 2 ms in rows, the macro expanded left to right in double"""
    rate = float(R) * NFFT * 10
    return F(2e-3 * 10 * rate / 10 / NFFT)


def row_start(nseg, R, resets):
    """first row of the (re)started stream that output row g belongs to, for every g"""
    start = np.zeros(nseg * R, np.int64)
    for k in sorted(resets):
        start[k * R:] = k * R
    return start


def fir_spectra(oracle, t, v, start):
    """v: float32 [rows][12500] voltages, start: row_start() -> complex64 [rows][6251]: the fp32 FIR over the rows
    g-3 .. g that are present (>= start[g]), then the oracle's FFT"""
    rows = v.shape[0]
    pad = np.concatenate([np.zeros((3, NFFT), F), v])
    g = np.arange(rows)
    acc = None
    for j in range(4):
        present = (g - 3 + j >= start)[:, None]
        x = np.where(present, pad[j:j + rows], F(0))
        prod = t[j] * x
        acc = prod if acc is None else (acc + prod).astype(F)
    return oracle.rfft(acc.ravel())


def window_weights(E, tot, flags, start):
    """w[g] of k_pfb_weights from the flags [rows][25] of the stream; rows before start[g] count as flagged"""
    rows = flags.shape[0]
    w = np.empty(rows, F)
    gone = np.ones(NBLK, bool)
    for g in range(rows):
        rr = [flags[g - 3 + j] if g - 3 + j >= start[g] else gone for j in range(4)]
        if not np.any(rr):
            w[g] = F(1.0)
            continue
        s = F(0)
        for j in range(4):
            for b in range(NBLK):
                if not rr[j][b]:
                    s = F(s + E[j, b])
        w[g] = F(s / tot)
    return w


def reported_weights(w, npol):
    """what pb_fetch reports: the weights tscrunch_weights sees -- after pscrunch_weights (npol 1, both pols carry
    the same weight) rows below MIN_WEIGHT are 0"""
    if npol == 2:
        return w.copy()
    return np.where(w.astype(np.float64) >= 0.2, w, F(0))


def pfb_chain(oracle, data, R, rfi_mode, npol, nbit, resets=(), frb_delays=None, inject_from=None, keep_spectra=False):
    """data: u8 [nseg_total][2][R*12500], one antenna's whole stream.  resets: segment indices at which the stream
    restarts (reset_history + reset_bandpass before that segment: earlier rows are absent, the bandpass state is
    zero).  frb_delays with inject_from = k: segment s >= k is processed with inject_now = s - k + 1.
    -> namespace: codes_raw, codes_kur (None for the stream the mode does not run), weights (as pb_fetch reports
    them; None in mode 0), w (the weights themselves), flags [rows][25], bp_raw, bp_kur (final state, 2*6251 each);
    with keep_spectra also spec_raw / spec_kur [2 pols][rows][6251]."""
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    pf = lambda a: a.ctypes.data_as(fp)
    data = np.asarray(data)
    nseg = data.shape[0]
    assert data.shape[1:] == (2, R * NFFT) and R % 8 == 0
    assert rfi_mode in (0, 1, 2) and npol in (1, 2) and nbit in (8, 4, 2)
    resets = tuple(int(k) for k in resets)
    assert all(0 < k < nseg for k in resets)
    rows = nseg * R
    t = taps32(oracle)
    start = row_start(nseg, R, resets)
    volts = [oracle.convertarray(np.concatenate([data[s, p] for s in range(nseg)])) for p in range(2)]
    want_raw, want_kur = rfi_mode != 1, rfi_mode != 0

    flags = np.zeros((rows, NBLK), bool)
    w = np.ones(rows, F)
    if rfi_mode:
        kur = np.concatenate([oracle.kurtosis(v)[1] for v in volts])
        dag = oracle.compute_dagostino(kur)                 # both pols carry the larger of their two statistics
        flags = (dag[:rows * NBLK] > 3.0).reshape(rows, NBLK)
        E, tot = tap_energy(t)
        w = window_weights(E, tot, flags, start)

    spec_raw = spec_kur = None
    if want_raw:
        spec_raw = [fir_spectra(oracle, t, volts[p].reshape(rows, NFFT), start) for p in range(2)]
    if want_kur:
        spec_kur = []
        for p in range(2):
            z = volts[p].reshape(rows, NBLK, NKURTO).copy()
            z[flags] = 0.0
            spec_kur.append(fir_spectra(oracle, t, z.reshape(rows, NFFT), start))

    bp_raw = np.zeros(2 * NCHAN, F)
    bp_kur = np.zeros(2 * NCHAN, F)
    codes_raw, codes_kur = [], []
    nave = (2 if npol == 2 else 1) * (R // 8) * NCHAN
    for s in range(nseg):
        if s in resets:
            bp_raw[:] = 0
            bp_kur[:] = 0
        sl = slice(s * R, (s + 1) * R)
        inject_now = 0
        if frb_delays is not None and inject_from is not None and s >= inject_from:
            inject_now = s - inject_from + 1

        def segment_planes(spec):
            fo = np.ascontiguousarray(np.stack([spec[0][sl], spec[1][sl]])).view(F)      # [pol][R][6251] c64
            if inject_now > 0:
                L.orc_inject_frb(pf(fo), pf(frb_delays), (inject_now - 1) * R, C.c_float(frb_width(R)),
                                 C.c_float(FRB_AMP), R)
            return fo

        if want_raw:
            fo = segment_planes(spec_raw)
            L.orc_detect_and_normalize2(pf(fo), pf(bp_raw), C.c_float(SCALE), R)
            if npol == 1:
                L.orc_pscrunch(pf(fo), R * NCHAN)
            ave = np.zeros(nave, F)
            L.orc_tscrunch(pf(fo), pf(ave), ave.size)
            codes_raw.append(oracle.sel_and_dig(ave, R, npol, nbit))
        if want_kur:
            fk = segment_planes(spec_kur)
            kw = np.ascontiguousarray(np.concatenate([w[sl], w[sl]]))
            L.orc_detect_and_normalize3(pf(fk), pf(kw), pf(bp_kur if rfi_mode == 2 else bp_raw), C.c_float(SCALE), R)
            if npol == 1:
                L.orc_pscrunch_weights(pf(fk), pf(kw), R * NCHAN)
            avek = np.zeros(nave, F)
            L.orc_tscrunch_weights(pf(fk), pf(avek), pf(kw), avek.size)
            codes_kur.append(oracle.sel_and_dig(avek, R, npol, nbit))
    r = types.SimpleNamespace(
        codes_raw=np.concatenate(codes_raw) if want_raw else None,
        codes_kur=np.concatenate(codes_kur) if want_kur else None,
        weights=reported_weights(w, npol) if rfi_mode else None,
        w=w, flags=flags, bp_raw=bp_raw, bp_kur=bp_kur)
    if keep_spectra:
        r.spec_raw = np.stack(spec_raw) if want_raw else None
        r.spec_kur = np.stack(spec_kur) if want_kur else None
    return r
