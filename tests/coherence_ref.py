"""CPU reference of coherence output (AA, BB, CR, CI; include/pb_hip.h).

The oracle's exported pieces give the spectra and the row weights (convertarray, kurtosis, compute_dagostino,
apply_kurtosis, orc_rfft, orc_inject_frb); the rest is a numpy float32 restatement of the definition, one IEEE
binary32 operation per numpy operation.  The restated bandpass recurrence is pinned by the AA / BB planes, which must
equal orc_segment's npol = 2 planes (test_gpu_coherence.py)."""
import numpy as np

NFFT, NCHAN, CHANMIN, NCHANOUT, NSCRUNCH = 12500, 6251, 2155, 4096, 8
F = np.float32
SCALE = F(12500 / 128000000 * 8 / 1.0)
OMS = F(F(1) - SCALE)
TSCALE = F(np.sqrt(1. / 8))
SQRT2 = F(1.41421356)


def spectra(O, udat, R, rfi_mode, delays=None, since=None):
    """-> {stream: (X [2 pols][R][4096] complex64, w [2][R] float32)} for the streams rfi_mode runs"""
    import ctypes as C
    t = O.convertarray(np.ascontiguousarray(udat)).ravel()
    out = {}
    w = np.ones((2, R), F)
    tk = t
    if rfi_mode:
        _, kur = O.kurtosis(t)
        dag = O.compute_dagostino(kur, 0)
        tk, norms = O.apply_kurtosis(t, dag)
        w = norms.reshape(2, R)
    for st in ((0,) if rfi_mode == 0 else (1,) if rfi_mode == 1 else (0, 1)):
        X = O.rfft(tk if st else t)               # [2R][6251]
        if delays is not None and since is not None:
            width = F(2e-3 * 10 * (R * NFFT * 10.) / 10 / NFFT)
            O.lib().orc_inject_frb(X.view(F).ctypes.data_as(C.POINTER(C.c_float)), O._f(delays), int(since),
                                   C.c_float(width), C.c_float(1.05), R)
        out[st] = (np.ascontiguousarray(X.reshape(2, R, NCHAN)[:, :, CHANMIN:CHANMIN + NCHANOUT]), w)
    return out


class CohState(object):
    """bandpass per stream, [2 pols][4096], 0 = initialise from the next segment"""

    def __init__(self):
        self.bp = {0: np.zeros((2, NCHANOUT), F), 1: np.zeros((2, NCHANOUT), F)}


def detect(X, w, bp, kur, clip_out=None):
    """One segment of one stream.  X [2][R][4096] complex64, w [2][R]; bp [2][4096] updated in place.
    -> fp32 planes [4][R/8][4096] (AA, BB, CR, CI).  clip_out: a list that receives the segment's [2][R][4096] bool
    array of samples that took the 11x clip (all False on the raw stream)"""
    R = X.shape[1]
    xr, xi = X.real.astype(F), X.imag.astype(F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xx = xr * xr
        yy = xi * xi
        pw = xx + yy                                                   # [2][R][4096]
        if kur:
            wr = w[:, :, None]
            pw = np.where(wr == 0, F(np.inf), pw / np.where(wr == 0, F(1), wr)).astype(F)
        for pol in range(2):
            init = bp[pol] == 0
            if init.any():
                acc = np.zeros(NCHANOUT, F)
                good = 0
                for t in range(R):
                    if kur and w[pol, t] == 0:
                        continue
                    good += 1
                    acc = acc + pw[pol, t]
                if kur and good == 0:
                    acc = np.ones(NCHANOUT, F)
                else:
                    acc = acc / F(R if not kur else good)
                bp[pol] = np.where(init, acc, bp[pol])
        v = np.empty((2, R, NCHANOUT), F)
        un = np.empty((2, R, NCHANOUT), F)
        clip = np.zeros((2, R, NCHANOUT), bool)
        for t in range(R):
            p = pw[:, t]
            c = OMS * bp
            s = SCALE * p
            bpn = s + c
            if kur:
                cl = p > bp * F(11)
                clip[:, t] = cl
                bp[:] = np.where(cl, bp, bpn)
            else:
                bp[:] = bpn
            un[:, t] = bp
            x = p / bp - F(1)
            if kur:
                x = np.where(clip[:, t], F(10), x)
                x = np.where((w[:, t] == 0)[:, None], F(0), x)
            v[:, t] = x
        ax, ay, bx, by = xr[0], xi[0], xr[1], xi[1]
        re = ax * bx + ay * by
        im = ay * bx - ax * by
        if kur:
            n = (un[0] * w[0][:, None]) * (un[1] * w[1][:, None])
        else:
            n = un[0] * un[1]
        d = np.sqrt(n)
        cr = re / d * SQRT2
        ci = im / d * SQRT2
        if kur:
            zero = (w[0] == 0)[:, None] | (w[1] == 0)[:, None] | clip[0] | clip[1]
            cr = np.where(zero, F(0), cr)
            ci = np.where(zero, F(0), ci)
    if clip_out is not None:
        clip_out.append(clip)
    prod = [v[0], v[1], cr, ci]
    nt = R // NSCRUNCH
    out = np.zeros((4, nt, NCHANOUT), F)
    for g in range(nt):
        rows = range(g * 8, g * 8 + 8)
        for k in range(4):
            acc = np.zeros(NCHANOUT, F)
            if not kur:
                for t in rows:
                    acc = acc + prod[k][t]
                acc = acc * TSCALE
            else:
                wt_sum, wt_sumf = 0, F(0)
                for t in rows:
                    if k < 2:
                        wt = w[k, t]
                        if float(wt) < 0.2:
                            continue
                    else:
                        if float(w[0, t]) < 0.2 or float(w[1, t]) < 0.2:
                            continue
                        wt = F(0.5 * float(F(w[0, t] + w[1, t])))
                    wt_sum += 1
                    wt_sumf = F(wt_sumf + wt)
                    acc = wt * prod[k][t] + acc
                if float(F(wt_sumf / F(NSCRUNCH))) >= 0.2:
                    acc = acc / np.sqrt(F(wt_sum))
                else:
                    acc = np.zeros(NCHANOUT, F)
            out[k, g] = acc
    return out


def quantise(O, planes, nbit):
    """[4][R/8][4096] -> the coherence codes [time][4][4096] of one segment (orc_sel_and_dig_*, npol = 4)"""
    nt = planes.shape[1]
    full = np.zeros((4, nt, NCHAN), F)
    full[:, :, CHANMIN:CHANMIN + NCHANOUT] = planes
    full = np.ascontiguousarray(full).ravel()
    nbytes = 4 * nt * NCHANOUT * nbit // 8
    out = np.zeros(nbytes, np.uint8)
    fn = {8: "orc_sel_and_dig_8b", 4: "orc_sel_and_dig_4b", 2: "orc_sel_and_dig_2b"}[nbit]
    getattr(O.lib(), fn)(O._f(full), O._u(out), nbytes, 4, nt)
    return out


class Streams(dict):
    """run's result: {stream: (codes, planes)}; .state is the CohState the run used and left updated"""
    state = None


def run(O, data, R, rfi_mode, nbit, delays=None, inject_now=0, state=None, clip_out=None):
    """data [nseg][2][R*12500] u8 -> {stream: (codes [nseg*trim], planes [nseg][4][R/8][4096])}, a Streams.
    state: the CohState to continue from (default: a fresh one); it is updated in place and returned as the result's
    .state.  clip_out: a dict that receives {stream: [per segment the clip array of detect]}"""
    st = CohState() if state is None else state
    codes = {0: [], 1: []}
    planes = {0: [], 1: []}
    inj = inject_now
    for s in range(data.shape[0]):
        since = (inj - 1) * R if (delays is not None and inj > 0) else None
        for stream, (X, w) in spectra(O, data[s], R, rfi_mode, delays, since).items():
            cl = None if clip_out is None else clip_out.setdefault(stream, [])
            p = detect(X, w, st.bp[stream], kur=stream == 1, clip_out=cl)
            planes[stream].append(p)
            codes[stream].append(quantise(O, p, nbit))
        if inj > 0:
            inj += 1
    out = Streams((k, (np.concatenate(codes[k]), np.stack(planes[k]))) for k in codes if codes[k])
    out.state = st
    return out
