"""Candidates on the host: the search's points, giants and sub-band points grouped into candidates (overlap .. subband_list,
below the TCP leg), the periodicity search's best table grouped by harmonic ratio (periodic_octaves .. candidates_from_periodic), and candidates to the coincidencer: the TCP leg heimdall's `-coincidencer host:port` plays in the reference
(scripts/start_heimdall_single_antenna:21 `-coincidencer vlite-nrl:27555`; server side
/root/reference/src/trigger.py:7-8,37-43,84-123).

Wire format, as that server parses it: one TCP connection per gulp, the client writes text and closes
(the server reads until recv() returns 0, :95-100, then splits on newlines and drops empty lines):
    line 0   "<utc> <x> <y> <beam>"      utc = toks[0] ('%Y-%m-%d-%H:%M:%S', :170), beam = int(toks[3]), 1-based (:119)
    line 1   (one more header line, skipped: candidates start at lines[2], :128)
    line 2.. one candidate per line, the nine columns of src/candidate.py:8-18
             S/N, peak index, peak time, filter index, DM index, DM, members, first sample, last sample
A message of exactly two lines means "no candidates in this gulp" (:111-112).
heimdall itself (third party, absent) defines what x, y and line 1 hold; the coincidencer reads neither,
so they are written as the gulp's first sample and sample count and a column legend.
"""
import socket

import numpy as np

HEIMDALL_PORT = 27555          # src/trigger.py:8


def candidate_line(c):
    """One heimdall-format text line (columns of src/candidate.py:8-18)."""
    return "%.6f\t%d\t%.6f\t%d\t%d\t%.4f\t%d\t%d\t%d" % (c["snr"], c["peak_idx"], c["peak_time"], c["tfilt"],
                                                        c["dmi"], c["dm"], c["ngiant"], c["i0"], c["i1"])


def format_message(utc_start, beam, cands, first_sample=0, nsamps=0):
    """The text of one gulp's message.  utc_start: the observation's UTC_START string (ring header key);
    beam: 1-based beam / antenna number as heimdall's -beam."""
    lines = ["%s %d %d %d" % (utc_start, first_sample, nsamps, beam),
             "# S/N peak_idx peak_time tfilt dmi dm ngiant i0 i1"]
    lines += [candidate_line(c) for c in cands]
    return ("\n".join(lines) + "\n").encode()


def send_candidates(host, port, utc_start, beam, cands, first_sample=0, nsamps=0, timeout=2.0):
    """Connect, write one gulp's message, close (the close is the end-of-message marker).
    Returns the number of bytes sent; raises OSError when the coincidencer is not reachable."""
    msg = format_message(utc_start, beam, cands, first_sample, nsamps)
    with socket.create_connection((host, port), timeout=timeout) as s:
        s.sendall(msg)
        s.shutdown(socket.SHUT_WR)
    return len(msg)


def parse_coincidencer(spec):
    """'host:port' as heimdall's -coincidencer takes it"""
    host, _, port = spec.rpartition(":")
    if not host:
        return spec, HEIMDALL_PORT
    return host, int(port)


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


PERIODIC_BINS = (32, 64, 128)
PERIODIC_K_MAX = 12            # the longest octave of the periodicity search (include/pb_hip.h, pb_search_set_periodic)


def periodic_octaves(p_lo, p_hi, bins, tsamp):
    """the octaves (k_lo, k_hi) whose periods bins 2^k tsamp .. 2 bins 2^k tsamp cover [p_lo, p_hi] seconds as far as the
    search reaches: k_lo = max(0, floor(log2(p_lo / (bins tsamp)))), k_hi = floor(log2(p_hi / (bins tsamp))).  ValueError,
    naming the bound, where p_hi is below the shortest searchable period or p_hi's octave is beyond the longest one."""
    base = bins * tsamp
    if not (p_lo > 0 and p_hi >= p_lo):
        raise ValueError("periodic: need 0 < P_LO <= P_HI")
    if p_hi < base:
        raise ValueError("periodic: P_HI %g s is below the shortest searchable period, %g s (bins x tsamp)" % (p_hi, base))
    k_lo = max(0, int(np.floor(np.log2(p_lo / base))))
    k_hi = int(np.floor(np.log2(p_hi / base)))
    if k_hi > PERIODIC_K_MAX:
        raise ValueError("periodic: P_HI %g s is beyond the longest searchable period, %g s (2 bins x 2^%d tsamp)"
                         % (p_hi, 2 * base * 2 ** PERIODIC_K_MAX, PERIODIC_K_MAX))
    return min(k_lo, k_hi), k_hi


def harmonic_ratio(period, period_c, tol, nmax=8):
    """the ratio (a, b), a and b in 1..nmax in lowest terms, smallest a + b first, with |period b / (period_c a) - 1| <= tol
    -- period is a / b of period_c within tol --, or None"""
    best = None
    for a in range(1, nmax + 1):
        for b in range(1, nmax + 1):
            if np.gcd(a, b) == 1 and abs(period * b / (period_c * a) - 1.0) <= tol and (best is None or a + b < sum(best)):
                best = (a, b)
    return best


def candidates_from_periodic(res, dms, tsamp, thresh, max_cands=64, p_range=None):
    """Searcher.periodic's best table as periodicity candidates.  The entries at or above thresh (with p_range = (lo, hi)
    only those whose period lies in it), strongest first (ties: the smaller DM index, octave, base period); a weaker entry is
    absorbed by a stronger kept candidate c when its period P is a small-integer ratio of c's, at any DM:
    |P b / (P_c a) - 1| <= (w_c + 1) / (m_c p_c) for some a, b in 1..8 -- a period error drifts m times per fold and a pulse
    survives a drift of about its own width.  At most max_cands are kept; what comes after them is dropped.  Each dict:
    snr, period_s, dm, dmi, k, p, i, q, j, m, M, width_s = 2^q 2^k tsamp, phase = j / p, nabsorbed, and nharm = "a/b", the
    ratio (harmonic_ratio) of the strongest absorbed entry's period to the candidate's ("1/1" with none absorbed)."""
    snr = np.asarray(res["snr"], np.float32)
    ok = (snr >= np.float32(thresh)) & (np.asarray(res["i"]) >= 0)
    if p_range is not None:
        with np.errstate(invalid="ignore"):
            ok &= (res["period_s"] >= p_range[0]) & (res["period_s"] <= p_range[1])
    idx = np.argwhere(ok)
    order = np.argsort(-snr[ok].astype(np.float64), kind="stable")      # (argwhere ascends in dmi, octave, base period)
    idx = idx[order]
    per = np.array([res["period_s"][tuple(e)] for e in idx], np.float64)
    live = np.ones(len(idx), bool)
    ab = [(a, b) for a in range(1, 9) for b in range(1, 9)]
    out = []
    for n, e in enumerate(idx):
        if not live[n]:
            continue
        if len(out) >= max_cands:
            break
        d, ki, pi = [int(v) for v in e]
        k, p, q = int(res["octaves"][ki]), int(res["p"][pi]), int(res["q"][d, ki, pi])
        m = int(res["m"][d, ki, pi])
        tol = ((1 << q) + 1.0) / (m * p)
        live[n] = False
        hit = np.zeros(len(idx), bool)
        for a, b in ab:
            hit |= np.abs(per * b / (per[n] * a) - 1.0) <= tol
        hit &= live
        live &= ~hit
        first = np.nonzero(hit)[0]
        ratio = (harmonic_ratio(per[first[0]], per[n], tol) if first.size else None) or (1, 1)
        out.append(dict(snr=float(snr[d, ki, pi]), period_s=float(per[n]), dm=float(dms[d]), dmi=d, k=k, p=p,
                        i=int(res["i"][d, ki, pi]), q=q, j=int(res["j"][d, ki, pi]), m=m, M=int(res["M"][d, ki, pi]),
                        width_s=float((1 << q) * (1 << k) * tsamp), phase=float(res["j"][d, ki, pi]) / p,
                        nabsorbed=int(hit.sum()), nharm="%d/%d" % ratio))
    return out
