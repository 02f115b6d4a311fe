"""NumPy restatement of the giants-and-clusters definition of include/pb_hip.h (pb_search_set_giants), step by step:
giants by splitting each series' hot samples at gaps, clusters by union-find over the linked pairs.  No GPU.  Written
for clarity, not speed: the link test visits all pairs of giants of nearby series."""
import numpy as np

GIANT_FIELDS = ("dmi", "begin", "end", "npts", "peak", "snr", "tfilt")
CAND_FIELDS = ("snr", "peak", "tfilt", "dmi", "members", "npoints", "i0", "i1")


def find_giants(snr, wl, thresh, t_lo, t_hi, sep_time):
    """steps 1-4: dict of arrays, ascending (dmi, begin)"""
    snr = np.asarray(snr, np.float32)
    thresh = np.float32(thresh)
    out = {k: [] for k in GIANT_FIELDS}
    for d in range(snr.shape[0]):
        row = snr[d, t_lo:t_hi]
        with np.errstate(invalid="ignore"):
            hot = np.nonzero(row >= thresh)[0] + t_lo           # a NaN compares false
        if hot.size == 0:
            continue
        cuts = np.nonzero(np.diff(hot) > sep_time)[0] + 1
        for run in np.split(hot, cuts):
            v = snr[d, run]
            peak = int(run[np.nonzero(v == v.max())[0][0]])     # the smallest t among equals (-0 == +0)
            out["dmi"].append(d)
            out["begin"].append(int(run[0]))
            out["end"].append(int(run[-1]) + 1)
            out["npts"].append(int(run.size))
            out["peak"].append(peak)
            out["snr"].append(snr[d, peak])
            out["tfilt"].append(int(wl[d, peak]))
    g = {k: np.asarray(out[k], np.int64) for k in GIANT_FIELDS if k != "snr"}
    g["snr"] = np.asarray(out["snr"], np.float32)
    return g


def linked(g, a, b, sep_time, sep_dm, sep_filter):
    """step 5"""
    return (abs(int(g["dmi"][a]) - int(g["dmi"][b])) <= sep_dm and abs(int(g["tfilt"][a]) - int(g["tfilt"][b])) <= sep_filter
            and g["begin"][a] < g["end"][b] + sep_time and g["begin"][b] < g["end"][a] + sep_time)


def label_giants(g, sep_time, sep_dm, sep_filter):
    """steps 5-6: each giant's label = the smallest index of its connected component"""
    n = g["dmi"].size
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    dmi, tf, b, e = g["dmi"], g["tfilt"], g["begin"], g["end"]
    for a in range(n):
        # all pairs at once for giant a; a itself and its own series drop out of the time test or are harmless
        m = ((np.abs(dmi[:a] - dmi[a]) <= sep_dm) & (np.abs(tf[:a] - tf[a]) <= sep_filter)
             & (b[a] < e[:a] + sep_time) & (b[:a] < e[a] + sep_time))
        for o in np.nonzero(m)[0]:
            ra, ro = find(a), find(int(o))
            if ra != ro:
                parent[max(ra, ro)] = min(ra, ro)
    return np.asarray([find(x) for x in range(n)], np.int64)


def merge(g, label):
    """steps 7-9 (device order): one candidate per cluster, in label order"""
    out = {k: [] for k in CAND_FIELDS}
    for lab in np.unique(label):
        mem = np.nonzero(label == lab)[0]
        v = g["snr"][mem]
        w = int(mem[np.nonzero(v == v.max())[0][0]])            # ties: the smallest giant index
        out["snr"].append(g["snr"][w])
        out["peak"].append(int(g["peak"][w]))
        out["tfilt"].append(int(g["tfilt"][w]))
        out["dmi"].append(int(g["dmi"][w]))
        out["members"].append(int(mem.size))
        out["npoints"].append(int(g["npts"][mem].sum()))
        out["i0"].append(int(g["begin"][mem].min()))
        out["i1"].append(int(g["end"][mem].max()))
    c = {k: np.asarray(out[k], np.int64) for k in CAND_FIELDS if k != "snr"}
    c["snr"] = np.asarray(out["snr"], np.float32)
    return c


def giants_ref(snr, wl, thresh, t_lo=0, t_hi=None, sep_time=3, sep_dm=200, sep_filter=3, max_giants=1 << 18):
    """The whole definition: dict(giants, label, cands, ngiants, overflow).  After an overflow (step 10) ngiants is
    exact and there are no giants, labels or candidates."""
    snr = np.asarray(snr, np.float32)
    wl = np.asarray(wl, np.uint8)
    t_hi = snr.shape[1] if t_hi is None else t_hi
    assert 0 <= t_lo < t_hi <= snr.shape[1] and 1 <= sep_time <= 64 and sep_dm >= 0 and sep_filter >= 0
    g = find_giants(snr, wl, thresh, t_lo, t_hi, sep_time)
    n = int(g["dmi"].size)
    if n > max_giants:
        g = find_giants(snr[:0], wl[:0], thresh, t_lo, t_hi, sep_time)
        return dict(giants=g, label=np.zeros(0, np.int64), cands=merge(g, np.zeros(0, np.int64)), ngiants=n, overflow=True)
    label = label_giants(g, sep_time, sep_dm, sep_filter)
    return dict(giants=g, label=label, cands=merge(g, label), ngiants=n, overflow=False)


def sort_strongest_first(c):
    """step 9, the host's order: strongest first, ties by (dmi, peak)"""
    order = np.lexsort((c["peak"], c["dmi"], -c["snr"].astype(np.float64)))
    return {k: v[order] for k, v in c.items()}
