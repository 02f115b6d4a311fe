"""CPU reference of the imager (include/pb_hip.h: pb_imager_run): a numpy restatement of the
definition, one IEEE binary32 (or, for the phase, binary64) operation per numpy operation, and a binary64 direct
evaluation of the same sums to bound it with.  Also the seeded point-source model that the localisation tests share."""
import numpy as np

NFFT, CHANMIN, NCHANOUT = 12500, 2155, 4096
DELAY, PHASE = 0, 1
F = np.float32
S = [F(float.fromhex(h)) for h in ("0x1.921fb6p+2", "-0x1.4abbbap+5", "0x1.465ec4p+6", "-0x1.2d9b7cp+6")]
C = [F(float.fromhex(h)) for h in ("-0x1.3bd3ccp+4", "0x1.03c1dep+6", "-0x1.55c64ap+6", "0x1.d9f188p+5")]
BINS = (CHANMIN + np.arange(NCHANOUT)).astype(np.float64)


def rotation(r):
    """r float32, |r| <= 0.5 turns -> (cr, sr) ~ (cos 2 pi r, sin 2 pi r): the header's polynomial, line by line"""
    r = np.asarray(r, F)
    q = np.rint(F(4) * r)
    f = r - q * F(0.25)
    f2 = f * f
    sn = (((S[3] * f2 + S[2]) * f2 + S[1]) * f2 + S[0]) * f
    cs = (((C[3] * f2 + C[2]) * f2 + C[1]) * f2 + C[0]) * f2 + F(1)
    k = q.astype(np.int32) & 3
    odd = (k & 1) == 1
    a = np.where(odd, sn, cs)
    b = np.where(odd, cs, sn)
    return np.where((k == 1) | (k == 2), -a, a), np.where(k >= 2, -b, b)


def phase(dd, dpsi=None):
    """dd, dpsi float64 [npix][nbl] -> r float32 [npix][nbl][4096]"""
    dd = np.asarray(dd, np.float64)
    psi = np.zeros_like(dd) if dpsi is None else np.asarray(dpsi, np.float64)
    t = psi[..., None] + BINS * (dd / 12500.0)[..., None]
    return (t - np.rint(t)).astype(F)


def image(u, dd, dpsi=None, mode=DELAY, block=64):
    """u complex64 [nbl][2][4096]; dd, dpsi float64 [npix][nbl] -> (image float32 [npix], per_bl complex64
    [npix][nbl][2]), both bit for bit what the library returns"""
    u = np.asarray(u, np.complex64)
    dd = np.asarray(dd, np.float64)
    npix, nbl = dd.shape
    assert u.shape == (nbl, 2, NCHANOUT)
    ur = np.ascontiguousarray(u.real, F)[None]            # [1][nbl][2][4096]
    ui = np.ascontiguousarray(u.imag, F)[None]
    per_bl = np.zeros((npix, nbl, 2), np.complex64)
    for p0 in range(0, npix, block):
        sl = slice(p0, min(npix, p0 + block))
        cr, sr = rotation(phase(dd[sl], None if dpsi is None else np.asarray(dpsi)[sl]))
        cr, sr = cr[:, :, None, :], sr[:, :, None, :]
        zr = ur * cr + ui * sr                             # [n][nbl][2][4096]
        zi = ui * cr - ur * sr
        out = []
        for z in (zr, zi):
            z = z.reshape(z.shape[:3] + (64, 64))          # [step][lane]
            P = np.zeros(z.shape[:3] + (64,), F)
            for step in range(64):
                P = P + z[..., step, :]
            o = 32
            while o >= 1:                                    # P[l] = P[l] + P[l + o]; lanes past the wave add their own
                P = np.concatenate([P[..., :64 - o] + P[..., o:], P[..., 64 - o:] + P[..., 64 - o:]], axis=-1)
                o >>= 1
            out.append(P[..., 0])
        per_bl[sl].real, per_bl[sl].imag = out
    return combine(per_bl, mode), per_bl


def combine(per_bl, mode):
    """per_bl complex64 [npix][nbl][2] -> image float32 [npix]: b ascending, slot 0 then 1"""
    img = np.zeros(per_bl.shape[0], F)
    for b in range(per_bl.shape[1]):
        for s in range(2):
            zr, zi = per_bl[:, b, s].real, per_bl[:, b, s].imag
            img = img + (np.sqrt(zr * zr + zi * zi) if mode == DELAY else zr)
    return img


def image64(u, dd, dpsi=None, mode=DELAY):
    """the same sums evaluated directly in binary64: (image [npix], per_bl complex128 [npix][nbl][2])"""
    u = np.asarray(u, np.complex128)
    dd = np.asarray(dd, np.float64)
    psi = np.zeros_like(dd) if dpsi is None else np.asarray(dpsi, np.float64)
    npix, nbl = dd.shape
    per_bl = np.zeros((npix, nbl, 2), np.complex128)
    for p in range(npix):
        t = psi[p][:, None] + BINS * (dd[p] / 12500.0)[:, None]
        rot = np.exp(-2j * np.pi * (t - np.rint(t)))
        per_bl[p] = (u * rot[:, None, :]).sum(axis=-1)
    img = (np.abs(per_bl) if mode == DELAY else per_bl.real).sum(axis=(1, 2))
    return img, per_bl


def error_bound(u, nbl_in_sum):
    """B of DESIGN.md section 11 for one image value: 2^-24 (120 + 2 nbl) sum |u| over what enters the value; with
    nbl_in_sum = 0 the bound of one z (u: that baseline's and slot's 4096 values)"""
    return 2.0 ** -24 * (120 + 2 * nbl_in_sum) * np.abs(np.asarray(u, np.complex128)).sum()


# ---- the point source that the CPU and the GPU tests image ----

def point_source(seed=11, nant=8, n=21, half_width_arcmin=30.0, pixel=(13, 6), extent_m=10e3):
    """nant antennas drawn from `seed` within extent_m of the VLA centre, a gnomonic n x n grid around a fixed position,
    and the noiseless visibilities of a source at grid pixel `pixel`: u = exp(+2 pi i k dd_true / 12500) on both slots.
    -> dict(xyz, unix, ra0, dec0, grid (ra, dec [n*n]), ipix, d_ant [n*n][nant], bls, dd [n*n][nbl], u)"""
    import importlib
    loc = importlib.import_module("vlite-fast_amd.localise")
    rng = np.random.default_rng(seed)
    centre = np.array([-1601185.4, -5041977.5, 3554875.9])
    xyz = centre + rng.uniform(-extent_m / 2, extent_m / 2, (nant, 3))
    unix, ra0, dec0 = 1700000000.0, np.radians(83.6), np.radians(22.0)
    ra, dec = loc.sky_grid(ra0, dec0, half_width_arcmin, n)
    d_ant = np.stack([loc.antenna_delays(xyz, loc.source_vector(a, d, unix)) for a, d in zip(ra, dec)])
    bls = [(i, j) for i in range(nant) for j in range(i + 1, nant)]
    dd = loc.antenna_to_baseline(d_ant, bls)
    ipix = pixel[0] * n + pixel[1]
    u = np.exp(2j * np.pi * BINS * (dd[ipix] / 12500.0)[:, None])
    u = np.repeat(u[:, None, :], 2, axis=1).astype(np.complex64)
    return dict(xyz=xyz, unix=unix, ra0=ra0, dec0=dec0, grid=(ra, dec), ipix=ipix, d_ant=d_ant, bls=bls, dd=dd, u=u, n=n)


class RefImager(object):
    """libpb.PbImager's interface on the CPU: the binary32 restatement (exact=True) or the binary64 model"""

    def __init__(self, nbl, exact=True):
        self.nbl, self.exact, self.u = nbl, exact, None

    def set_vis(self, u):
        self.u = np.asarray(u, np.complex64)

    def run(self, dd, dpsi=None, mode="delay", per_baseline=False):
        m = PHASE if mode == "phase" else DELAY
        img, per_bl = (image if self.exact else image64)(self.u, dd, dpsi, m)
        return (img, per_bl) if per_baseline else img


def delayed_gate(seed=5, nrows=8, delays=(0, 58, 131)):
    """the binary64 model of the delay tests: correlate_ref.delayed_antennas through numpy.fft.rfft rows, bins
    2155..6250, every antenna pair and pol product added over the rows.
    -> (gate_vis complex128 [1][nbl][4][4096], gate_rows_used int [1][nbl][4096]) in the correlator's baseline order"""
    import correlate_ref as CO
    v = CO.delayed_antennas(seed, nrows * NFFT, delays).astype(np.float64) - 128.0
    X = np.fft.rfft(v.reshape(len(delays), 2, nrows, NFFT), axis=-1)[..., CHANMIN:CHANMIN + NCHANOUT]
    bls = CO.baselines(len(delays))
    vis = np.zeros((1, len(bls), 4, NCHANOUT), np.complex128)
    for b, (i, j) in enumerate(bls):
        for p in range(2):
            for q in range(2):
                vis[0, b, 2 * p + q] = (X[i, p] * np.conj(X[j, q])).sum(axis=0)
    return vis, np.full((1, len(bls), NCHANOUT), nrows, np.int64)
