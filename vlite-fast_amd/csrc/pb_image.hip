// The imager (include/pb_hip.h: pb_imager*): a caller's weighted visibilities u[b][s][c] rotated by each pixel's delay
// slope, added over the 4096 channels per baseline and product slot, and the baselines combined into an image value.
// Every rotation phase differs per (pixel, baseline, channel), so this is vector arithmetic, not a GEMM.
//
// k_image_z: one 64-lane workgroup = one baseline and a tile of IMG_PX pixels.  A lane owns the channels l, l + 64, ..
//   of the definition; per step it loads its two u values (one 8-byte load per product slot, coalesced over the lanes)
//   ONCE and rotates them for every pixel of the tile, whose 4 IMG_PX partial sums stay in registers.  The delay and
//   phase of a (pixel, baseline) are the same in every lane.  Double arithmetic only for the phase (a convert, a
//   multiply, an add, a round, a subtract, a convert back); the rotation is the header's binary32 polynomial.  After the
//   64 steps the __shfl_down tree of the definition, and lane 0 stores z as one 16-byte value per pixel.
// k_image_sum: one lane per pixel adds the moduli (or real parts) of its baselines in the definition's order.
// No LDS, no atomics, no scratch.
// Host side: pb_imager is a job of csrc/pb_job.h (stream, stage events and times, owned buffers, teardown); it has no
// handle, so its errors go through img_fail / g_imager_err and its buffers are allocated once, at create.
#include "pb_job.h"
#include "rotation_dev.h"      // img_rotation: the header's binary32 polynomial

#define IMG_PX 8            // pixels of a workgroup's tile (libpb.py: IMAGE_PX)
#define IMG_MAX_NBL 256

struct ImgArgs {
    const float2 *u;        // [nbl][2][4096]
    const double *q;        // [npix][nbl]  dd / 12500
    const double *psi;      // [npix][nbl]
    float4 *z;              // [npix][nbl]  (re, im) of slot 0, (re, im) of slot 1
    int npix, nbl;
};

struct PB_LOCAL pb_imager : PbJob<3> {      // stages: upload of dd and dpsi, kernels, copy to the host
    int device = 0, nbl = 0, max_pix = 0;
    bool has_vis = false;
    DevBuf<float2> u;
    DevBuf<double> q, psi;
    DevBuf<float4> z;
    DevBuf<float> img;
    std::vector<double> h_q, h_psi;
    std::string err;
};

static std::string g_imager_err;      // the error of a call that has no object to keep it in

static int img_fail(pb_imager *m, int rc, const std::string &what)
{
    (m ? m->err : g_imager_err) = what;
    return rc;
}

__global__ __launch_bounds__(64) void k_image_z(ImgArgs a)
{
    const int lane = threadIdx.x, b = blockIdx.y, p0 = blockIdx.x * IMG_PX;
    double q[IMG_PX], psi[IMG_PX];
#pragma unroll
    for (int i = 0; i < IMG_PX; ++i) {
        // a tile's pixels past the grid repeat its last pixel (computed, never stored): no address leaves the arrays
        const int p = p0 + i < a.npix ? p0 + i : a.npix - 1;
        q[i] = a.q[(size_t)p * a.nbl + b];
        psi[i] = a.psi[(size_t)p * a.nbl + b];
    }
    const float2 *u0 = a.u + (size_t)b * 2 * PB_NCHANOUT + lane, *u1 = u0 + PB_NCHANOUT;
    float acc[IMG_PX][4];
#pragma unroll
    for (int i = 0; i < IMG_PX; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

#pragma unroll 2
    for (int c = 0; c < PB_NCHANOUT; c += 64) {
        const float2 v0 = u0[c], v1 = u1[c];
        const double k = (double)(PB_CHANMIN + c + lane);
#pragma unroll
        for (int i = 0; i < IMG_PX; ++i) {
            const double kq = k * q[i];
            const double t = psi[i] + kq;
            const double r64 = t - rint(t);
            float cr, sr;
            img_rotation((float)r64, cr, sr);
            // one term (include/pb_hip.h), for the two product slots
            const float a0 = v0.x * cr, b0 = v0.y * sr, c0 = v0.y * cr, d0 = v0.x * sr;
            const float a1 = v1.x * cr, b1 = v1.y * sr, c1 = v1.y * cr, d1 = v1.x * sr;
            const float zr0 = a0 + b0, zi0 = c0 - d0, zr1 = a1 + b1, zi1 = c1 - d1;
            acc[i][0] = acc[i][0] + zr0;
            acc[i][1] = acc[i][1] + zi0;
            acc[i][2] = acc[i][2] + zr1;
            acc[i][3] = acc[i][3] + zi1;
        }
    }
#pragma unroll
    for (int i = 0; i < IMG_PX; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            for (int o = 32; o >= 1; o >>= 1) acc[i][j] = acc[i][j] + __shfl_down(acc[i][j], o);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < IMG_PX; ++i)
            if (p0 + i < a.npix) a.z[(size_t)(p0 + i) * a.nbl + b] = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
    }
}

__global__ __launch_bounds__(64) void k_image_sum(const float4 *z, int npix, int nbl, int mode, float *image)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= npix) return;
    const float4 *zp = z + (size_t)p * nbl;
    float s = 0.f;
    for (int b = 0; b < nbl; ++b) {
        const float4 v = zp[b];
        if (mode == PB_IMAGE_DELAY) {
            const float m0 = v.x * v.x, n0 = v.y * v.y, m1 = v.z * v.z, n1 = v.w * v.w;
            const float s0 = m0 + n0, s1 = m1 + n1;
            s = s + sqrtf(s0);
            s = s + sqrtf(s1);
        } else {
            s = s + v.x;
            s = s + v.z;
        }
    }
    image[p] = s;
}

extern "C" int pb_imager_create(int device, int nbl, int max_pix, pb_imager **out)
{
    if (!out) return img_fail(nullptr, PB_EINVAL, "pb_imager_create: out is null");
    *out = nullptr;
    if (nbl < 1 || nbl > IMG_MAX_NBL) return img_fail(nullptr, PB_EINVAL, "pb_imager_create: nbl must be 1..256");
    if (max_pix < 1) return img_fail(nullptr, PB_EINVAL, "pb_imager_create: max_pix must be positive");
    if (device < 0) return img_fail(nullptr, PB_EINVAL, "pb_imager_create: bad device id");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev)
        return img_fail(nullptr, PB_EHIP, "pb_imager_create: no HIP device (no CPU fallback)");
    pb_imager *m = new pb_imager();
    m->device = device;
    m->nbl = nbl;
    m->max_pix = max_pix;
    const size_t n = (size_t)max_pix * nbl;
    hipError_t e = m->ensure(device);
    if (e == hipSuccess) e = m->u.alloc((size_t)nbl * 2 * PB_NCHANOUT);
    if (e == hipSuccess) e = m->q.alloc(n);
    if (e == hipSuccess) e = m->psi.alloc(n);
    if (e == hipSuccess) e = m->z.alloc(n);
    if (e == hipSuccess) e = m->img.alloc((size_t)max_pix);
    if (e != hipSuccess) {
        img_fail(nullptr, PB_EHIP, std::string("pb_imager_create: ") + hipGetErrorString(e));
        pb_imager_destroy(m);
        return e == hipErrorOutOfMemory ? PB_ENOMEM : PB_EHIP;
    }
    *out = m;
    return PB_OK;
}

extern "C" void pb_imager_destroy(pb_imager *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    job_free(m);
}

extern "C" const char *pb_imager_last_error(const pb_imager *m) { return m ? m->err.c_str() : g_imager_err.c_str(); }

extern "C" int pb_imager_set_vis(pb_imager *m, const float *u)
{
    if (!m) return img_fail(nullptr, PB_EINVAL, "pb_imager_set_vis: no imager");
    if (!u) return img_fail(m, PB_EINVAL, "pb_imager_set_vis: u is null");
    HIPCHK(m, hipSetDevice(m->device));
    HIPCHK(m, m->u.from_host((const float2 *)u, m->u.cap, m->st));
    HIPCHK(m, hipStreamSynchronize(m->st));
    m->has_vis = true;
    return PB_OK;
}

extern "C" int pb_imager_run(pb_imager *m, int mode, int npix, const double *dd, const double *dpsi, float *image,
                             float *per_bl)
{
    if (!m) return img_fail(nullptr, PB_EINVAL, "pb_imager_run: no imager");
    if (mode != PB_IMAGE_DELAY && mode != PB_IMAGE_PHASE) return img_fail(m, PB_EINVAL, "pb_imager_run: mode must be 0 (delay) or 1 (phase)");
    if (npix < 1 || npix > m->max_pix) return img_fail(m, PB_EINVAL, "pb_imager_run: npix must be 1..max_pix");
    if (!dd) return img_fail(m, PB_EINVAL, "pb_imager_run: dd is null");
    if (!m->has_vis) return img_fail(m, PB_ESTATE, "pb_imager_run: no pb_imager_set_vis yet");
    const size_t n = (size_t)npix * m->nbl;
    m->h_q.resize(n);
    m->h_psi.resize(n);
    for (size_t k = 0; k < n; ++k) {
        if (!delay_ok(dd[k])) return img_fail(m, PB_EINVAL, "pb_imager_run: a dd is not finite or beyond 2^24 samples");
        if (dpsi && !std::isfinite(dpsi[k])) return img_fail(m, PB_EINVAL, "pb_imager_run: a dpsi is not finite");
        m->h_q[k] = delay_slope(dd[k]);
        m->h_psi[k] = dpsi ? dpsi[k] : 0.0;
    }
    HIPCHK(m, hipSetDevice(m->device));
    HIPCHK(m, m->mark(0));
    HIPCHK(m, m->q.from_host(m->h_q.data(), n, m->st));
    HIPCHK(m, m->psi.from_host(m->h_psi.data(), n, m->st));
    HIPCHK(m, m->mark(1));
    ImgArgs a;
    a.u = m->u.p;
    a.q = m->q.p;
    a.psi = m->psi.p;
    a.z = m->z.p;
    a.npix = npix;
    a.nbl = m->nbl;
    k_image_z<<<dim3((npix + IMG_PX - 1) / IMG_PX, m->nbl), 64, 0, m->st>>>(a);
    if (image) k_image_sum<<<(npix + 63) / 64, 64, 0, m->st>>>(m->z.p, npix, m->nbl, mode, m->img.p);
    HIPCHK(m, m->launched(2));
    HIPCHK(m, m->img.to_host(image, (size_t)npix, m->st));
    HIPCHK(m, m->z.to_host(per_bl, n, m->st));
    HIPCHK(m, m->finish());
    return PB_OK;
}

extern "C" int pb_imager_timers(const pb_imager *m, float *ms3)
{
    if (!m || !ms3) return PB_EINVAL;
    for (int k = 0; k < 3; ++k) ms3[k] = m->ms[k];
    return PB_OK;
}
