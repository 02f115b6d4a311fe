// The rotation polynomial of include/pb_hip.h (the imager's block), shared by the imager (pb_image.hip) and the
// beamformer's steering weight (pb_beamform.hip: beam_steer, for both of its calls).
#pragma once
#include <hip/hip_runtime.h>

// (cr, sr) ~ (cos 2 pi r, sin 2 pi r), |r| <= 0.5: the lines of the header, one binary32 operation each (the files that
// include this are compiled with -ffp-contract=off)
__device__ __forceinline__ void img_rotation(float r, float &cr, float &sr)
{
    const float q = rintf(4.0f * r);
    const float f = r - q * 0.25f;
    const float f2 = f * f;
    const float sn = (((-0x1.2d9b7cp+6f * f2 + 0x1.465ec4p+6f) * f2 + -0x1.4abbbap+5f) * f2 + 0x1.921fb6p+2f) * f;
    const float cs = (((0x1.d9f188p+5f * f2 + -0x1.55c64ap+6f) * f2 + 0x1.03c1dep+6f) * f2 + -0x1.3bd3ccp+4f) * f2 + 1.0f;
    const int k = (int)q;                                            // -2 .. 2
    const float a = (k & 1) ? sn : cs, b = (k & 1) ? cs : sn;        // k odd: (-+sn, +-cs)
    // the negations as sign bits: cr = -a for k & 3 in {1, 2}, sr = -b for k & 3 in {2, 3}
    cr = __uint_as_float(__float_as_uint(a) ^ ((unsigned)((k + 1) & 2) << 30));
    sr = __uint_as_float(__float_as_uint(b) ^ ((unsigned)(k & 2) << 30));
}
