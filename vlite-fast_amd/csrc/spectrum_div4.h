// The division of the spectrum step: the four powers a thread holds, over the row's weight, behind ONE test.
// No HIP dependencies: the kernels (k_channelize.hip) and a plain host compiler build the same text
// (tests/test_spectrum_div4_cpu.py runs it over every binary32).
//
// A row without flags has the weight 1 + 2^-23, and x / (1 + 2^-23) can be had on the bits (k_channelize.hip states
// the rule and why it holds): with b the bits of x and m1 = mantissa field - 1, the quotient is  b - 2  when
// m1 >= 0x400001 (mantissa 0 wraps round to 0xffffffff) and  b - 1  otherwise, for every positive normal x from
// 0x00800002 up.  Everything else -- zeros, denormals, the two smallest normals, inf, NaN, negative values -- takes
// the IEEE division, and so does every value of a row whose weight is another one.
//
// Written per value with an early return, the range test became one exec-mask diamond around each of a thread's
// sixteen values (13 issue slots apiece).  Here the rule is applied to all four values unconditionally, the four range
// tests become one (b - 0x00800002 as an unsigned number is >= the bound exactly when b is out of range, so the
// maximum of the four decides), and the branch is taken on a vote of the whole wave: a scalar branch that is never
// taken on ordinary data.  Behind it, the lanes whose value is out of range divide.
#ifndef PB_SPECTRUM_DIV4_H
#define PB_SPECTRUM_DIV4_H

#if defined(__HIP__)
#define PB_DIV4_FN __host__ __device__ __forceinline__
#else
#define PB_DIV4_FN static inline
#endif

#define PB_DIV4_LOW 0x00800002u                    // the smallest value the bit rule is proved for
#define PB_DIV4_SPAN (0x7f800000u - PB_DIV4_LOW)   // b - LOW >= SPAN: out of the rule's range

PB_DIV4_FN unsigned pb_div4_umax(unsigned a, unsigned b) { return a > b ? a : b; }

// does any lane of the wave see `c`?  (a host thread is its own wave)
PB_DIV4_FN bool pb_div4_any(bool c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(c) != 0;
#else
    return c;
#endif
}

// p[q] <- p[q] / w, q = 0..3, bit for bit the IEEE quotient.  full_w (the same for the whole wave): w is
// 1.00000011920928955078125f = 1 + 2^-23, the bits 0x3f800001u.
PB_DIV4_FN void div_row_weight4(float (&p)[4], float w, bool full_w)
{
    unsigned b[4], over = full_w ? 0u : 0xffffffffu;
    float x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        x[q] = p[q];
        b[q] = __builtin_bit_cast(unsigned, x[q]);
        const unsigned m1 = (b[q] & 0x7fffffu) - 1u;
        p[q] = __builtin_bit_cast(float, b[q] - (m1 >= 0x400001u ? 2u : 1u));
        over = pb_div4_umax(over, b[q] - PB_DIV4_LOW);
    }
    if (__builtin_expect(pb_div4_any(over >= PB_DIV4_SPAN), 0)) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (!full_w || b[q] - PB_DIV4_LOW >= PB_DIV4_SPAN) p[q] = x[q] / w;
    }
}

#endif
