// log1p_exact.h -- log1p(-u), u in [0, 1), the way the reference computes it: glibc's log1p, bit for bit.
//
// NumPy's Generator.standard_normal draws the ziggurat's tail (|x| > R = 3.654, one draw in ~4 000) as R + (-1/R) log1p(-u), with the C
// library's log1p (numpy/random/src/distributions/distributions.c random_standard_normal): every bit of it goes into the velocities of a
// HalfCheetah / Ant / InvertedDoublePendulum reset (mjx_kernels.h standard_normal).  glibc's log1p is accurate to below one ulp, not correctly
// rounded: it misses the correctly rounded result for ~7 % of these arguments, so a device log1p that is merely accurate disagrees with
// NumPy in the last bit of a few percent of the tail draws.  This is glibc's routine (sysdeps/ieee754/dbl-64/s_log1p.c, the FreeBSD msun /
// Sun fdlibm algorithm; x86-64 has no FMA variant of it: every operation is rounded separately) restated for the one domain the sampler
// uses, x = -u in (-1, 0]:
//   |x| < 2^-29:          x - x^2 / 2 (x itself below 2^-54);
//   x > -0.2929:          f = x, k = 0;
//   otherwise:            1 + x = 2^k (1 + f), sqrt(2)/2 < 1 + f < sqrt(2), with the correction term c = (x - ((1 + x) - 1)) / (1 + x);
//   log1p(f) = f - f^2/2 + s (f^2/2 + R(s^2)), s = f / (2 + f), R the degree-14 polynomial Lp1 .. Lp7 in the four-way split form glibc
//   evaluates; result k ln2_hi - ((f^2/2 - (s (f^2/2 + R) + (k ln2_lo + c))) - f).
// Arguments outside (-1, 0] are not the sampler's and are not handled (x > 0 would need the k > 0 correction term, x <= -1 the pole).
// Checked against the running libm on 10^8 arguments over every binade of u, and on the recorded vectors of tests/golden/normal_sampler.npz,
// by tests/test_log1p_exact.py (host build) and tests/test_gpu_exact_math.py (device build).
// Compile with -ffp-contract=off.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define MI_L1_DEV __device__ __forceinline__
#else
#define MI_L1_DEV static inline
#endif

namespace mi_log1p {

MI_L1_DEV uint64_t bits(double x) {
    union { double d; uint64_t u; } v;
    v.d = x;
    return v.u;
}
MI_L1_DEV double from_bits(uint64_t u) {
    union { double d; uint64_t u; } v;
    v.u = u;
    return v.d;
}
MI_L1_DEV double with_high_word(double x, uint32_t hi) { return from_bits(((uint64_t)hi << 32) | (bits(x) & 0xffffffffull)); }

// log1p(x) for x in (-1, 0]
MI_L1_DEV double log1p_neg_unit(double x) {
    const double ln2_hi = from_bits(0x3fe62e42fee00000ull), ln2_lo = from_bits(0x3dea39ef35793c76ull);
    const double Lp1 = from_bits(0x3FE5555555555593ull), Lp2 = from_bits(0x3FD999999997FA04ull), Lp3 = from_bits(0x3FD2492494229359ull),
                 Lp4 = from_bits(0x3FCC71C51D8E78AFull), Lp5 = from_bits(0x3FC7466496CB03DEull), Lp6 = from_bits(0x3FC39A09D078C69Full),
                 Lp7 = from_bits(0x3FC2F112DF3E5244ull);
    const int32_t hx = (int32_t)(bits(x) >> 32);
    const int32_t ax = hx & 0x7fffffff;
    if (ax < 0x3e200000) {                  // |x| < 2^-29
        if (ax < 0x3c900000) return x;      // |x| < 2^-54 (here: -0.0)
        return x - x * x * 0.5;
    }
    int32_t k = 1, hu = 1;
    double f = x, c = 0.0;
    if (hx <= (int32_t)0xbfd2bec3) {        // -0.2929 < x
        k = 0;
    } else {
        double u = 1.0 + x;
        hu = (int32_t)(bits(u) >> 32);
        k = (hu >> 20) - 1023;              // <= 0 on this domain
        c = x - (u - 1.0);                  // correction term (exactly 0 for the sampler's u = m 2^-53: 1 - u is representable)
        c /= u;
        hu &= 0x000fffff;
        if (hu < 0x6a09e) {
            u = with_high_word(u, (uint32_t)hu | 0x3ff00000u);  // normalize u
        } else {
            k += 1;
            u = with_high_word(u, (uint32_t)hu | 0x3fe00000u);  // normalize u / 2
            hu = (0x00100000 - hu) >> 2;
        }
        f = u - 1.0;
    }
    const double hfsq = 0.5 * f * f;
    if (hu == 0) {                          // |f| < 2^-20
        if (f == 0.0) {
            if (k == 0) return 0.0;
            c += k * ln2_lo;
            return k * ln2_hi + c;
        }
        const double R = hfsq * (1.0 - 0.66666666666666666 * f);
        if (k == 0) return f - R;
        return k * ln2_hi - ((R - (k * ln2_lo + c)) - f);
    }
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double R1 = z * Lp1, z2 = z * z;
    const double R2 = Lp2 + z * Lp3, z4 = z2 * z2;
    const double R3 = Lp4 + z * Lp5, z6 = z4 * z2;
    const double R4 = Lp6 + z * Lp7;
    const double R = R1 + z2 * R2 + z4 * R3 + z6 * R4;
    if (k == 0) return f - (hfsq - s * (hfsq + R));
    return k * ln2_hi - ((hfsq - (s * (hfsq + R) + (k * ln2_lo + c))) - f);
}

}  // namespace mi_log1p
