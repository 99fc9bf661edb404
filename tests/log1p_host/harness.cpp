// TEST INFRASTRUCTURE: gymnasium_amd/csrc/log1p_exact.h compiled for the host (g++ -ffp-contract=off), compared with the running libm
// by tests/test_log1p_exact.py.
#include "../../gymnasium_amd/csrc/log1p_exact.h"

#include <math.h>
#include <string.h>
static inline uint64_t xs128(uint64_t s[2]) {
    uint64_t a = s[0], b = s[1];
    s[0] = b, a ^= a << 23, s[1] = a ^ b ^ (a >> 17) ^ (b >> 26);
    return s[1] + b;
}
// one argument -u with u in the binade [2^-(b+1), 2^-b), b = 0 .. 52.  mode 0: u = m 2^-53, what Pcg64::next_double gives (the low b bits of
// the significand are zero); mode 1: every significand bit random; mode 2: one of the 2^20 doubles upwards of the binade's lower end (the routine's
// branch points 2^-29 and 2^-54 are such ends)
static inline double draw(uint64_t s[2], int b, int mode) {
    const uint64_t r = xs128(s);
    uint64_t m = (r >> 12) | (1ull << 52);                  // 53-bit significand
    if (mode == 0) m &= ~((1ull << b) - 1);
    double u = (double)m * 0x1p-53;                          // [0.5, 1)
    u = __builtin_ldexp(u, -b);
    if (mode == 2) {
        double lo = __builtin_ldexp(0.5, -b);
        uint64_t bits;
        memcpy(&bits, &lo, 8);
        bits += (r >> 12) & 0xfffff;
        memcpy(&u, &bits, 8);
    }
    return -u;
}
extern "C" {
__attribute__((visibility("default"))) void log1p_batch(const double *x, double *out, long n) {
    for (long i = 0; i < n; i++) out[i] = mi_log1p::log1p_neg_unit(x[i]);
}
__attribute__((visibility("default"))) void libm_log1p_batch(const double *x, double *out, long n) {
    for (long i = 0; i < n; i++) out[i] = log1p(x[i]);
}
// out: {examined, differ from the running libm, first differing argument's bits}
__attribute__((visibility("default"))) void log1p_scan(uint64_t seed, long n, int b, int mode, uint64_t *out) {
    uint64_t s[2] = {seed * 0x9E3779B97F4A7C15ull + 1, seed ^ 0xD1B54A32D192ED03ull};
    for (int i = 0; i < 8; i++) xs128(s);
    out[0] = out[1] = out[2] = 0;
    for (long i = 0; i < n; i++) {
        const double x = draw(s, b, mode);
        const double want = log1p(x), got = mi_log1p::log1p_neg_unit(x);
        out[0]++;
        if (memcmp(&want, &got, 8) != 0) {
            if (!out[1]) memcpy(&out[2], &x, 8);
            out[1]++;
        }
    }
}
}
