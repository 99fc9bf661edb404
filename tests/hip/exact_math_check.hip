// The DEVICE build of the exact-math routines against the C library, bit for bit, on the GPU.
//
// sincos_exact.h, pow_exact.h and the division helpers of envs_classic.h restate glibc's sin / cos / fmod / pow(x, 2) / powf(x, 2) and the compiler's
// float64 division.  tests/test_sincos_exact.py and tests/test_pow_exact.py check them as HOST code; this program checks what the kernels execute:
// every member of mi::ExactMathT<true> (constant Horner steps as inline-asm v_fma_f64) and mi::ExactMathT<false> (the builtin), called from
// 256-thread workgroups with the tables and the fill_hot constants in LDS (init<true, true>(), default MI_HOT_TRIG), plus
// SharedDivisor(b).under(a) behind the call sites' range tests and div_unscaled; and log1p_exact.h's log1p_neg_unit (glibc's log1p on (-1, 0], the tail
// of mjx::standard_normal), which has one form only.
//
// Reference: the running C library on the host side of this program (sin, cos, fmod, pow, powf, log1p looked up with dlsym, so that the compiler cannot fold
// pow(x, 2.0) into x * x), and the host's a / b for the divisions.  Bit patterns are compared; NaN matches NaN; the sign of a zero counts.
// With --vectors FILE the same kernels also run on recorded arguments and results (tests/golden/exact_math_vectors.npz written out flat by
// tests/test_gpu_exact_math.py), which pins the device to the reference's libm whatever this machine's is.
//
// Every kernel is launched twice on the same inputs and the two outputs must be identical ("relaunch." cases: the launch-to-launch flips of
// profiles/r03_acrobot_inline_asm_nondeterminism.txt).
//
// Output: `case <name> checked N mismatches M` per case (the first ten mismatches of a case are printed); exit status 0 only when every M is 0.
// What is NOT claimed and only reported: sin / cos at |x| >= 105414336 (the header hands over to the platform's routine there).
// --describe: no GPU, no HIP call: generates the same inputs and prints what they contain (tests/test_exact_math_check.py asserts on that).
// Build: hipcc --offload-arch=gfx950 <build.FLAGS> -I gymnasium_amd/csrc exact_math_check.hip -ldl
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "envs_classic.h"
#include "log1p_exact.h"

typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------------------------------------------------------
enum Op { SIN, COS, SINCOS, SPREAD, SIN_B, COS_B, SINCOS_B, COS_BL, MAIN_UNCHECKED, FMOD, SQ, SQ2, SQ3, SQ_PLAIN, SQF, SQF_PLAIN, DIV_SHARED, DIV_UNSCALED, LOG1P, N_OPS };
enum Dom { D_ALL, D_LIBM, D_BOUNDED, D_MAIN, D_FLAG };

__device__ __host__ static inline bool libm_range(u64 xb) {  // where the unbounded forms are glibc's algorithm (or return NaN): not the ocml hand-over
    const uint32_t k = (uint32_t)(xb >> 32) & 0x7fffffffu;
    return k < 0x419921fbu || k >= 0x7ff00000u;
}
__device__ __host__ static inline double as_double(u64 b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}
__device__ __host__ static inline u64 as_bits(double d) {
    u64 b;
    memcpy(&b, &d, 8);
    return b;
}
__device__ __host__ static inline bool in_domain(int dom, u64 xb) {
    const double ax = fabs(as_double(xb));
    return dom == D_ALL || (dom == D_LIBM && libm_range(xb)) || (dom == D_BOUNDED && ax < 105414336.0) || (dom == D_MAIN && ax < 0.85546875);
}

template <class M, int OP>
__global__ __launch_bounds__(256) void member(const void *xv, const void *yv, void *o0v, void *o1v, long n, u64 base) {
    M::template init<true, true>();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double *x = (const double *)xv, *y = (const double *)yv;
    double *o0 = (double *)o0v, *o1 = (double *)o1v;
    double s = 0.0, c = 0.0;
    if constexpr (OP == SIN) {
        o0[i] = M::sin(x[i]);
    } else if constexpr (OP == COS) {
        o0[i] = M::cos(x[i]);
    } else if constexpr (OP == SINCOS) {
        M::sincos(x[i], s, c);
        o0[i] = s, o1[i] = c;
    } else if constexpr (OP == SPREAD) {
        M::sincos_spread(x[i], s, c);
        o0[i] = s, o1[i] = c;
    } else if constexpr (OP == SIN_B || OP == COS_B || OP == COS_BL || OP == SINCOS_B) {  // the caller's promise: |x| < 105414336
        const double v = x[i];
        if (fabs(v) < 105414336.0) {
            if constexpr (OP == SIN_B) s = M::sin_bounded(v);
            if constexpr (OP == COS_B) s = M::cos_bounded(v);
            if constexpr (OP == COS_BL) s = M::cos_bounded_literals(v);
            if constexpr (OP == SINCOS_B) M::sincos_bounded(v, s, c);
        }
        o0[i] = s;
        if constexpr (OP == SINCOS_B) o1[i] = c;
    } else if constexpr (OP == MAIN_UNCHECKED) {
        // evaluated whatever the range, as CartPole's step does -- up to the magnitudes tests/wide_states.py feeds it -- and kept only where in_main_range
        const double v = x[i];
        if (M::in_main_range(v) || fabs(v) <= 1e5) M::sincos_main_unchecked(v, s, c);
        if (!M::in_main_range(v)) s = c = 0.0;
        o0[i] = s, o1[i] = c;
    } else if constexpr (OP == FMOD) {
        o0[i] = M::fmod_2pi(x[i]);
    } else if constexpr (OP == SQ) {
        o0[i] = M::sq(x[i]);
    } else if constexpr (OP == SQ2) {
        M::sq2(x[2 * i], x[2 * i + 1], s, c);
        o0[2 * i] = s, o0[2 * i + 1] = c;
    } else if constexpr (OP == SQ3) {
        double t;
        M::sq3(x[3 * i], x[3 * i + 1], x[3 * i + 2], s, c, t);
        o0[3 * i] = s, o0[3 * i + 1] = c, o0[3 * i + 2] = t;
    } else if constexpr (OP == SQ_PLAIN) {
        const bool p = M::sq_is_plain(x[i], s);
        o0[i] = s, ((u64 *)o1v)[i] = p;
    } else if constexpr (OP == SQF || OP == SQF_PLAIN) {
        const uint32_t pat = xv ? ((const uint32_t *)xv)[i] : (uint32_t)(base + (u64)i);
        const float v = mi_pow::from_bitsf(pat);
        if constexpr (OP == SQF) {
            ((uint32_t *)o0v)[i] = mi_pow::bitsf(M::sqf(v));
        } else {
            float hi;
            const bool p = M::sqf_is_plain(v, hi);
            ((uint32_t *)o0v)[i] = mi_pow::bitsf(hi), ((uint32_t *)o1v)[i] = p;
        }
    } else if constexpr (OP == DIV_SHARED) {
        // CartPoleAttrT::attrs_arrive / by_total_mass (Acrobot's d1 is the same with the divisor always inside the range)
        const double a = x[i], b = y[i];
        const uint32_t e = (uint32_t)(mi_sincos::bits(b) >> 52) & 0x7ffu;
        const bool shared = e >= 1023u - 20u && e <= 1023u + 19u;
        const mi::SharedDivisor by(shared ? b : 1.0);
        double q = by.under(a);
        if (__builtin_expect(!(shared & mi::SharedDivisor::ordinary(a)), 0)) q = a / b;
        o0[i] = q;
    } else if constexpr (OP == DIV_UNSCALED) {
        o0[i] = mi::div_unscaled(x[i], y[i]);
    } else if constexpr (OP == LOG1P) {  // mjx::standard_normal's tail (mjx_kernels.h); not a member of the math policies: M only loads its tables
        o0[i] = mi_log1p::log1p_neg_unit(x[i]);
    }
}

struct Result {
    u64 checked, bad;
    long long idx[10];
    u64 got[10];
};
__device__ static void tally(Result *r, bool valid, bool bad, long i, u64 got) {
    const u64 v = __ballot(valid);
    if (valid && (u64)__ffsll((long long)v) - 1 == (u64)(threadIdx.x & 63)) atomicAdd(&r->checked, (u64)__popcll(v));
    if (valid && bad) {
        const u64 slot = atomicAdd(&r->bad, 1ull);
        if (slot < 10) r->idx[slot] = i, r->got[slot] = got;
    }
}
__global__ __launch_bounds__(256) void compare64(const u64 *got, const u64 *ref, const u64 *x, const u64 *flag, long n, int dom, Result *r) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const u64 g = in ? got[i] : 0, w = in ? ref[i] : 0;
    const bool valid = in && (dom == D_FLAG ? flag[i] != 0 : in_domain(dom, dom == D_ALL ? 0 : x[i]));
    const u64 mag = 0x7fffffffffffffffull, inf = 0x7ff0000000000000ull;
    const bool same = g == w || ((g & mag) > inf && (w & mag) > inf);
    tally(r, valid, !same, i, g);
}
__global__ __launch_bounds__(256) void compare32(const uint32_t *got, const uint32_t *ref, const uint32_t *flag, long n, Result *r) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const uint32_t g = in ? got[i] : 0, w = in ? ref[i] : 0;
    const bool valid = in && (!flag || flag[i] != 0);
    const bool same = g == w || ((g & 0x7fffffffu) > 0x7f800000u && (w & 0x7fffffffu) > 0x7f800000u);
    tally(r, valid, !same, i, g);
}
__global__ __launch_bounds__(256) void identical(const u64 *a, const u64 *b, long n, Result *r) {  // two launches of one kernel: every bit
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const u64 g = in ? a[i] : 0, w = in ? b[i] : 0;
    tally(r, in, g != w, i, w);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------------
#define CHECK(e)                                                                                 \
    do {                                                                                         \
        hipError_t err_ = (e);                                                                   \
        if (err_ != hipSuccess) {                                                                \
            std::printf("hip error %s at line %d\n", hipGetErrorString(err_), __LINE__);          \
            std::fflush(stdout);                                                                 \
            std::exit(2);                                                                        \
        }                                                                                        \
    } while (0)

typedef double (*fn1_t)(double);
typedef double (*fn2_t)(double, double);
typedef float (*fn2f_t)(float, float);
static fn1_t volatile ref_sin, ref_cos, ref_log1p;
static fn2_t volatile ref_fmod, ref_pow;
static fn2f_t volatile ref_powf;
static const double kTwoPi = 6.283185307179586;

static int g_threads = 1;
static const int kSlices = 64;  // fixed, so that what a scan collects does not depend on the number of threads
template <class F>
static void parallel_for(long n, F f) {  // f(lo, hi, slice)
    std::atomic<int> next{0};
    auto work = [&] {
        for (;;) {
            const int s = next++;
            if (s >= kSlices) break;
            f(n * s / kSlices, n * (s + 1) / kSlices, s);
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < g_threads; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}

// counter-based generator: value k of stream s, the same whatever thread asks
static inline u64 mix(u64 z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline u64 rnd(u64 stream, u64 k) { return mix(mix(stream * 0xD1B54A32D192ED03ull + 12345) + k); }
static inline double u01(u64 r) { return (double)(r >> 11) * 0x1p-53; }
static inline double uniform(u64 r, double lo, double hi) { return lo + (hi - lo) * u01(r); }
static inline double pow2_random(u64 r, int e) {  // 2^e * [1, 2), random sign
    return as_double((r & 0x800fffffffffffffull) | ((u64)(1023 + e) << 52));
}
static inline double next_up(double v) { return std::nextafter(v, INFINITY); }
static inline double next_down(double v) { return std::nextafter(v, -INFINITY); }
static inline bool same64(u64 a, u64 b) {
    const u64 mag = 0x7fffffffffffffffull, inf = 0x7ff0000000000000ull;
    return a == b || ((a & mag) > inf && (b & mag) > inf);
}
static inline bool ordinary(double a) { return (((uint32_t)(as_bits(a) >> 32) & 0x7fffffffu) - 0x20000000u) < 0x40000000u; }  // SharedDivisor::ordinary

// ---- the inputs ----------------------------------------------------------------------------------------------------------------------------
static const char *kClassNames[8] = {"below_2^-27", "below_2^-26", "taylor", "table", "quarter", "reduced", "beyond", "nonfinite"};
static int trig_class(double x) {  // the branches of s_sin.c as sincos_exact.h restates them
    const uint32_t k = (uint32_t)(as_bits(x) >> 32) & 0x7fffffffu;
    if (k >= 0x7ff00000u) return 7;
    if (k < 0x3e400000u) return 0;
    if (k < 0x3e500000u) return 1;
    if (std::fabs(x) < 0.126) return 2;
    if (k < 0x3feb6000u) return 3;
    if (k < 0x400368fdu) return 4;
    if (k < 0x419921fbu) return 5;
    return 6;
}
static const double kTrigEdges[19] = {0x1p-27, 0x1p-26, 0.126, 0.855469, 0.8554688, 2.426265, 105414350.0, 105414336.0 /* the hand-over itself: high word 0x419921fb */, 0.7853981633974483, 1.5707963267948966, 3.141592653589793,
                                      4.71238898038469, 6.283185307179586, 1.0 / 128, 0.5 / 128, 109.5 / 128, 110.0 / 128, 1.5707963267948966 - 0.126,
                                      1.5707963267948966 - 0.855469};
static void trig_edge_inputs(std::vector<double> &X) {  // tests/test_sincos_exact.py::test_bit_identical_around_every_branch_point_and_special_values
    for (double e : kTrigEdges)
        for (int sgn = 0; sgn < 2; sgn++)
            for (long d = -2000; d <= 2000; d++) {
                const double v = as_double(as_bits(e) + (u64)d);
                X.push_back(sgn ? -v : v);
            }
    for (int t = 0; t <= 220; t++) {
        const double v = t / 256.0;
        X.push_back(v), X.push_back(next_up(v)), X.push_back(next_down(v)), X.push_back(-v);
    }
    const double special[] = {0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-300, 1e-30, INFINITY, -INFINITY, NAN, 1e10, -1e10, 1e300};
    for (double v : special) X.push_back(v);
    for (long k = 0; k < 200000; k++) X.push_back(uniform(rnd(11, k), -1.0, 1.0) * std::ldexp(1.0, -1070 + (int)(rnd(12, k) % 1050)));
}
static void trig_inputs(std::vector<double> &X) {
    const double ranges[6] = {0.86, 2.45, 3.1415926535897936, 100.0, 1.0e6, 1.2e8};  // test_bit_identical_to_libm_on_random_arguments, 2^24 arguments each
    const long per = 1L << 24;
    X.resize(6 * per);
    for (int r = 0; r < 6; r++)
        parallel_for(per, [&](long lo, long hi, int) {
            for (long k = lo; k < hi; k++) X[r * per + k] = uniform(rnd(20 + r, k), -ranges[r], ranges[r]);
        });
    trig_edge_inputs(X);
}
static void sort_by_class(std::vector<double> &X) {  // stable: wavefronts of one branch range each
    std::vector<double> out(X.size());
    long at[9] = {0};
    for (double v : X) at[trig_class(v) + 1]++;
    for (int c = 0; c < 8; c++) at[c + 1] += at[c];
    for (double v : X) out[at[trig_class(v)]++] = v;
    X.swap(out);
}
static long gcd(long a, long b) { return b ? gcd(b, a % b) : a; }
static void spread(const std::vector<double> &X, std::vector<double> &Y) {  // neighbouring lanes take arguments a golden-ratio stride apart in the sorted set: every wavefront mixes the ranges
    const long n = (long)X.size();
    long a = (long)(n * 0.6180339887498949) | 1;
    while (gcd(a, n) != 1) a += 2;
    Y.resize(n);
    parallel_for(n, [&](long lo, long hi, int) {
        for (long j = lo; j < hi; j++) Y[j] = X[(long)(((unsigned __int128)j * (u64)a + 12345) % (u64)n)];
    });
}
static void describe_trig(const char *name, const std::vector<double> &X) {
    long cls[8] = {0}, uniform_waves = 0, mixed_waves = 0, main_only_waves = 0;
    for (size_t w = 0; w < X.size(); w += 64) {
        int first = -1;
        bool mixed = false, main_only = true;
        for (size_t k = w; k < std::min(X.size(), w + 64); k++) {
            const int c = trig_class(X[k]);
            cls[c]++;
            if (first < 0) first = c;
            mixed |= c != first;
            main_only &= c <= 3;
        }
        (mixed ? mixed_waves : uniform_waves)++;
        main_only_waves += main_only;
    }
    std::printf("describe %s arguments=%zu", name, X.size());
    for (int c = 0; c < 8; c++) std::printf(" %s=%ld", kClassNames[c], cls[c]);
    std::printf(" uniform_wavefronts=%ld mixed_wavefronts=%ld main_first_wavefronts=%ld\n", uniform_waves, mixed_waves, main_only_waves);
}

static bool fmod_in_domain(double x) { return std::fabs(x) < 0x1p52 * kTwoPi; }
static void fmod_big_inputs(std::vector<double> &X, long randoms, long multiples) {  // per binade of the quotient, 2^20 .. 2^52
    for (int b = 20; b < 52; b++) {
        for (long k = 0; k < randoms; k++) {
            const u64 r = rnd(40 + b, k);
            const double v = std::ldexp(1.0 + u01(r), b) * kTwoPi;
            X.push_back((r & 1) ? -v : v);
        }
        for (long k = 0; k < multiples; k++) {
            const u64 r = rnd(80 + b, k);
            const double q = (double)((1ull << b) + (r >> 1) % (1ull << b)), m = (r & 1) ? -(q * kTwoPi) : q * kTwoPi;
            X.push_back(m), X.push_back(next_up(m)), X.push_back(next_down(m));
        }
    }
}
static void fmod_inputs(std::vector<double> &X) {  // tests/test_sincos_exact.py::test_fmod_by_a_constant_is_the_c_library_fmod, then the large quotients
    for (long k = 0; k < 2000000; k++) X.push_back(uniform(rnd(30, k), -50, 50));
    for (long k = 0; k < 1000000; k++) X.push_back(uniform(rnd(31, k), -1e6, 1e6));
    for (long k = 0; k < 500000; k++) X.push_back(uniform(rnd(32, k), -1e12, 1e12));
    for (long k = 0; k < 200000; k++) X.push_back(uniform(rnd(33, k), -1.0, 1.0) * std::ldexp(1.0, -1070 + (int)(rnd(34, k) % 1070)));
    for (long k = -5000; k <= 5000; k++) {
        const double m = (double)k * kTwoPi;
        X.push_back(m), X.push_back(next_up(m)), X.push_back(next_down(m));
    }
    const double special[] = {0.0, -0.0, kTwoPi, -kTwoPi, 3.141592653589793, 1e15};
    for (double v : special) X.push_back(v);
    fmod_big_inputs(X, 1L << 16, 1L << 14);
    X.erase(std::remove_if(X.begin(), X.end(), [](double v) { return !fmod_in_domain(v); }), X.end());
}
static void describe_fmod(const std::vector<double> &X) {
    long binade[64] = {0}, small = 0;
    for (double v : X) {
        const double q = std::floor(std::fabs(v) / kTwoPi);
        const int b = q >= 1.0 ? std::ilogb(q) : -1;
        (b >= 20 && b < 64 ? binade[b] : small)++;
    }
    std::printf("describe fmod_2pi arguments=%zu quotient_below_2^20=%ld", X.size(), small);
    for (int b = 20; b < 52; b++) std::printf(" quotient_2^%d=%ld", b, binade[b]);  // [2^b, 2^(b+1))
    std::printf("\n");
}

static const double kSqSpecial[18] = {0.0, -0.0, 1.0, -1.0, INFINITY, -INFINITY, 5e-324, 1e-200, 1e200, 1e-160, 1e154, 0x1p-95, 0x1p95, 0x1.fffffffffffffp-1, 0x1.0000000000001p+0,
                                      1.4142135623730951, 0x1.6a09e667f3bccp+0, 1.4142135623730951 * 0x1p20};
static bool pow_differs(double x) { return !same64(as_bits(ref_pow(x, 2.0)), as_bits(x * x)); }
static void find_hard(std::vector<double> &hard) {  // arguments with pow(x, 2) != x * x, found by scanning the reference
    std::vector<double> part[kSlices];
    parallel_for(1L << 24, [&](long lo, long hi, int s) {
        for (long k = lo; k < hi; k++) {
            const double x = uniform(rnd(50, k), -10, 10);
            if (pow_differs(x)) part[s].push_back(x);
        }
    });
    for (auto &p : part) hard.insert(hard.end(), p.begin(), p.end());
}
static void sq_inputs(std::vector<double> &X, const std::vector<double> &hard) {
    const double ranges[5][2] = {{-10, 10}, {-1, 1}, {0.99, 1.01}, {-1e-3, 1e-3}, {-1e5, 1e5}};  // test_square_is_bit_identical_to_libm_pow
    for (int r = 0; r < 5; r++)
        for (long k = 0; k < (1L << 21); k++) X.push_back(uniform(rnd(60 + r, k), ranges[r][0], ranges[r][1]));
    X.insert(X.end(), hard.begin(), hard.end());
    const double special[] = {0.0, -0.0, 1.0, -1.0, 2.0, 0.5, 0x1.0000000000001p+0, 0x1.fffffffffffffp-1, 1e-200, 1e200, 5e-324, INFINITY, -INFINITY, 1e-160, 1e154, 3.0, -8.0, NAN};
    for (double v : special) X.push_back(v);
}
// the flat array both sq2 (pairs) and sq3 (triples) read: its length is a multiple of 6
static void group_inputs(std::vector<double> &F, const std::vector<double> &hard, long &hard_from, long &hard_count) {
    const double ranges[3] = {10.0, 0.1, 30.0};  // test_grouped_squares_are_bit_identical_to_libm_pow
    for (int r = 0; r < 3; r++)
        for (long k = 0; k < 6 * (1L << 17); k++) F.push_back(uniform(rnd(70 + r, k), -ranges[r], ranges[r]));
    hard_from = (long)F.size(), hard_count = (long)hard.size() / 6 * 6;  // groups made ONLY of hard arguments
    F.insert(F.end(), hard.begin(), hard.begin() + hard_count);
    auto h = [&](size_t k) { return hard.empty() ? 3.0 : hard[k % hard.size()]; };
    for (int k = 0; k < 18; k++) F.push_back(kSqSpecial[k]), F.push_back(h(k)), F.push_back(kSqSpecial[(k + 17) % 18]);  // test_grouped_squares_with_several_hard_arguments_per_group
    for (int k = 0; k < 18; k++) F.push_back(h(k)), F.push_back(kSqSpecial[k]), F.push_back(kSqSpecial[k]);
    const double nan_group[6] = {NAN, 3.0, h(0), h(1), NAN, 0.5};
    F.insert(F.end(), nan_group, nan_group + 6);
}

static void shared_divisor_inputs(std::vector<double> &A, std::vector<double> &B) {
    const long n = 1L << 24;
    A.resize(n), B.resize(n);
    parallel_for(n, [&](long lo, long hi, int) {
        for (long k = lo; k < hi; k++) {
            const u64 r = rnd(90, k), s = rnd(91, k), t = rnd(92, k);
            B[k] = (r & 7) == 0 ? uniform(s, 2.5, 4.5) : pow2_random(s, -20 + (int)((r >> 3) % 40));  // Acrobot's d1 / any exponent of [2^-20, 2^20), either sign
            double a;
            if ((r >> 16) % 32 == 0) {  // outside ordinary(): the call sites divide the long way
                switch ((r >> 24) % 6) {
                case 0: a = (t & 1) ? -0.0 : 0.0; break;
                case 1: a = as_double(t & 0x800fffffffffffffull); break;                   // subnormal
                case 2: a = pow2_random(t, -1022 + (int)((r >> 32) % 511)); break;           // 2^-1022 .. 2^-511
                case 3: a = pow2_random(t, 513 + (int)((r >> 32) % 511)); break;             // 2^513 .. 2^1024
                case 4: a = (t & 1) ? -INFINITY : INFINITY; break;
                default: a = NAN;
                }
            } else {
                a = pow2_random(t, -511 + (int)((r >> 32) % 1024));  // log-uniform over [2^-511, 2^513), either sign
            }
            A[k] = a;
        }
    });
    const double db[] = {0x1p-20, next_up(0x1p-20), next_down(0x1p-20), 0x1p20, next_down(0x1p20), next_down(next_down(0x1p20)), 2.5, next_up(2.5), next_down(2.5), 4.5, next_up(4.5),
                         next_down(4.5), 1.1, 1.0, 3.0};
    const double da[] = {0x1p-511, next_up(0x1p-511), next_down(0x1p-511), 0x1p513, next_down(0x1p513), next_down(next_down(0x1p513)), next_up(0x1p513), 1.0, 9.8, 0.0, 5e-324, 0x1p-1022, 1e-300,
                         1e300, 1.7976931348623157e308, INFINITY, NAN};
    for (double b : db)
        for (double a : da)
            for (int sg = 0; sg < 4; sg++) A.push_back((sg & 1) ? -a : a), B.push_back((sg & 2) ? -b : b);
}
static void div_unscaled_inputs(std::vector<double> &A, std::vector<double> &B) {  // the ranges of tests/hip/div_unscaled_check.hip
    const double lo = 0x1p-969, hi = 2e221;
    const double xe[] = {lo, next_up(lo), 1.2e-269, 1.24e-269, 1e-100, 1.0, 9.8, hi, next_down(hi), 1e200};
    const double ye[] = {0.6, 0.6212121212121212, 0.621212121212121, 0.6474747474747475, 0.64747474747475, 0.65, 0.66, 0.625};
    for (double a : xe)
        for (double b : ye) A.push_back(a), B.push_back(b), A.push_back(-a), B.push_back(b);
    const double top = std::log2(hi);
    for (long k = 0; k < (1L << 22); k++) {
        const u64 r = rnd(95, k);
        const double m = std::exp2(uniform(rnd(96, k), -969.0, top));
        A.push_back((k & 3) == 0 ? uniform(rnd(96, k), -40, 40) : ((r & 1) ? -m : m)), B.push_back(uniform(rnd(97, k), 0.6, 0.66));
    }
}

// ---- cases -------------------------------------------------------------------------------------------------------------------------------
struct Case {
    std::string name;
    u64 checked = 0, bad = 0;
};
static std::vector<Case> g_cases;
static Case &get_case(const std::string &name) {
    for (auto &c : g_cases)
        if (c.name == name) return c;
    g_cases.push_back(Case{name});
    return g_cases.back();
}

static const long kChunk = 3L << 22;  // 64-bit words per device buffer (a multiple of 6 and of 256)
static void *d_x, *d_y, *d_r0, *d_r1, *d_a0, *d_a1, *d_b0, *d_b1;
static Result *d_res;
static const u64 *h_x, *h_y, *h_r0, *h_r1;  // the chunk that is on the device, for the mismatch lines
static u64 h_base;                          // ... or its first pattern when the arguments are the patterns themselves (the float32 scan)

typedef void (*kern_t)(const void *, const void *, void *, void *, long, u64);
template <class M>
static kern_t pick(int op) {
    switch (op) {
#define PICK(o) \
    case o: return member<M, o>;
        PICK(SIN) PICK(COS) PICK(SINCOS) PICK(SPREAD) PICK(SIN_B) PICK(COS_B) PICK(SINCOS_B) PICK(COS_BL) PICK(MAIN_UNCHECKED) PICK(FMOD) PICK(SQ) PICK(SQ2) PICK(SQ3)
        PICK(SQ_PLAIN) PICK(SQF) PICK(SQF_PLAIN) PICK(DIV_SHARED) PICK(DIV_UNSCALED) PICK(LOG1P)
#undef PICK
    }
    return nullptr;
}
static dim3 grid(long n) { return dim3((unsigned)((n + 255) / 256)); }
static Result fetch() {
    Result r;
    CHECK(hipMemcpy(&r, d_res, sizeof r, hipMemcpyDeviceToHost));
    return r;
}
static void upload(const u64 *x, const u64 *y, const u64 *r0, const u64 *r1, long words) {
    h_x = x, h_y = y, h_r0 = r0, h_r1 = r1;
    if (x) CHECK(hipMemcpy(d_x, x, 8 * words, hipMemcpyHostToDevice));
    if (y) CHECK(hipMemcpy(d_y, y, 8 * words, hipMemcpyHostToDevice));
    if (r0) CHECK(hipMemcpy(d_r0, r0, 8 * words, hipMemcpyHostToDevice));
    if (r1) CHECK(hipMemcpy(d_r1, r1, 8 * words, hipMemcpyHostToDevice));
}
enum Print { P_F64, P_F32, P_WORDS32 };  // how report() prints a mismatch: float64 values, float32 values, or a 64-bit word that packs two float32 results
static void report(Case &c, const Result &r, const u64 *want, Print how) {
    for (u64 k = 0; k < std::min<u64>(r.bad, 10) && c.bad + k < 10; k++) {
        const long long i = r.idx[k];
        if (how == P_F32) {
            const uint32_t xb = h_x ? ((const uint32_t *)h_x)[i] : (uint32_t)(h_base + (u64)i), wb = want ? ((const uint32_t *)want)[i] : 0, gb = (uint32_t)r.got[k];
            float xf, wf, gf;
            memcpy(&xf, &xb, 4), memcpy(&wf, &wb, 4), memcpy(&gf, &gb, 4);
            std::printf("  mismatch %s x=%.9g (0x%08x) got=%.9g (0x%08x) want=%.9g (0x%08x)\n", c.name.c_str(), xf, xb, gf, gb, wf, wb);
        } else if (how == P_WORDS32) {
            const uint32_t x0 = h_x ? ((const uint32_t *)h_x)[2 * i] : (uint32_t)(h_base + 2 * (u64)i), x1 = h_x ? ((const uint32_t *)h_x)[2 * i + 1] : x0 + 1;
            std::printf("  mismatch %s results of x=0x%08x and x=0x%08x: second launch 0x%08x 0x%08x\n", c.name.c_str(), x0, x1, (uint32_t)r.got[k], (uint32_t)(r.got[k] >> 32));
        } else {
            std::printf("  mismatch %s x=%.17g (0x%016llx)", c.name.c_str(), as_double(h_x[i]), h_x[i]);
            if (h_y) std::printf(" y=%.17g (0x%016llx)", as_double(h_y[i]), h_y[i]);
            std::printf(" got=%.17g (0x%016llx)", as_double(r.got[k]), r.got[k]);
            if (want) std::printf(" want=%.17g (0x%016llx)", as_double(want[i]), want[i]);
            std::printf("\n");
        }
    }
    c.checked += r.checked, c.bad += r.bad;
}
// One member of the math policies and how its outputs are judged
struct Member {
    const char *name;
    int op;
    int dom = D_ALL;                          // which arguments are compared (Dom)
    int ref0 = 0, ref1 = -1;                  // the reference array (0: d_r0, 1: d_r1) output 0 / output 1 is compared with; -1: no such output
    const char *sub0 = "", *sub1 = nullptr;   // what the outputs add to the case name
    bool flagged = false;                     // output 1 is a flag: output 0 is compared where it is set (the is_plain tests)
    bool is32 = false;                        // float32 member: a 64-bit word of a buffer holds two results
    bool patterns = false;                    // float32 member whose arguments are the bit patterns base, base + 1, ... themselves
    u64 base = 0;
};
// `m` on the chunk that upload() put on the device, for both math policies: two launches, the first compared with the reference, both with each other.
// threads: how many lanes; words: how many 64-bit words each output holds
static void run_member(const Member &m, const std::string &tag, long threads, long words) {
    const long cmp_n = m.is32 ? words * 2 : words;
    for (int kasm = 1; kasm >= 0; kasm--) {
        const kern_t k = kasm ? pick<mi::ExactMathT<true>>(m.op) : pick<mi::ExactMathT<false>>(m.op);
        const std::string who = std::string(m.name) + (kasm ? ".kasm" : ".builtin");
        const bool two = m.sub1 != nullptr || m.flagged;
        for (int launch = 0; launch < 2; launch++) {
            hipLaunchKernelGGL(k, grid(threads), dim3(256), 0, 0, m.patterns ? nullptr : d_x, d_y, launch ? d_b0 : d_a0, launch ? d_b1 : d_a1, threads, m.base);
            CHECK(hipGetLastError());
        }
        for (int o = 0; o < (two && !m.flagged ? 2 : 1); o++) {
            const int ref = o ? m.ref1 : m.ref0;
            Case &c = get_case(who + (o ? m.sub1 : m.sub0) + "." + tag);
            CHECK(hipMemset(d_res, 0, sizeof(Result)));
            if (m.is32)
                hipLaunchKernelGGL(compare32, grid(cmp_n), dim3(256), 0, 0, (const uint32_t *)d_a0, (const uint32_t *)d_r0, m.flagged ? (const uint32_t *)d_a1 : nullptr, cmp_n, d_res);
            else
                hipLaunchKernelGGL(compare64, grid(cmp_n), dim3(256), 0, 0, (const u64 *)(o ? d_a1 : d_a0), (const u64 *)(ref ? d_r1 : d_r0), (const u64 *)d_x, (const u64 *)d_a1, cmp_n,
                                   m.flagged ? (int)D_FLAG : m.dom, d_res);
            CHECK(hipGetLastError());
            report(c, fetch(), ref ? h_r1 : h_r0, m.is32 ? P_F32 : P_F64);
        }
        Case &again = get_case("relaunch." + who + "." + tag);
        for (int o = 0; o < (two ? 2 : 1); o++) {
            CHECK(hipMemset(d_res, 0, sizeof(Result)));
            hipLaunchKernelGGL(identical, grid(words), dim3(256), 0, 0, (const u64 *)(o ? d_a1 : d_a0), (const u64 *)(o ? d_b1 : d_b0), words, d_res);
            CHECK(hipGetLastError());
            report(again, fetch(), nullptr, m.is32 ? P_WORDS32 : P_F64);
        }
    }
}
static Member member_of(const char *name, int op, int dom = D_ALL, int ref0 = 0) {
    Member m{name, op};
    m.dom = dom, m.ref0 = ref0;
    return m;
}
static Member pair_of(const char *name, int op, int dom) {  // sin in output 0, cos in output 1
    Member m{name, op};
    m.dom = dom, m.ref1 = 1, m.sub0 = ".s", m.sub1 = ".c";
    return m;
}

static void check_trig(const double *x, const u64 *rs, const u64 *rc, long n, const std::string &tag) {
    upload((const u64 *)x, nullptr, rs, rc, n);
    run_member(member_of("sin", SIN, D_LIBM, 0), tag, n, n);
    run_member(member_of("cos", COS, D_LIBM, 1), tag, n, n);
    run_member(pair_of("sincos", SINCOS, D_LIBM), tag, n, n);
    run_member(pair_of("sincos_spread", SPREAD, D_LIBM), tag, n, n);
    run_member(member_of("sin_bounded", SIN_B, D_BOUNDED, 0), tag, n, n);
    run_member(member_of("cos_bounded", COS_B, D_BOUNDED, 1), tag, n, n);
    run_member(pair_of("sincos_bounded", SINCOS_B, D_BOUNDED), tag, n, n);
    run_member(member_of("cos_bounded_literals", COS_BL, D_BOUNDED, 1), tag, n, n);
    run_member(pair_of("sincos_main_unchecked", MAIN_UNCHECKED, D_MAIN), tag, n, n);
}
static u64 g_beyond = 0, g_beyond_differ = 0;  // the ocml hand-over beyond 105414350: reported, not claimed
static void trig_set(const std::vector<double> &X, const std::string &tag, bool count_beyond) {
    std::vector<u64> rs(kChunk), rc(kChunk);
    for (long off = 0; off < (long)X.size(); off += kChunk) {
        const long n = std::min<long>(kChunk, (long)X.size() - off);
        parallel_for(n, [&](long lo, long hi, int) {
            for (long k = lo; k < hi; k++) rs[k] = as_bits(ref_sin(X[off + k])), rc[k] = as_bits(ref_cos(X[off + k]));
        });
        check_trig(X.data() + off, rs.data(), rc.data(), n, tag);
        if (count_beyond) {  // (d_a0 / d_a1 hold the last member's outputs; run sin once more for the record)
            std::vector<u64> got(n);
            hipLaunchKernelGGL(pick<mi::ExactMathT<true>>(SIN), grid(n), dim3(256), 0, 0, d_x, d_y, d_a0, d_a1, n, 0);
            CHECK(hipGetLastError());
            CHECK(hipMemcpy(got.data(), d_a0, 8 * n, hipMemcpyDeviceToHost));
            for (long k = 0; k < n; k++)
                if (!libm_range(as_bits(X[off + k]))) g_beyond++, g_beyond_differ += !same64(got[k], rs[k]);
        }
    }
}
static void check_fmod(const std::vector<double> &X, const std::vector<u64> &ref, const std::string &tag) {
    for (long off = 0; off < (long)X.size(); off += kChunk) {
        const long n = std::min<long>(kChunk, (long)X.size() - off);
        upload((const u64 *)X.data() + off, nullptr, ref.data() + off, nullptr, n);
        run_member(member_of("fmod_2pi", FMOD), tag, n, n);
    }
}
static void check_sq(const std::vector<double> &X, const std::vector<u64> &ref, const std::string &tag) {
    for (long off = 0; off < (long)X.size(); off += kChunk) {
        const long n = std::min<long>(kChunk, (long)X.size() - off);
        upload((const u64 *)X.data() + off, nullptr, ref.data() + off, nullptr, n);
        run_member(member_of("sq", SQ), tag, n, n);
        Member plain = member_of("sq_is_plain", SQ_PLAIN);
        plain.flagged = true;
        run_member(plain, tag, n, n);
    }
}
static void check_groups(const std::vector<double> &F, const std::vector<u64> &ref, const std::string &tag) {  // F.size() % 6 == 0
    for (long off = 0; off < (long)F.size(); off += kChunk) {
        const long n = std::min<long>(kChunk, (long)F.size() - off);
        upload((const u64 *)F.data() + off, nullptr, ref.data() + off, nullptr, n);
        run_member(member_of("sq2", SQ2), tag, n / 2, n);
        run_member(member_of("sq3", SQ3), tag, n / 3, n);
    }
}
static void check_sqf(const uint32_t *x, const uint32_t *ref, long n, u64 base, const std::string &tag) {  // n even; x == nullptr: the patterns base .. base + n - 1
    upload((const u64 *)x, nullptr, (const u64 *)ref, nullptr, n / 2);
    h_base = base;
    Member sqf = member_of("sqf", SQF), plain = member_of("sqf_is_plain", SQF_PLAIN);
    sqf.is32 = plain.is32 = true, sqf.patterns = plain.patterns = x == nullptr, sqf.base = plain.base = base;
    plain.flagged = true;
    run_member(sqf, tag, n, n / 2);
    run_member(plain, tag, n, n / 2);
}
static void check_div(const char *name, int op, const std::vector<double> &A, const std::vector<double> &B) {
    std::vector<u64> ref(A.size());
    for (size_t k = 0; k < A.size(); k++) ref[k] = as_bits(A[k] / B[k]);
    for (long off = 0; off < (long)A.size(); off += kChunk) {
        const long n = std::min<long>(kChunk, (long)A.size() - off);
        upload((const u64 *)A.data() + off, (const u64 *)B.data() + off, ref.data() + off, nullptr, n);
        const kern_t k = pick<mi::ExactMathT<true>>(op);
        Case &c = get_case(std::string(name) + ".ieee"), &again = get_case(std::string("relaunch.") + name + ".ieee");
        for (int launch = 0; launch < 2; launch++) {
            hipLaunchKernelGGL(k, grid(n), dim3(256), 0, 0, d_x, d_y, launch ? d_b0 : d_a0, launch ? d_b1 : d_a1, n, 0);
            CHECK(hipGetLastError());
        }
        CHECK(hipMemset(d_res, 0, sizeof(Result)));
        hipLaunchKernelGGL(compare64, grid(n), dim3(256), 0, 0, (const u64 *)d_a0, (const u64 *)d_r0, (const u64 *)d_x, (const u64 *)d_a1, n, (int)D_ALL, d_res);
        CHECK(hipGetLastError());
        report(c, fetch(), h_r0, P_F64);
        CHECK(hipMemset(d_res, 0, sizeof(Result)));
        hipLaunchKernelGGL(identical, grid(n), dim3(256), 0, 0, (const u64 *)d_a0, (const u64 *)d_b0, n, d_res);
        CHECK(hipGetLastError());
        report(again, fetch(), nullptr, P_F64);
    }
    h_y = nullptr;
}

// ---- log1p(-u), u in [0, 1): log1p_exact.h, the tail of mjx::standard_normal ------------------------------------------------------------------
// Per binade [2^-(b+1), 2^-b) of u, b = 0 .. 52: u = m 2^-53 as Pcg64::next_double gives it (the low b significand bits zero), u with every significand bit
// random, and the 2^15 doubles upwards of the binade's lower end; then the neighbourhoods of the routine's branch points.
static const long kLog1pGrid = 1L << 17, kLog1pEdge = 1L << 15;
static void log1p_inputs(std::vector<double> &X) {
    for (int b = 0; b < 53; b++) {
        for (long k = 0; k < 2 * kLog1pGrid; k++) {
            u64 m = (rnd(900 + b, (u64)k) >> 12) | (1ull << 52);
            if (k < kLog1pGrid) m &= ~((1ull << b) - 1);
            X.push_back(-std::ldexp((double)m * 0x1p-53, -b));
        }
        const u64 lo = as_bits(std::ldexp(0.5, -b));
        for (long k = 0; k < kLog1pEdge; k++) X.push_back(-as_double(lo + (u64)k));
    }
    // branch points: 2^-29 and 2^-54 (the short forms), 1 - sqrt(2)/2 (k = 0 from there down) and u = 1 - 2^-j (1 + x crosses a power of two), the ends
    const double edges[] = {0x1p-29, 0x1p-54, 0.2928932188134524, 0.5, 0.75, 0.875, 0.9375, 1.0 - 0x1p-20, 1.0 - 0x1p-40};
    for (double e : edges)
        for (long d = -4096; d <= 4096; d++) X.push_back(-as_double(as_bits(e) + (u64)d));
    for (long d = 0; d < 4096; d++) X.push_back(-as_double(as_bits(1.0) - 1 - (u64)d));  // the largest u
    X.push_back(-0.0), X.push_back(-0x1p-53), X.push_back(-0x1p-52);
}
static void describe_log1p(const std::vector<double> &X) {
    long binade[53] = {0}, grid = 0, short_form = 0, direct = 0, reduced = 0, zero = 0;
    for (double x : X) {
        const double u = -x;
        if (u == 0.0) {
            zero++;
            continue;
        }
        int e;
        std::frexp(u, &e);  // u in [2^(e-1), 2^e)
        if (-e >= 0 && -e < 53) binade[-e]++;
        grid += std::ldexp(u, 53) == std::floor(std::ldexp(u, 53));
        const uint32_t ax = (uint32_t)(as_bits(x) >> 32) & 0x7fffffffu;
        if (ax < 0x3e200000u) short_form++;
        else if (ax <= 0x3fd2bec3u) direct++;
        else reduced++;
    }
    std::printf("describe log1p_neg_unit arguments=%zu zero=%ld generator_grid=%ld below_2^-29=%ld direct=%ld reduced=%ld", X.size(), zero, grid, short_form, direct, reduced);
    for (int b = 0; b < 53; b++) std::printf(" u_2^-%d=%ld", b + 1, binade[b]);
    std::printf("\n");
}
static void check_log1p(const double *x, const u64 *ref, long total, const std::string &tag) {
    for (long off = 0; off < total; off += kChunk) {
        const long n = std::min<long>(kChunk, total - off);
        upload((const u64 *)x + off, nullptr, ref + off, nullptr, n);
        const kern_t k = pick<mi::ExactMathT<true>>(LOG1P);
        Case &c = get_case("log1p_neg_unit." + tag), &again = get_case("relaunch.log1p_neg_unit." + tag);
        for (int launch = 0; launch < 2; launch++) {
            hipLaunchKernelGGL(k, grid(n), dim3(256), 0, 0, d_x, d_y, launch ? d_b0 : d_a0, launch ? d_b1 : d_a1, n, 0);
            CHECK(hipGetLastError());
        }
        CHECK(hipMemset(d_res, 0, sizeof(Result)));
        hipLaunchKernelGGL(compare64, grid(n), dim3(256), 0, 0, (const u64 *)d_a0, (const u64 *)d_r0, (const u64 *)d_x, (const u64 *)d_a1, n, (int)D_ALL, d_res);
        CHECK(hipGetLastError());
        report(c, fetch(), h_r0, P_F64);
        CHECK(hipMemset(d_res, 0, sizeof(Result)));
        hipLaunchKernelGGL(identical, grid(n), dim3(256), 0, 0, (const u64 *)d_a0, (const u64 *)d_b0, n, d_res);
        CHECK(hipGetLastError());
        report(again, fetch(), nullptr, P_F64);
    }
}

// the float32 scan: all 2^32 patterns, `step` at a time; with_gpu = false: only count (--describe)
static void sqf_scan(bool with_gpu, bool with_libm) {
    const long step = 2 * kChunk;
    std::vector<uint32_t> ref(step);
    u64 differ = 0, patterns = 0;
    for (u64 base = 0; base < (1ull << 32); base += step) {
        const long n = (long)std::min<u64>(step, (1ull << 32) - base);
        std::atomic<u64> d{0};
        parallel_for(n, [&](long lo, long hi, int) {
            u64 mine = 0;
            for (long k = lo; k < hi; k++) {
                const uint32_t pat = (uint32_t)(base + k);
                float v, p;
                memcpy(&v, &pat, 4);
                const float w = ref_powf(v, 2.0f);
                p = v * v;
                memcpy(&ref[k], &w, 4);
                mine += !(w == p || (w != w && p != p));
            }
            d += mine;
        });
        differ += d, patterns += n;
        if (with_gpu && with_libm) check_sqf(nullptr, ref.data(), n, base, "all");
    }
    std::printf("describe sqf patterns=%llu powf_ne_product=%llu\n", patterns, differ);
}

// ---- the recorded vectors (--vectors): u64 words; "EXMATHV1", then sections {id, n, payload}: 1 trig x sin cos, 2 fmod x r, 3 pow x r, 4 powf x r (32-bit values widened),
// 5 log1p x r (tests/golden/normal_sampler.npz: the calls of its tail lanes)
static bool read_vectors(const char *path, std::vector<std::vector<u64>> sec[6]) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    std::vector<u64> w;
    u64 buf[4096];
    size_t got;
    while ((got = std::fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + got);
    std::fclose(f);
    if (w.empty() || memcmp(&w[0], "EXMATHV1", 8) != 0) return false;
    size_t at = 1;
    while (at + 2 <= w.size()) {
        const u64 id = w[at], n = w[at + 1];
        const int arrays = id == 1 ? 3 : 2;
        if (id < 1 || id > 5 || at + 2 + arrays * n > w.size()) return false;
        for (int a = 0; a < arrays; a++) sec[id].emplace_back(w.begin() + at + 2 + a * n, w.begin() + at + 2 + (a + 1) * n);
        at += 2 + arrays * n;
    }
    return at == w.size();
}
static int vectors_leg(const char *path) {
    std::vector<std::vector<u64>> sec[6];
    if (!read_vectors(path, sec) || sec[1].size() != 3 || sec[2].size() != 2 || sec[3].size() != 2 || sec[4].size() != 2 || sec[5].size() != 2) {
        std::printf("vectors: cannot read %s\n", path);
        return 2;
    }
    if ((long)sec[1][0].size() > kChunk || (long)sec[3][0].size() > kChunk) return 2;
    check_trig((const double *)sec[1][0].data(), sec[1][1].data(), sec[1][2].data(), (long)sec[1][0].size(), "vectors");
    std::vector<double> fx((const double *)sec[2][0].data(), (const double *)sec[2][0].data() + sec[2][0].size());
    check_fmod(fx, sec[2][1], "vectors");
    std::vector<double> px((const double *)sec[3][0].data(), (const double *)sec[3][0].data() + sec[3][0].size());
    check_sq(px, sec[3][1], "vectors");
    px.resize(px.size() / 6 * 6);
    check_groups(px, sec[3][1], "vectors");
    const long nf = (long)sec[4][0].size() / 2 * 2;
    std::vector<uint32_t> x32(nf), r32(nf);
    for (long k = 0; k < nf; k++) x32[k] = (uint32_t)sec[4][0][k], r32[k] = (uint32_t)sec[4][1][k];
    check_sqf(x32.data(), r32.data(), nf, 0, "vectors");
    check_log1p((const double *)sec[5][0].data(), sec[5][1].data(), (long)sec[5][0].size(), "vectors");
    std::printf("vectors: %zu sin / cos, %zu fmod, %zu pow, %ld powf, %zu log1p rows\n", sec[1][0].size(), fx.size(), sec[3][0].size(), nf, sec[5][0].size());
    return 0;
}

int main(int argc, char **argv) {
    bool describe = false;
    const char *vectors = nullptr;
    for (int a = 1; a < argc; a++) {
        if (!strcmp(argv[a], "--describe")) describe = true;
        else if (!strcmp(argv[a], "--vectors") && a + 1 < argc) vectors = argv[++a];
        else {
            std::printf("usage: exact_math_check [--describe] [--vectors FILE]\n");
            return 2;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    g_threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    void *libm = dlopen("libm.so.6", RTLD_NOW);
    if (!libm) libm = RTLD_DEFAULT;
    ref_sin = (fn1_t)dlsym(libm, "sin"), ref_cos = (fn1_t)dlsym(libm, "cos"), ref_fmod = (fn2_t)dlsym(libm, "fmod"), ref_pow = (fn2_t)dlsym(libm, "pow");
    ref_powf = (fn2f_t)dlsym(libm, "powf"), ref_log1p = (fn1_t)dlsym(libm, "log1p");
    if (!ref_sin || !ref_cos || !ref_fmod || !ref_pow || !ref_powf || !ref_log1p) {
        std::printf("libm: sin / cos / fmod / pow / powf / log1p not found\n");
        return 2;
    }
    // known answers of glibc's FMA build (the tests/test_sincos_exact.py and tests/test_pow_exact.py guards)
    const bool expected = as_bits(ref_sin(0.5)) == 0x3fdeaee8744b05f0ull && as_bits(ref_cos(0.5)) == 0x3fec1528065b7d50ull && as_bits(ref_pow(1.3, 2.0)) == 0x3ffb0a3d70a3d70bull;
    if (expected)
        std::printf("libm: the expected glibc FMA build\n");
    else
        std::printf("libm: NOT the expected glibc FMA build (sin(0.5)=%a cos(0.5)=%a pow(1.3,2)=%a): libm comparison skipped\n", ref_sin(0.5), ref_cos(0.5), ref_pow(1.3, 2.0));
    const bool with_libm = expected || describe;

    if (!describe) {
        for (void **p : {&d_x, &d_y, &d_r0, &d_r1, &d_a0, &d_a1, &d_b0, &d_b1}) {
            CHECK(hipMalloc(p, 8 * kChunk));
            CHECK(hipMemset(*p, 0, 8 * kChunk));
        }
        CHECK(hipMalloc((void **)&d_res, sizeof(Result)));
        if (vectors)
            if (int rc = vectors_leg(vectors)) return rc;
    }
    {  // the divisions: IEEE on the host is the reference, whatever the libm
        std::vector<double> A, B;
        shared_divisor_inputs(A, B);
        long outside = 0, b_outside = 0, acrobot = 0;
        for (size_t k = 0; k < A.size(); k++) {
            const double ab = std::fabs(B[k]);
            outside += !ordinary(A[k]), b_outside += !(ab >= 0x1p-20 && ab < 0x1p20), acrobot += B[k] >= 2.5 && B[k] <= 4.5;
        }
        std::printf("describe shared_divisor pairs=%zu numerators_outside_ordinary=%ld numerators_ordinary=%ld divisors_outside_range=%ld divisors_2.5_to_4.5=%ld\n", A.size(), outside,
                    (long)A.size() - outside, b_outside, acrobot);
        if (!describe) check_div("shared_divisor", DIV_SHARED, A, B);
        A.clear(), B.clear();
        div_unscaled_inputs(A, B);
        std::printf("describe div_unscaled pairs=%zu\n", A.size());
        if (!describe) check_div("div_unscaled", DIV_UNSCALED, A, B);
    }
    if (with_libm) {
        {
            std::vector<double> X, Y;
            trig_inputs(X);
            sort_by_class(X);
            describe_trig("trig.sorted", X);
            if (!describe) trig_set(X, "sorted", true);
            spread(X, Y);
            std::vector<double>().swap(X);
            describe_trig("trig.shuffled", Y);
            if (!describe) trig_set(Y, "shuffled", false);
        }
        {
            std::vector<double> X;
            fmod_inputs(X);
            describe_fmod(X);
            if (!describe) {
                std::vector<u64> ref(X.size());
                parallel_for((long)X.size(), [&](long lo, long hi, int) {
                    for (long k = lo; k < hi; k++) ref[k] = as_bits(ref_fmod(X[k], kTwoPi));
                });
                check_fmod(X, ref, "libm");
            }
        }
        {
            std::vector<double> hard, X, F;
            find_hard(hard);
            sq_inputs(X, hard);
            long hard_from = 0, hard_count = 0;
            group_inputs(F, hard, hard_from, hard_count);
            std::vector<u64> rx(X.size()), rf(F.size());
            std::atomic<long> dx{0};
            parallel_for((long)X.size(), [&](long lo, long hi, int) {
                long mine = 0;
                for (long k = lo; k < hi; k++) rx[k] = as_bits(ref_pow(X[k], 2.0)), mine += !same64(rx[k], as_bits(X[k] * X[k]));
                dx += mine;
            });
            parallel_for((long)F.size(), [&](long lo, long hi, int) {
                for (long k = lo; k < hi; k++) rf[k] = as_bits(ref_pow(F[k], 2.0));
            });
            long all_hard[4] = {0}, df = 0;
            for (int w = 2; w <= 3; w++)
                for (size_t g = 0; g + w <= F.size(); g += w) {
                    bool all = true;
                    for (int k = 0; k < w; k++) all &= !same64(rf[g + k], as_bits(F[g + k] * F[g + k]));
                    all_hard[w] += all;
                }
            for (size_t k = 0; k < F.size(); k++) df += !same64(rf[k], as_bits(F[k] * F[k]));
            std::printf("describe sq arguments=%zu pow_ne_product=%ld\n", X.size(), (long)dx);
            std::printf("describe sq_groups arguments=%zu pow_ne_product=%ld all_hard_groups_sq2=%ld all_hard_groups_sq3=%ld\n", F.size(), df, all_hard[2], all_hard[3]);
            if (!describe) check_sq(X, rx, "libm"), check_groups(F, rf, "libm");
        }
        {
            std::vector<double> X;
            log1p_inputs(X);
            describe_log1p(X);
            if (!describe) {
                std::vector<u64> ref(X.size());
                parallel_for((long)X.size(), [&](long lo, long hi, int) {
                    for (long k = lo; k < hi; k++) ref[k] = as_bits(ref_log1p(X[k]));
                });
                check_log1p(X.data(), ref.data(), (long)X.size(), "libm");
            }
        }
        sqf_scan(!describe, expected);
    }
    if (describe) return 0;
    if (g_beyond) std::printf("beyond 105414336 (the hand-over to the platform's sin, not claimed): %llu of %llu arguments differ from libm\n", g_beyond_differ, g_beyond);
    bool ok = true;
    for (const auto &c : g_cases) {
        std::printf("case %s checked %llu mismatches %llu\n", c.name.c_str(), c.checked, c.bad);
        ok &= c.bad == 0;
    }
    std::printf("elapsed %.1f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return ok ? 0 : 1;
}
