// div_unscaled (envs_classic.h) against the compiler's float64 division `/`, bit for bit, on the GPU.
//
// Checked range: divisors in [0.6, 0.66] (CartPole's thetaacc divisor lies in [0.6212, 0.6475]) and numerators of either sign with magnitudes
// from 2^-969 to 2e221 -- what CartPole's range test on t3 admits (1.2e-269 .. 2e221) and more -- log-uniform, plus the edges of both
// intervals and ordinary magnitudes.  Prints "checked N mismatches M" (M must be 0), then, for the record, what happens just outside: zeros,
// subnormal and tiny numerators (the unscaled quotient may differ there; the caller keeps those lanes on the exact path).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I gymnasium_amd/csrc div_unscaled_check.hip
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "envs_classic.h"

__global__ void quotients(const double *x, const double *y, double *fast, double *ref, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        fast[i] = mi::div_unscaled(x[i], y[i]);
        ref[i] = x[i] / y[i];
    }
}

#define CHECK(e)                                                                      \
    do {                                                                              \
        hipError_t err_ = (e);                                                        \
        if (err_ != hipSuccess) {                                                     \
            std::printf("hip error %s at line %d\n", hipGetErrorString(err_), __LINE__); \
            return 2;                                                                 \
        }                                                                             \
    } while (0)

static int run(const std::vector<double> &x, const std::vector<double> &y, std::vector<double> &fast, std::vector<double> &ref) {
    const int n = (int)x.size();
    const size_t bytes = sizeof(double) * (size_t)n;
    double *dx, *dy, *df, *dr;
    CHECK(hipMalloc(&dx, bytes));
    CHECK(hipMalloc(&dy, bytes));
    CHECK(hipMalloc(&df, bytes));
    CHECK(hipMalloc(&dr, bytes));
    CHECK(hipMemcpy(dx, x.data(), bytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dy, y.data(), bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(quotients, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, df, dr, n);
    CHECK(hipGetLastError());
    fast.resize(n), ref.resize(n);
    CHECK(hipMemcpy(fast.data(), df, bytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(ref.data(), dr, bytes, hipMemcpyDeviceToHost));
    CHECK(hipFree(dx));
    CHECK(hipFree(dy));
    CHECK(hipFree(df));
    CHECK(hipFree(dr));
    return 0;
}

static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

int main() {
    std::mt19937_64 g(20261016);
    std::uniform_real_distribution<double> uy(0.6, 0.66), ue(std::log2(0x1p-969), std::log2(2e221)), uo(-40.0, 40.0), u01(0.0, 1.0);
    std::vector<double> x, y;
    const double lo = 0x1p-969, hi = 2e221;
    const double xedges[] = {lo, std::nextafter(lo, 1.0), 1.2e-269, 1.24e-269, 1e-100, 1.0, 9.8, 2e221, std::nextafter(hi, 0.0), 1e200};
    const double yedges[] = {0.6, 0.6212121212121212, 0.621212121212121, 0.6474747474747475, 0.64747474747475, 0.65, 0.66, 0.625};
    for (double a : xedges)
        for (double b : yedges)
            for (double s : {1.0, -1.0}) x.push_back(s * a), y.push_back(b);
    for (int k = 0; k < (1 << 22); k++) {
        const double m = (k & 3) == 0 ? uo(g) : std::exp2(ue(g)) * (u01(g) < 0.5 ? -1.0 : 1.0);
        x.push_back(m), y.push_back(uy(g));
    }
    std::vector<double> f, r;
    if (int rc = run(x, y, f, r)) return rc;
    size_t bad = 0;
    for (size_t k = 0; k < x.size(); k++)
        if (bits(f[k]) != bits(r[k])) {
            if (bad < 10) std::printf("mismatch x=%.17g y=%.17g fast=%.17g ref=%.17g\n", x[k], y[k], f[k], r[k]);
            bad++;
        }
    std::printf("checked %zu mismatches %zu\n", x.size(), bad);
    // outside the range, for the record
    std::vector<double> ox, oy;
    const double outside[] = {0.0, -0.0, 0x1p-1074, 0x1p-1022, 0x1p-970, 1e-300};
    for (double a : outside)
        for (double b : yedges) ox.push_back(a), oy.push_back(b), ox.push_back(-a), oy.push_back(b);
    if (int rc = run(ox, oy, f, r)) return rc;
    size_t obad = 0;
    for (size_t k = 0; k < ox.size(); k++) obad += bits(f[k]) != bits(r[k]);
    std::printf("outside the range: %zu of %zu differ\n", obad, ox.size());
    return bad == 0 ? 0 : 1;
}
