// lane_common.h -- the device helpers every family's kernels use (classic_kernels.h, tabular_kernels.h, the utility kernels of engine.hip and
// mj_glue_kernels.h): the lane's statistics and their per-workgroup totals, the sub-environment's generator in memory, the output function of a PCG64 state.
#ifndef MI355ENV_LANE_COMMON_H
#define MI355ENV_LANE_COMMON_H
#include "engine_types.h"

namespace {

struct LaneStats {
    uint32_t env_steps, reset_steps, episodes;
    uint64_t length_sum;
    double return_sum;
};

// step_kernel's form of load_lane + load_rng: the raw words are REQUESTED here and looked at only after the math tables are staged (arrive()),
// held opaque in between -- the compiler otherwise starts on them at once (the first 128-bit multiply of the generator is speculated out of
// the reset branch), i.e. waits for this trip to memory before it requests the tables: two trips in a row where one does.
template <class T>
MI_DEV void hold_opaque(T &x) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "one or two VGPRs");
    asm volatile("" : "+v"(x));
}
MI_DEV Pcg64 load_rng(const DevEnv &d, int i) {
    Pcg64 r;
    r.state = make_u128(d.rng[i], d.rng[(size_t)d.N + i]);
    r.inc = make_u128(d.rng[(size_t)2 * d.N + i], d.rng[(size_t)3 * d.N + i]);
    return r;
}
MI_DEV void store_rng_state(const DevEnv &d, int i, const Pcg64 &r) {
    d.rng[i] = (uint64_t)(r.state >> 64), d.rng[(size_t)d.N + i] = (uint64_t)r.state;
}

// XSL-RR output of a PCG64 state (the state AFTER its step: what the action-stream lanes hold)
MI_DEV uint64_t pcg_output(u128 state) {
    const uint64_t hi = (uint64_t)(state >> 64), lo = (uint64_t)state;
    const uint64_t x = hi ^ lo;
    const unsigned rot = (unsigned)(hi >> 58);
    return (x >> rot) | (x << ((0u - rot) & 63u));
}

MI_DEV double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
MI_DEV uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor((int)v, off, 64);
    return v;
}
MI_DEV uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_xor((long long)v, off, 64);
    return v;
}

// Per-workgroup totals: wavefront butterflies, 4 partials through LDS, one plain read-modify-write of the
// workgroup's own slot (no atomics: 1024 same-address atomics would cost more than the whole step).
// The workgroup's previous totals as step_kernel loads them AHEAD (with the lane's state): the read-modify-write at the end of the kernel is
// then a plain store, not one more dependent trip to memory in a kernel whose whole run time is a handful of such trips.
struct BlockTotals {
    uint64_t count;  // threads 0..3: blk_count[block][thread]
    double ret;      // thread 64: blk_ret[block]
    bool loaded;
};
MI_DEV BlockTotals block_totals_load(const DevEnv &d) {
    BlockTotals t = {0ull, 0.0, true};
    if (threadIdx.x < 4) t.count = d.blk_count[(size_t)blockIdx.x * 4 + threadIdx.x];
    if (threadIdx.x == 64) {
        uint32_t zero = 0;  // (an offset the compiler cannot see through: a VECTOR load that stays in flight -- the uniform address would make it an s_load, which the wavefront waits for on the spot)
        hold_opaque(zero);
        t.ret = d.blk_ret[(size_t)blockIdx.x + zero];
    }
    return t;
}
MI_DEV void block_accumulate(const DevEnv &d, const LaneStats &st, const BlockTotals &before = BlockTotals{0ull, 0.0, false}) {
    __shared__ uint64_t sh_c[4][kBlock / 64];
    __shared__ double sh_r[kBlock / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t c0 = wave_sum(st.env_steps), c1 = wave_sum(st.reset_steps), c2 = wave_sum(st.episodes);
    // c2 is wavefront-uniform: the two wide reductions are skipped by wavefronts in which no episode finished
    const uint64_t c3 = c2 ? wave_sum(st.length_sum) : 0;
    const double r = c2 ? wave_sum(st.return_sum) : 0.0;
    if (lane == 0) sh_c[0][wave] = c0, sh_c[1][wave] = c1, sh_c[2][wave] = c2, sh_c[3][wave] = c3, sh_r[wave] = r;
    __syncthreads();
    if (threadIdx.x < 4) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) t += sh_c[threadIdx.x][w];
        if (t) {
            uint64_t *slot = &d.blk_count[(size_t)blockIdx.x * 4 + threadIdx.x];
            *slot = (before.loaded ? before.count : *slot) + t;
        }
    } else if (threadIdx.x == 64) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) t += sh_r[w];
        if (t != 0.0) d.blk_ret[blockIdx.x] = (before.loaded ? before.ret : d.blk_ret[blockIdx.x]) + t;
    }
}

}  // namespace
#endif  // MI355ENV_LANE_COMMON_H
