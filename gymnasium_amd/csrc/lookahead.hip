// lookahead.hip -- mi_lookahead's kernels as their own translation unit: namespace mi_lookahead_unit, the launch function engine.hip calls (engine_types.h
// declares it) and every instantiation of lookahead_kernel.
//
// What it computes (include/mi355env.h mi_lookahead): for every sub-environment i, the discounted return of K candidate action sequences of length H,
// each started from a PRIVATE copy of lane i -- state, elapsed steps, flags, attribute registers, generator -- with lane_step's own sequence per step
// (validity check, E::step, elapsed += 1, TimeLimit) and stopped after the first step that terminates or truncates.  The env is only read.
//
// How: one lane per candidate, lane j = k * N + i.  The lane's state and attributes are loaded from row i of the env's arrays (consecutive lanes,
// consecutive addresses, except where j wraps around N), its actions from [t][j], its results go to [j].  Nothing is stored inside the step loop and the
// loop has no data-dependent control flow of its own: a candidate that has finished keeps stepping from the state it finished in -- that state is held
// by selects, so it is finite and it is what final_obs reports -- and its return, step count and flags are held the same way (lane_step_fused's idiom:
// the classic kernels are issue-bound).  The next step's action is requested one step ahead.
//
// Why a unit, why max-ILP (build.py TU_FLAGS): classic.hip's reasons -- at 65 536 lanes one wavefront runs per SIMD and hides latency with its own
// independent instructions.  Unlike the rollouts there is no trajectory traffic to overlap, so there is no second role; instead the kernels are
// bounded to half the register file (two wavefronts per SIMD beyond 65 536 lanes) which costs no instantiation a spill (kLookWaves, below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_step.h"

namespace {

struct LookPtrs {
    const void *actions;  // [H][K * N] E::Act
    double *returns;      // [K * N]
    int32_t *steps;       // [K * N]
    uint8_t *terminated, *truncated;
    float *final_obs;     // [K * N][OBS]
    int H, KN;
    double gamma;
};

// wavefronts per SIMD the kernels' registers are bounded for: at most 256 registers each.  Every instantiation fits without a spill -- the widest,
// Acrobot with per-lane attributes (~20 attribute registers next to four RK4 stages), at 241; docs/results_log.md has the table.
constexpr int kLookWaves = 2;

template <class E>
__global__ __launch_bounds__(kBlock, kLookWaves) void lookahead_kernel(DevEnv d, LookPtrs io, AttrDev at) {
    typedef typename E::Act Act;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const bool live = j < io.KN;
    const int i = live ? j % d.N : 0;
    const Act *acts = static_cast<const Act *>(io.actions);
    // everything the lane reads before its first step -- state, elapsed | flags, attributes, generator (a type whose step draws), first action -- is
    // requested before the math tables are staged into LDS: one trip to memory, not two (step_kernel's order)
    double s[E::S];
    uint32_t meta = 0;
    uint64_t g[4] = {0, 0, 0, 0};
    Act a_next = (Act)0;
    AttrRequest<E> ar;
    if (live) {
#pragma unroll
        for (int k = 0; k < E::S; k++) s[k] = d.state[(size_t)k * d.N + i];
        meta = d.meta[i];
        if constexpr (HasStepDraws<E>::value) {
#pragma unroll
            for (int k = 0; k < 4; k++) g[k] = d.rng[(size_t)k * d.N + i];
        }
        ar.request(at, d, i);
        a_next = acts[j];
    }
    tables_init<E>();
    if (!live) return;
    Lane<E> L;
#pragma unroll
    for (int k = 0; k < E::S; k++) hold_opaque(s[k]), L.s[k] = s[k];
    hold_opaque(meta), hold_opaque(a_next);
    L.elapsed = meta & kElapsedMask, L.flags = meta >> kFlagShift;
    trig_invalidate(L.trig);
    ar.arrive(L.trig);
    [[maybe_unused]] Pcg64 gen;  // the sub-environment's generator, copied: every candidate of i sees the draws the env would see next
    if constexpr (HasStepDraws<E>::value) {
#pragma unroll
        for (int k = 0; k < 4; k++) hold_opaque(g[k]);
        gen.state = make_u128(g[0], g[1]), gen.inc = make_u128(g[2], g[3]);
    }
    // a lane that waits for its reset (NEXT_STEP, DISABLED) has nothing to look ahead from: it starts finished
    // (integers, not bools, for what lives across the loop: ResetQueue::have's reason)
    uint32_t active = (L.flags & kNeedsReset) ? 0u : 1u, te_last = 0u, tr_last = 0u, bad_any = 0u;
    int32_t steps = 0;
    double G = 0.0, disc = 1.0;
    const size_t KN = (size_t)io.KN;
    for (int t = 0; t < io.H; t++) {
        Act a = a_next;
        const int tn = t + 1 < io.H ? t + 1 : t;
        a_next = acts[(size_t)tn * KN + j];
        // lane_step: an action outside the space is reported through the sticky error word and the lane is left untouched
        const bool bad = active && !E::valid(a);
        bad_any |= bad ? 1u : 0u;
        a = bad ? (Act)0 : a;
        const bool go = active && !bad;
        if constexpr (HasStepDraws<E>::value) {
            if (go && E::step_draws(L.trig)) E::step_drawn(L.trig, gen.next_double());
        }
        double s0[E::S];
#pragma unroll
        for (int k = 0; k < E::S; k++) s0[k] = L.s[k];
        uint32_t sflags = L.flags;
        double rew;
        bool te;
        E::step(L.s, sflags, a, d.P, rew, te, L.trig);
        const uint32_t elapsed = L.elapsed + 1u;  // TimeLimit.step (wrappers/common.py:129-133)
        const bool tr = d.max_steps > 0 && (int)elapsed >= d.max_steps;
#pragma unroll
        for (int k = 0; k < E::S; k++) L.s[k] = go ? L.s[k] : s0[k];
        L.flags = go ? sflags : L.flags;
        L.elapsed = go ? elapsed : L.elapsed;
        const double term = disc * rew;  // (rounded before the sum: -ffp-contract=off)
        G = go ? G + term : G;
        disc = go ? disc * io.gamma : disc;
        steps += go ? 1 : 0;
        te_last = go ? (te ? 1u : 0u) : te_last;
        tr_last = go ? (tr ? 1u : 0u) : tr_last;
        active = (go && (te || tr)) ? 0u : active;
    }
    if (bad_any) *d.error = kErrInvalidAction;
    if (io.returns) io.returns[j] = G;
    if (io.steps) io.steps[j] = steps;
    if (io.terminated) io.terminated[j] = (uint8_t)te_last;
    if (io.truncated) io.truncated[j] = (uint8_t)tr_last;
    if (io.final_obs) {
        float o[E::OBS];
        E::obs(L.s, L.flags, o, L.trig);
        store_row<E::OBS>(io.final_obs + (size_t)j * E::OBS, o);
    }
}

template <class E>
int launch(mi_vecenv *v, const LookPtrs &p) {
    const AttrDev at = {v->d_attr, v->attr_mask};
    const unsigned grid = (unsigned)(((int64_t)p.KN + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((lookahead_kernel<E>), dim3(grid), dim3(kBlock), 0, v->stream, v->d, p, at);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// the env's kind and the element type of the action rows to the exact env type (classic.hip dispatch_kind_act_math / dispatch_kind_attr)
int launch_plain(mi_vecenv *v, const LookPtrs &p, int act_kind) {
    typedef ExactMath M;
    switch (v->cfg.kind) {
    case MI_ENV_CARTPOLE: return launch<CartPoleT<M>>(v, p);
    case MI_ENV_PENDULUM: return act_kind != MI_F32 ? launch<PendulumT<M, ActF64>>(v, p) : launch<PendulumT<M>>(v, p);
    case MI_ENV_ACROBOT: return launch<AcrobotT<ExactMathBuiltinFma>>(v, p);  // (the math policy of Acrobot's other kernels, envs_classic.h)
    case MI_ENV_MOUNTAIN_CAR: return launch<MountainCarT<M>>(v, p);
    case MI_ENV_MOUNTAIN_CAR_CONTINUOUS:
        if (act_kind == MI_F64) return launch<MountainCarContinuousT<M, ActF64>>(v, p);
        if (act_kind == MI_F64_WEAK) return launch<MountainCarContinuousT<M, ActF64Weak>>(v, p);
        return launch<MountainCarContinuousT<M>>(v, p);
    }
    return fail(MI_ERR_UNSUPPORTED, "mi_lookahead: the five classic-control kinds only");
}
int launch_attr(mi_vecenv *v, const LookPtrs &p, int act_kind) {
    typedef ExactMath M;
    switch (v->cfg.kind) {
    case MI_ENV_CARTPOLE: return launch<CartPoleAttrT<M>>(v, p);
    case MI_ENV_PENDULUM: return act_kind != MI_F32 ? launch<PendulumAttrT<M, ActF64>>(v, p) : launch<PendulumAttrT<M>>(v, p);
    case MI_ENV_ACROBOT: return launch<AcrobotAttrT<ExactMathBuiltinFma>>(v, p);
    case MI_ENV_MOUNTAIN_CAR: return launch<MountainCarAttrT<M>>(v, p);
    case MI_ENV_MOUNTAIN_CAR_CONTINUOUS:
        if (act_kind == MI_F64) return launch<MountainCarContinuousAttrT<M, ActF64>>(v, p);
        if (act_kind == MI_F64_WEAK) return launch<MountainCarContinuousAttrT<M, ActF64Weak>>(v, p);
        return launch<MountainCarContinuousAttrT<M>>(v, p);
    }
    return fail(MI_ERR_UNSUPPORTED, "mi_lookahead: the five classic-control kinds only");
}

}  // namespace

namespace mi_lookahead_unit {
int launch(mi_vecenv *v, const void *actions, int act_kind, int horizon, int candidates, double gamma, double *returns, int32_t *steps, uint8_t *terminated,
           uint8_t *truncated, float *final_obs) {
    const LookPtrs p = {actions, returns, steps, terminated, truncated, final_obs, horizon, candidates * v->cfg.num_envs, gamma};
    // an env on the per-lane types (mi_set_env_attr; once mi_set_step_wrappers was on) stays on them, as in mi_classic::step
    return (v->attr_mask || v->per_lane) ? launch_attr(v, p, act_kind) : launch_plain(v, p, act_kind);
}
}  // namespace mi_lookahead_unit
