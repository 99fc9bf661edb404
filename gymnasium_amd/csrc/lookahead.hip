// lookahead.hip -- mi_lookahead's kernels as their own translation unit: namespace mi_lookahead_unit, the launch function engine.hip calls (engine_types.h
// declares it) and every instantiation of lookahead_kernel.
//
// What it computes (include/mi355env.h mi_lookahead): for every sub-environment i, the discounted return of K candidate action sequences of length H.
// The candidate -- its private copy of lane i, its step, its tally, the lane mapping and the loop's idiom -- is candidate_lane.h's.  This unit's own:
// the actions come from [t][j], the next step's requested one step ahead with everything else the lane reads before tables_init; lane_step's validity
// check (an action outside the space is reported through the sticky error word and leaves the candidate untouched); the observation is taken once,
// after the loop, and only when final_obs is asked for.
//
// Why a unit, why max-ILP (build.py TU_FLAGS): classic.hip's reasons -- at 65 536 lanes one wavefront runs per SIMD and hides latency with its own
// independent instructions.  Unlike the rollouts there is no trajectory traffic to overlap, so there is no second role; instead the kernels are
// bounded to half the register file (two wavefronts per SIMD beyond 65 536 lanes) which costs no instantiation a spill (kLookWaves, below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "candidate_lane.h"

namespace {

struct LookPtrs {
    const void *actions;  // [H][K * N] E::Act
    CandidateOut out;
    int H, KN;
    double gamma;
};

// wavefronts per SIMD the kernels' registers are bounded for: at most 256 registers each.  Every instantiation fits without a spill -- the widest,
// Acrobot with per-lane attributes (~20 attribute registers next to four RK4 stages), at 241; docs/results_log.md has the table.
constexpr int kLookWaves = 2;

template <class E>
__global__ __launch_bounds__(kBlock, kLookWaves) void lookahead_kernel(DevEnv d, LookPtrs io, AttrDev at) {
    typedef typename E::Act Act;
    const CandidateIndex c(d.N, io.KN);
    const int j = c.j;
    const Act *acts = static_cast<const Act *>(io.actions);
    CandidateStart<E> start;
    Act a_next = (Act)0;
    if (c.live) {
        start.request(d, at, c.i);
        a_next = acts[j];
    }
    tables_init<E>();
    if (!c.live) return;
    Lane<E> L;
    Pcg64 gen;
    CandidateTally tally(start.arrive(L, gen));
    hold_opaque(a_next);
    uint32_t bad_any = 0u;
    const size_t KN = (size_t)io.KN;
    for (int t = 0; t < io.H; t++) {
        Act a = a_next;
        const int tn = t + 1 < io.H ? t + 1 : t;
        a_next = acts[(size_t)tn * KN + j];
        // lane_step: an action outside the space is reported through the sticky error word and the lane is left untouched
        const bool bad = tally.active && !E::valid(a);
        bad_any |= bad ? 1u : 0u;
        a = bad ? (Act)0 : a;
        const bool go = tally.active && !bad;
        double rew;
        bool te;
        candidate_draw(L, gen, go);
        double s0[E::S];
#pragma unroll
        for (int k = 0; k < E::S; k++) s0[k] = L.s[k];
        uint32_t sflags = L.flags;
        E::step(L.s, sflags, a, d.P, rew, te, L.trig);
#pragma unroll
        for (int k = 0; k < E::S; k++) L.s[k] = go ? L.s[k] : s0[k];
        L.flags = go ? sflags : L.flags;
        const bool tr = candidate_time_limit(d, L, go);
        tally.take(go, rew, te, tr, io.gamma);
    }
    if (bad_any) *d.error = kErrInvalidAction;
    float o[E::OBS];
    if (io.out.final_obs) E::obs(L.s, L.flags, o, L.trig);
    tally.store<E::OBS>(io.out, j, o);
}

template <class E>
int launch_for(mi_vecenv *v, const LookPtrs &p) {
    const AttrDev at = {v->d_attr, v->attr_mask};
    hipLaunchKernelGGL((lookahead_kernel<E>), dim3(candidate_grid(p.KN)), dim3(kBlock), 0, v->stream, v->d, p, at);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace

namespace mi_lookahead_unit {
int launch(mi_vecenv *v, const void *actions, int act_kind, int horizon, int candidates, double gamma, double *returns, int32_t *steps, uint8_t *terminated,
           uint8_t *truncated, float *final_obs) {
    const LookPtrs p = {actions, {returns, steps, terminated, truncated, final_obs}, horizon, candidates * v->cfg.num_envs, gamma};
    return dispatch_candidate_env<true>(v, act_kind, "mi_lookahead", [&](auto e) { return launch_for<typename decltype(e)::type>(v, p); });
}
}  // namespace mi_lookahead_unit
