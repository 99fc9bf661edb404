// candidate_lane.h -- the candidate loop of mi_lookahead and mi_lookahead_policy: the parts lookahead_kernel (lookahead.hip) is made of, and the host
// dispatch both units launch through.  lookahead_policy_kernel keeps device text of its own (its unit's head says why).  No kernel here.
//
// What a candidate is: K candidates per sub-environment, each a PRIVATE copy of lane i -- state, elapsed steps, flags, attribute registers, generator --
// stepped with lane_step's own sequence (E::step, elapsed += 1, TimeLimit) and stopped after the first step that terminates or truncates.  The env is
// only read.  One lane per candidate, lane j = k * N + i: consecutive lanes read consecutive rows of the env's arrays (except where j wraps around N)
// and write consecutive results.
//
// The loop's idiom (lane_step_fused's: the classic kernels are issue-bound): nothing is stored inside the step loop and it has
// no data-dependent control flow of its own.  A candidate that has finished -- or never started, because its row waits for a reset -- keeps stepping
// from the state it holds; that state, its return, step count and flags are held by selects on `go`, so the state stays finite and is what final_obs
// reports.
#ifndef MI355ENV_CANDIDATE_LANE_H
#define MI355ENV_CANDIDATE_LANE_H
#include <type_traits>

#include "lane_step.h"

namespace {

// The outputs, device pointers, every one nullable; lane j writes element j.
struct CandidateOut {
    double *returns;  // [K * N]
    int32_t *steps;   // [K * N]
    uint8_t *terminated, *truncated;
    float *final_obs;  // [K * N][OBS]
};

struct CandidateIndex {
    int j0;  // the workgroup's first lane (< KN < 2^31)
    bool live;
    int j, k, i;  // lane, candidate, sub-environment
    MI_DEV CandidateIndex(int N, int KN) {
        const unsigned ju = blockIdx.x * (unsigned)kBlock + threadIdx.x;  // (the last workgroup's lanes may pass 2^31: compared as unsigned)
        j0 = (int)(blockIdx.x * (unsigned)kBlock);
        live = ju < (unsigned)KN;
        j = (int)ju;
        k = live ? j / N : 0;
        i = live ? j - k * N : 0;
    }
};

template <class E>
struct CandidateStart {
    double s[E::S];
    uint32_t meta = 0;
    uint64_t g[4] = {0, 0, 0, 0};
    AttrRequest<E> ar;
    // a live lane, before tables_init
    MI_DEV void request(const DevEnv &d, const AttrDev &at, int i) {
#pragma unroll
        for (int q = 0; q < E::S; q++) s[q] = d.state[(size_t)q * d.N + i];
        meta = d.meta[i];
        if constexpr (HasStepDraws<E>::value) {
#pragma unroll
            for (int q = 0; q < 4; q++) g[q] = d.rng[(size_t)q * d.N + i];
        }
        ar.request(at, d, i);
    }
    // after the barrier.  `gen` is the sub-environment's generator, copied: every candidate of i sees the draws the env would see next.  Returns the
    // initial `active`: a lane that waits for its reset (NEXT_STEP, DISABLED) has nothing to look ahead from and starts finished.
    MI_DEV uint32_t arrive(Lane<E> &L, [[maybe_unused]] Pcg64 &gen) {
#pragma unroll
        for (int q = 0; q < E::S; q++) hold_opaque(s[q]), L.s[q] = s[q];
        hold_opaque(meta);
        L.elapsed = meta & kElapsedMask, L.flags = meta >> kFlagShift;
        trig_invalidate(L.trig);
        ar.arrive(L.trig);
        if constexpr (HasStepDraws<E>::value) {
#pragma unroll
            for (int q = 0; q < 4; q++) hold_opaque(g[q]);
            gen.state = make_u128(g[0], g[1]), gen.inc = make_u128(g[2], g[3]);
        }
        return (L.flags & kNeedsReset) ? 0u : 1u;
    }
};

// The pieces around one private step.  The step itself -- keep the state, E::step, select state and flags by `go` -- stays written out in the kernel:
// the select behind a function of this header cost lookahead_kernel<MountainCarContinuousT<.., ActF64>> two registers (docs/results_log.md).
// The draw of a type whose step draws (a lane that goes takes it before the dynamics, lane_step's order):
template <class E>
MI_DEV void candidate_draw(Lane<E> &L, [[maybe_unused]] Pcg64 &gen, [[maybe_unused]] bool go) {
    if constexpr (HasStepDraws<E>::value) {
        if (go && E::step_draws(L.trig)) E::step_drawn(L.trig, gen.next_double());
    }
}
// TimeLimit.step (wrappers/common.py:129-133) on the candidate's own count
template <class E>
MI_DEV bool candidate_time_limit(const DevEnv &d, Lane<E> &L, bool go) {
    const uint32_t elapsed = L.elapsed + 1u;
    const bool tr = d.max_steps > 0 && (int)elapsed >= d.max_steps;
    L.elapsed = go ? elapsed : L.elapsed;
    return tr;
}

// What a candidate has gathered (integers, not bools, for what lives across the loop: ResetQueue::have's reason).
struct CandidateTally {
    uint32_t active, te_last = 0u, tr_last = 0u;
    int32_t steps = 0;
    double G = 0.0, disc = 1.0;
    MI_DEV explicit CandidateTally(uint32_t active_) : active(active_) {}
    MI_DEV void take(bool go, double rew, bool te, bool tr, double gamma) {
        const double term = disc * rew;  // (rounded before the sum: -ffp-contract=off)
        G = go ? G + term : G;
        disc = go ? disc * gamma : disc;
        steps += go ? 1 : 0;
        te_last = go ? (te ? 1u : 0u) : te_last;
        tr_last = go ? (tr ? 1u : 0u) : tr_last;
        active = (go && (te || tr)) ? 0u : active;
    }
    // `o`: the OBS floats of the observation of the state the lane holds; read only when final_obs is asked for
    template <int OBS>
    MI_DEV void store(const CandidateOut &out, int j, const float *o) const {
        if (out.returns) out.returns[j] = G;
        if (out.steps) out.steps[j] = steps;
        if (out.terminated) out.terminated[j] = (uint8_t)te_last;
        if (out.truncated) out.truncated[j] = (uint8_t)tr_last;
        if (out.final_obs) store_row<OBS>(out.final_obs + (size_t)j * OBS, o);
    }
};

// ---- host: the env's kind to the exact env type (classic.hip dispatch_kind_act_math / dispatch_kind_attr) -------------------------------------------
template <class E>
struct EnvType {
    typedef E type;
};
// f(EnvType<E>{}) for the type of `kind`: the per-lane types with `attr`; with F64_ROWS -- the caller's compile-time choice, so that a unit without
// float64 action rows instantiates nothing for them -- the float64 variants of the Box kinds by `act_kind`.  false: not a classic-control kind.
template <bool F64_ROWS, bool ATTR, class F>
bool for_candidate_env_of(int kind, [[maybe_unused]] int act_kind, F &&f) {
    typedef ExactMath M;
    typedef ExactMathBuiltinFma MA;  // (the math policy of Acrobot's other kernels, envs_classic.h)
    switch (kind) {
    case MI_ENV_CARTPOLE: f(EnvType<std::conditional_t<ATTR, CartPoleAttrT<M>, CartPoleT<M>>>{}); return true;
    case MI_ENV_PENDULUM:
        if constexpr (F64_ROWS) {
            if (act_kind != MI_F32) return f(EnvType<std::conditional_t<ATTR, PendulumAttrT<M, ActF64>, PendulumT<M, ActF64>>>{}), true;
        }
        f(EnvType<std::conditional_t<ATTR, PendulumAttrT<M>, PendulumT<M>>>{});
        return true;
    case MI_ENV_ACROBOT: f(EnvType<std::conditional_t<ATTR, AcrobotAttrT<MA>, AcrobotT<MA>>>{}); return true;
    case MI_ENV_MOUNTAIN_CAR: f(EnvType<std::conditional_t<ATTR, MountainCarAttrT<M>, MountainCarT<M>>>{}); return true;
    case MI_ENV_MOUNTAIN_CAR_CONTINUOUS:
        if constexpr (F64_ROWS) {
            if (act_kind == MI_F64) return f(EnvType<std::conditional_t<ATTR, MountainCarContinuousAttrT<M, ActF64>, MountainCarContinuousT<M, ActF64>>>{}), true;
            if (act_kind == MI_F64_WEAK)
                return f(EnvType<std::conditional_t<ATTR, MountainCarContinuousAttrT<M, ActF64Weak>, MountainCarContinuousT<M, ActF64Weak>>>{}), true;
        }
        f(EnvType<std::conditional_t<ATTR, MountainCarContinuousAttrT<M>, MountainCarContinuousT<M>>>{});
        return true;
    }
    return false;
}
template <bool F64_ROWS, class F>
bool for_candidate_env(int kind, bool attr, int act_kind, F &&f) {
    return attr ? for_candidate_env_of<F64_ROWS, true>(kind, act_kind, f) : for_candidate_env_of<F64_ROWS, false>(kind, act_kind, f);
}
// ... for an env: `launch(EnvType<E>{})` returns the status.  `who` is the entry point's name, for the message.
template <bool F64_ROWS, class F>
int dispatch_candidate_env(const mi_vecenv *v, int act_kind, const char *who, F &&launch) {
    int rc = MI_OK;
    // an env on the per-lane types (mi_set_env_attr; once mi_set_step_wrappers was on) stays on them, as in mi_classic::step
    if (!for_candidate_env<F64_ROWS>(v->cfg.kind, v->attr_mask || v->per_lane, act_kind, [&](auto e) { rc = launch(e); }))
        return fail(MI_ERR_UNSUPPORTED, "%s: the five classic-control kinds only", who);
    return rc;
}
inline unsigned candidate_grid(int KN) { return (unsigned)(((int64_t)KN + kBlock - 1) / kBlock); }

}  // namespace
#endif
