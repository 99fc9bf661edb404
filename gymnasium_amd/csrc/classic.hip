// classic.hip -- the classic-control kernels as their own translation unit: namespace mi_classic, the launch functions engine.hip calls for the kinds
// CARTPOLE ... MOUNTAIN_CAR_CONTINUOUS (engine_types.h declares them), and every instantiation of the kernels of classic_kernels.h.
//
// Why a unit, why max-ILP (build.py TU_FLAGS): these kernels run ONE wavefront per SIMD at the benchmark's 65 536 sub-environments, where nothing
// hides a dependent instruction's latency but the wavefront's own independent instructions: max-ILP scheduling
// measured +6.4 % (CartPole), +5.8 % (Pendulum), +2.7 % (MountainCarContinuous) against the default max-occupancy scheduler, with every result bit
// unchanged (scheduling reorders, it does not re-associate; tests/test_gpu_parity.py compares array_equal) -- and -1 ... -2 % on the ToyText and
// one-lane MuJoCo kernels, which therefore stay on the default scheduler (tabular.hip, mujoco.hip) (profiles/r04_maxilp_classic.txt).
//
// Here: the dispatchers from the env's kind to its type (envs_classic.h), the host ends of the step epilogue, the launch_step* / launch_rollout*
// templates and namespace mi_classic.  No MuJoCo or ToyText code, and no part of the C ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "classic_kernels.h"

namespace {

template <class M>
struct AcrobotMath {
    typedef M type;
};
template <>
struct AcrobotMath<ExactMath> {
    typedef ExactMathBuiltinFma type;
};
template <class M, class F>
int dispatch_kind_math(int kind, F &&f) {
    switch (kind) {
    case MI_ENV_CARTPOLE: return f(CartPoleT<M>());
    case MI_ENV_PENDULUM: return f(PendulumT<M>());
    case MI_ENV_ACROBOT: return f(AcrobotT<typename AcrobotMath<M>::type>());  // (exact math: without the inline-asm Horner steps, envs_classic.h)
    case MI_ENV_MOUNTAIN_CAR: return f(MountainCarT<M>());
    case MI_ENV_MOUNTAIN_CAR_CONTINUOUS: return f(MountainCarContinuousT<M>());
    }
    return fail(MI_ERR_INVALID_ARGUMENT, "unknown env kind");
}
// fast_math: MI_CFG_FAST_MATH (envs_classic.h FastMath); the default is the reference's libm bit for bit
template <class F>
int dispatch_kind(int kind, bool fast_math, F &&f) {
    return fast_math ? dispatch_kind_math<FastMath>(kind, f) : dispatch_kind_math<ExactMath>(kind, f);
}
// ... and the kind of the action rows (mi_step_io.actions_dtype): the two Box kinds have float64 instantiations (envs_classic.h ActF64 / ActF64Weak)
template <class M, class F>
int dispatch_kind_act_math(int kind, int act_kind, F &&f) {
    if (act_kind != MI_F32) {
        if (kind == MI_ENV_PENDULUM) return f(PendulumT<M, ActF64>());  // (a Python float and an np.float64 behave alike there)
        if (kind == MI_ENV_MOUNTAIN_CAR_CONTINUOUS) return act_kind == MI_F64_WEAK ? f(MountainCarContinuousT<M, ActF64Weak>()) : f(MountainCarContinuousT<M, ActF64>());
    }
    return dispatch_kind_math<M>(kind, f);
}
template <class F>
int dispatch_kind_act(int kind, bool fast_math, int act_kind, F &&f) {
    return fast_math ? dispatch_kind_act_math<FastMath>(kind, act_kind, f) : dispatch_kind_act_math<ExactMath>(kind, act_kind, f);
}
// per-lane attributes (mi_set_env_attr has refused fast math and the shared generator)
template <class F>
int dispatch_kind_attr(int kind, int act_kind, F &&f) {
    switch (kind) {
    case MI_ENV_CARTPOLE: return f(CartPoleAttrT<ExactMath>());
    case MI_ENV_PENDULUM: return act_kind != MI_F32 ? f(PendulumAttrT<ExactMath, ActF64>()) : f(PendulumAttrT<ExactMath>());
    case MI_ENV_ACROBOT: return f(AcrobotAttrT<ExactMathBuiltinFma>());  // (the math policy of Acrobot's other kernels, envs_classic.h)
    case MI_ENV_MOUNTAIN_CAR: return f(MountainCarAttrT<ExactMath>());
    case MI_ENV_MOUNTAIN_CAR_CONTINUOUS:
        if (act_kind == MI_F64) return f(MountainCarContinuousAttrT<ExactMath, ActF64>());
        if (act_kind == MI_F64_WEAK) return f(MountainCarContinuousAttrT<ExactMath, ActF64Weak>());
        return f(MountainCarContinuousAttrT<ExactMath>());
    }
    return fail(MI_ERR_UNSUPPORTED, "per-sub-environment attributes: not for this kind");
}

// the statistics handles' current buffer sets into the device view (they swap after every step that updated them)
void epilogue_bind(mi_vecenv *v) {
    EpiDev &d = v->epi;
    if (const mi_running_stats *o = v->epi_host.obs_rms)
        d.obs_mean = o->mean, d.obs_var = o->var, d.obs_count = o->count, d.obs_mean2 = o->mean2, d.obs_var2 = o->var2, d.obs_count2 = o->count2;
    if (const mi_running_stats *r = v->epi_host.return_rms)
        d.ret_mean = r->mean, d.ret_var = r->var, d.ret_count = r->count, d.ret_mean2 = r->mean2, d.ret_var2 = r->var2, d.ret_count2 = r->count2;
}
void epilogue_swap(mi_vecenv *v) {
    auto swap = [](mi_running_stats *s) {
        double *t;
        t = s->mean, s->mean = s->mean2, s->mean2 = t;
        t = s->var, s->var = s->var2, s->var2 = t;
        t = s->count, s->count = s->count2, s->count2 = t;
    };
    if (v->epi.obs_on && v->epi.obs_update) swap(v->epi_host.obs_rms);
    if (v->epi.ret_on && v->epi.ret_update) swap(v->epi_host.return_rms);
}

template <class E, bool EPI, bool SAMPLE = false>
void launch_step_mode(mi_vecenv *v, const StepPtrs &p) {
    const dim3 g(v->grid), b(kBlock);
    const AttrDev at = {v->d_attr, v->attr_mask};
    switch (v->cfg.autoreset_mode) {
    case MI_AUTORESET_NEXT_STEP: hipLaunchKernelGGL((step_kernel<E, MI_AUTORESET_NEXT_STEP, EPI, SAMPLE>), g, b, 0, v->stream, v->d, p, v->epi, at); break;
    case MI_AUTORESET_SAME_STEP: hipLaunchKernelGGL((step_kernel<E, MI_AUTORESET_SAME_STEP, EPI, SAMPLE>), g, b, 0, v->stream, v->d, p, v->epi, at); break;
    default: hipLaunchKernelGGL((step_kernel<E, MI_AUTORESET_DISABLED, EPI, SAMPLE>), g, b, 0, v->stream, v->d, p, v->epi, at); break;
    }
}
// the wrapped kernels' last argument; MAXSKIP (mi_set_max_and_skip): RepeatAction is off (the two refuse each other) and its loop runs `skip` trips
template <bool MAXSKIP>
WrapArg<MAXSKIP> wrap_arg(const mi_vecenv *v) {
    WrapArg<MAXSKIP> w = v->wrap;
    if constexpr (MAXSKIP) w.repeats = w.skip;
    return w;
}
template <class E, bool SAMPLE, bool MAXSKIP = false>
void launch_step_wrapped_mode(mi_vecenv *v, const StepPtrs &p) {
    const dim3 g(v->grid), b(kBlock);
    const AttrDev at = {v->d_attr, v->attr_mask};
    const WrapArg<MAXSKIP> w = wrap_arg<MAXSKIP>(v);
    switch (v->cfg.autoreset_mode) {
    case MI_AUTORESET_NEXT_STEP: hipLaunchKernelGGL((step_wrapped_kernel<E, MI_AUTORESET_NEXT_STEP, SAMPLE, MAXSKIP>), g, b, 0, v->stream, v->d, p, at, w); break;
    case MI_AUTORESET_SAME_STEP: hipLaunchKernelGGL((step_wrapped_kernel<E, MI_AUTORESET_SAME_STEP, SAMPLE, MAXSKIP>), g, b, 0, v->stream, v->d, p, at, w); break;
    default: hipLaunchKernelGGL((step_wrapped_kernel<E, MI_AUTORESET_DISABLED, SAMPLE, MAXSKIP>), g, b, 0, v->stream, v->d, p, at, w); break;
    }
}
// (mi_set_max_and_skip: the MAXSKIP instantiations, chosen on the host)
template <class E, bool SAMPLE>
void launch_step_wrapped_form(mi_vecenv *v, const StepPtrs &p) {
    if (v->wrap.skip)
        launch_step_wrapped_mode<E, SAMPLE, true>(v, p);
    else
        launch_step_wrapped_mode<E, SAMPLE>(v, p);
}
template <class E>
int launch_step(mi_vecenv *v, const StepPtrs &p) {
    if (v->wrap_on) {  // (mi_set_step_wrappers and mi_set_step_epilogue refuse each other; the env is on the per-lane types: the others have no such kernels)
        if constexpr (!HasAttrs<E>::value) {
            return fail(MI_ERR_STATE, "mi_set_step_wrappers: the wrapped kernels exist for the per-lane types");
        } else if constexpr (E::ACT_KIND == MI_F32 || E::ACT_KIND == MI_I64) {
            if (p.act_lane)
                launch_step_wrapped_form<E, true>(v, p);
            else
                launch_step_wrapped_form<E, false>(v, p);
        } else {
            launch_step_wrapped_form<E, false>(v, p);
        }
    } else if (!v->has_epi) {
        // the on-device policy draws the space's own dtype (float32 rows / int64): the float64-row instantiations never sample (the caller, step_enqueue,
        // sends a wrapped step that samples through the stand-alone sampler + this kernel with p.actions set instead)
        if constexpr (E::ACT_KIND == MI_F32 || E::ACT_KIND == MI_I64) {
            if (p.act_lane)
                launch_step_mode<E, false, true>(v, p);
            else
                launch_step_mode<E, false>(v, p);
        } else {
            launch_step_mode<E, false>(v, p);
        }
    } else {
        if (!p.obs || !p.reward || !p.terminated || !p.truncated) return fail(MI_ERR_INVALID_ARGUMENT, "a step with an epilogue needs obs, reward, terminated and truncated");
        epilogue_bind(v);
        launch_step_mode<E, true>(v, p);
        const EpiDev &e = v->epi;
        if (e.obs_on || e.ret_on) {
            if (!e.fold_in_finish && epi_reduces(e)) hipLaunchKernelGGL((epilogue_combine<E::OBS>), dim3(1), dim3(kBlock), 0, v->stream, e, v->d.N);
            hipLaunchKernelGGL((epilogue_finish<E::OBS>), dim3(v->grid), dim3(kBlock), 0, v->stream, e, v->d.N, p.obs, p.reward, p.terminated, p.truncated);
            epilogue_swap(v);
        }
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// mi_rollout / mi_rollout_infos with mi_set_step_wrappers (MAXSKIP: mi_set_max_and_skip) on: one kernel stores whatever is asked for
template <class E, bool MAXSKIP>
int launch_rollout_wrapped_form(mi_vecenv *v, const RolloutPtrs &p, const RolloutExtra &ex, const ActionStream &as, int T, bool sample) {
    const bool next_step = v->cfg.autoreset_mode == MI_AUTORESET_NEXT_STEP;
    const AttrDev at = {v->d_attr, v->attr_mask};
    const dim3 g(v->grid), b(kBlock);
    const WrapArg<MAXSKIP> w = wrap_arg<MAXSKIP>(v);
    constexpr bool F64 = E::ACT_KIND == MI_F64 || E::ACT_KIND == MI_F64_WEAK;  // float64 action rows are always the caller's (the sampler draws float32)
    if (F64 && sample) return fail(MI_ERR_INVALID_ARGUMENT, "the on-device policy samples float32 actions");
    if constexpr (!HasAttrs<E>::value) {  // (the env is on the per-lane types once the wrappers were on: the others have no such kernels)
        return fail(MI_ERR_STATE, "mi_set_step_wrappers: the wrapped kernels exist for the per-lane types");
    } else {
    if constexpr (!F64) {
        if (sample && next_step) hipLaunchKernelGGL((rollout_wrapped_kernel<E, MI_AUTORESET_NEXT_STEP, true, MAXSKIP>), g, b, 0, v->stream, v->d, p, as, T, at, ex, w);
        if (sample && !next_step) hipLaunchKernelGGL((rollout_wrapped_kernel<E, MI_AUTORESET_SAME_STEP, true, MAXSKIP>), g, b, 0, v->stream, v->d, p, as, T, at, ex, w);
    }
    if (!sample && next_step) hipLaunchKernelGGL((rollout_wrapped_kernel<E, MI_AUTORESET_NEXT_STEP, false, MAXSKIP>), g, b, 0, v->stream, v->d, p, as, T, at, ex, w);
    if (!sample && !next_step) hipLaunchKernelGGL((rollout_wrapped_kernel<E, MI_AUTORESET_SAME_STEP, false, MAXSKIP>), g, b, 0, v->stream, v->d, p, as, T, at, ex, w);
    HIP_TRY(hipGetLastError());
    return MI_OK;
    }
}

template <class E>
int launch_rollout_wrapped(mi_vecenv *v, const RolloutPtrs &p, const RolloutExtra &ex, const ActionStream &as, int T, bool sample) {
    if (v->wrap.skip) return launch_rollout_wrapped_form<E, true>(v, p, ex, as, T, sample);
    return launch_rollout_wrapped_form<E, false>(v, p, ex, as, T, sample);
}

template <class E, int MODE, bool SAMPLE, bool FULL>
void launch_rollout_variant(mi_vecenv *v, const RolloutPtrs &p, const ActionStream &as, int T) {
    const AttrDev at = {v->d_attr, v->attr_mask};
    hipLaunchKernelGGL((rollout_kernel<E, MODE, SAMPLE, FULL>), dim3(v->grid), dim3(kBlock), 0, v->stream, v->d, p, as, T, at);
}

template <class E>
int launch_rollout(mi_vecenv *v, const RolloutPtrs &p, const ActionStream &as, int T, bool sample) {
    const bool next_step = v->cfg.autoreset_mode == MI_AUTORESET_NEXT_STEP;
    const bool full = p.obs && p.reward && p.terminated && p.truncated && (!sample || p.actions_out);
    if (v->wrap_on) return launch_rollout_wrapped<E>(v, p, RolloutExtra{}, as, T, sample);
    if constexpr (E::ACT_KIND == MI_F64 || E::ACT_KIND == MI_F64_WEAK) {  // float64 action rows are always the caller's (the sampler draws float32)
        if (sample) return fail(MI_ERR_INVALID_ARGUMENT, "the on-device policy samples float32 actions");
        if (next_step)
            launch_rollout_variant<E, MI_AUTORESET_NEXT_STEP, false, false>(v, p, as, T);
        else
            launch_rollout_variant<E, MI_AUTORESET_SAME_STEP, false, false>(v, p, as, T);
    } else if (next_step && sample && full) {  // the collector's configuration (bench.py)
        bool duo = false;
        if constexpr (E::DUO_ROLLOUT) {
            const char *env = getenv("MI355ENV_ROLLOUT_DUO");  // "0": the one-role kernel (A/B: scripts/r04/duo_ab_bench.sh)
            duo = !(env && env[0] == '0') && T % DuoTraits<E>::CHUNK == 0;
            if (duo) hipLaunchKernelGGL((rollout_duo_kernel<E>), dim3(v->grid), dim3(kDuoBlock), 0, v->stream, v->d, p, as, T);
        }
        if (!duo) launch_rollout_variant<E, MI_AUTORESET_NEXT_STEP, true, true>(v, p, as, T);
    }
    else if (next_step && sample)
        launch_rollout_variant<E, MI_AUTORESET_NEXT_STEP, true, false>(v, p, as, T);
    else if (next_step)
        launch_rollout_variant<E, MI_AUTORESET_NEXT_STEP, false, false>(v, p, as, T);
    else if (sample)
        launch_rollout_variant<E, MI_AUTORESET_SAME_STEP, true, false>(v, p, as, T);
    else
        launch_rollout_variant<E, MI_AUTORESET_SAME_STEP, false, false>(v, p, as, T);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

template <class E>
int launch_rollout_infos(mi_vecenv *v, const RolloutPtrs &p, const RolloutExtra &ex, const ActionStream &as, int T, bool sample) {
    const bool next_step = v->cfg.autoreset_mode == MI_AUTORESET_NEXT_STEP;
    const AttrDev at = {v->d_attr, v->attr_mask};
    const dim3 g(v->grid), b(kBlock);
    if (v->wrap_on) return launch_rollout_wrapped<E>(v, p, ex, as, T, sample);
    if constexpr (E::ACT_KIND == MI_F64 || E::ACT_KIND == MI_F64_WEAK) {
        if (sample) return fail(MI_ERR_INVALID_ARGUMENT, "the on-device policy samples float32 actions");
        if (next_step)
            hipLaunchKernelGGL((rollout_infos_kernel<E, MI_AUTORESET_NEXT_STEP, false>), g, b, 0, v->stream, v->d, p, as, T, at, ex);
        else
            hipLaunchKernelGGL((rollout_infos_kernel<E, MI_AUTORESET_SAME_STEP, false>), g, b, 0, v->stream, v->d, p, as, T, at, ex);
    } else if (next_step && sample)
        hipLaunchKernelGGL((rollout_infos_kernel<E, MI_AUTORESET_NEXT_STEP, true>), g, b, 0, v->stream, v->d, p, as, T, at, ex);
    else if (next_step)
        hipLaunchKernelGGL((rollout_infos_kernel<E, MI_AUTORESET_NEXT_STEP, false>), g, b, 0, v->stream, v->d, p, as, T, at, ex);
    else if (sample)
        hipLaunchKernelGGL((rollout_infos_kernel<E, MI_AUTORESET_SAME_STEP, true>), g, b, 0, v->stream, v->d, p, as, T, at, ex);
    else
        hipLaunchKernelGGL((rollout_infos_kernel<E, MI_AUTORESET_SAME_STEP, false>), g, b, 0, v->stream, v->d, p, as, T, at, ex);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace

// ---- the launchers the other translation unit calls (this unit is compiled with the max-ILP scheduler, see the head of the file) ----------------
namespace mi_classic {
int step(mi_vecenv *v, const StepPtrs &p, int act_kind) {
    if (v->attr_mask || v->per_lane) return dispatch_kind_attr(v->cfg.kind, act_kind, [&](auto env) -> int { return launch_step<decltype(env)>(v, p); });
    return dispatch_kind_act(v->cfg.kind, (v->cfg.reserved[0] & MI_CFG_FAST_MATH) != 0, act_kind, [&](auto env) -> int { return launch_step<decltype(env)>(v, p); });
}
int reset(mi_vecenv *v, const uint8_t *dm, int has_bounds, double b0, double b1, float *dobs) {
    return dispatch_kind(v->cfg.kind, (v->cfg.reserved[0] & MI_CFG_FAST_MATH) != 0, [&](auto env) -> int {
        using E = decltype(env);
        hipLaunchKernelGGL((reset_kernel<E>), dim3(v->grid), dim3(kBlock), 0, v->stream, v->d, dm, has_bounds, b0, b1, dobs);
        HIP_TRY(hipGetLastError());
        return (int)MI_OK;
    });
}
int rollout(mi_vecenv *v, const RolloutPtrs &p, const ActionStream &as, int T, bool sample, int in_kind) {
    if (v->attr_mask || v->per_lane) return dispatch_kind_attr(v->cfg.kind, in_kind, [&](auto env) -> int { return launch_rollout<decltype(env)>(v, p, as, T, sample); });
    return dispatch_kind_act(v->cfg.kind, (v->cfg.reserved[0] & MI_CFG_FAST_MATH) != 0, in_kind, [&](auto env) -> int { return launch_rollout<decltype(env)>(v, p, as, T, sample); });
}
int rollout_infos(mi_vecenv *v, const RolloutPtrs &p, const RolloutExtra &ex, const ActionStream &as, int T, bool sample, int in_kind) {
    if (v->attr_mask || v->per_lane) return dispatch_kind_attr(v->cfg.kind, in_kind, [&](auto env) -> int { return launch_rollout_infos<decltype(env)>(v, p, ex, as, T, sample); });
    return dispatch_kind_act(v->cfg.kind, (v->cfg.reserved[0] & MI_CFG_FAST_MATH) != 0, in_kind, [&](auto env) -> int { return launch_rollout_infos<decltype(env)>(v, p, ex, as, T, sample); });
}
// ---- MI_CFG_SHARED_RNG: MI_ENV_CARTPOLE only (mi_create refuses the bit for every other kind) ---------------------------------------------
template <class F>
static int dispatch_shared(mi_vecenv *v, F &&f) {
    if (v->cfg.reserved[0] & MI_CFG_FAST_MATH) return f(CartPoleT<FastMath>());
    return f(CartPoleT<ExactMath>());
}
int shared_reset(mi_vecenv *v, float *dobs) {
    hipLaunchKernelGGL(shared_scan_kernel, dim3(1), dim3(kBlock), 0, v->stream, v->shared, v->grid, (uint64_t)4 * (uint64_t)v->cfg.num_envs);
    return dispatch_shared(v, [&](auto env) -> int {
        hipLaunchKernelGGL((shared_reset_kernel<decltype(env)>), dim3(v->grid), dim3(kBlock), 0, v->stream, v->d, v->shared, dobs);
        HIP_TRY(hipGetLastError());
        return (int)MI_OK;
    });
}
int shared_step(mi_vecenv *v, const StepPtrs &p) {
    dispatch_shared(v, [&](auto env) -> int {
        using E = decltype(env);
        hipLaunchKernelGGL((shared_validate_kernel<E>), dim3(v->grid), dim3(kBlock), 0, v->stream, v->d, static_cast<const typename E::Act *>(p.actions), v->shared);
        return (int)MI_OK;
    });
    hipLaunchKernelGGL(shared_scan_kernel, dim3(1), dim3(kBlock), 0, v->stream, v->shared, v->grid, (uint64_t)0);
    return dispatch_shared(v, [&](auto env) -> int {
        hipLaunchKernelGGL((shared_step_kernel<decltype(env)>), dim3(v->grid), dim3(kBlock), 0, v->stream, v->d, p, v->shared);
        HIP_TRY(hipGetLastError());
        return (int)MI_OK;
    });
}
int shared_rollout(mi_vecenv *v, const RolloutPtrs &p, const ActionStream &as, int T, bool sample, const RolloutExtra *ex) {
    const size_t N = (size_t)v->cfg.num_envs;
    for (int t = 0; t < T; t++) {
        StepPtrs sp;
        memset(&sp, 0, sizeof sp);
        if (sample) {
            int64_t *dst = p.actions_out ? static_cast<int64_t *>(p.actions_out) + (size_t)t * N : static_cast<int64_t *>(v->d_actions);
            const int rc = dispatch_shared(v, [&](auto env) -> int {
                hipLaunchKernelGGL((shared_sample_kernel<decltype(env)>), dim3(v->grid), dim3(kBlock), 0, v->stream, v->d, as, t, dst);
                return (int)MI_OK;
            });
            if (rc) return rc;
            sp.actions = dst;
        } else {
            sp.actions = static_cast<const int64_t *>(p.actions_in) + (size_t)t * N;
        }
        sp.obs = p.obs ? static_cast<float *>(p.obs) + (size_t)t * N * CartPole::OBS : nullptr;
        sp.reward = p.reward ? p.reward + (size_t)t * N : nullptr;
        sp.terminated = p.terminated ? p.terminated + (size_t)t * N : nullptr;
        sp.truncated = p.truncated ? p.truncated + (size_t)t * N : nullptr;
        if (ex) {  // (the step kernel writes every row of the two: 0 where no episode ended)
            sp.ep_ret = ex->ep_ret ? ex->ep_ret + (size_t)t * N : nullptr;
            sp.ep_len = ex->ep_len ? ex->ep_len + (size_t)t * N : nullptr;
        }
        if (const int rc = shared_step(v, sp)) return rc;
    }
    return MI_OK;
}
int shared_recount(mi_vecenv *v) {
    hipLaunchKernelGGL(shared_count_kernel, dim3(v->grid), dim3(kBlock), 0, v->stream, v->d, v->shared);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
}  // namespace mi_classic
