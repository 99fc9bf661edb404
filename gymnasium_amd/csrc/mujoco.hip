// mujoco.hip -- the MuJoCo family over the stock models as its own translation unit: namespace mi_mujoco, the functions engine.hip calls for the eleven
// MuJoCo kinds once the arguments are validated and the buffers chosen (engine_types.h declares them), and every instantiation of the kernels of
// mj_glue_kernels.h / mj_wrapped_kernels.h over the compiled-in models.
//
// Why a unit, why the default flag set: these kernels were four fifths of engine.o's device code and take minutes to compile; here they compile beside
// the C ABI's host code instead of with every change to it.  They stay on the default scheduler, as in engine.o: under iterative-maxocc the one-lane
// Humanoid kernel diverged (build.py TU_FLAGS), under max-ILP Hopper lost 2 % (profiles/r04_maxilp_classic.txt).
//
// Here: the stock one-lane kernels through MjLaneLaunch (mj_lane_launch.h), as mjx_model.hip and mjx_mass_model.hip launch theirs; the one place that
// chooses between the three (lane_launchers); what only the cooperative robots add -- the physics launch (mi_phys, physics16.hip / physics32.hip), its
// glue instantiations and the per-step sampler; and what engine.hip's host side needs to know about a robot.  No ToyText, classic-control or ABI code.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "mj_lane_launch.h"
#include "mjx_physics.h"

namespace {

template <class M>
using StockModel = M;  // the compiled-in model itself: MjLaneLaunch's env types are then mjx::MjEnv<mjx::AntModel, mjx::kAnt> ...
typedef MjLaneLaunch<StockModel> Stock;

// The one-lane kernels an env runs: over the stock models, or over its per-sub-environment model fields (mi_set_model_field: mjx_model.hip), or those
// with the mass rows in their view while a body mass scale is held (mjx_mass_model.hip).  An env that never set a scale keeps the stock reset kernel.
struct LaneLaunchers {
    decltype(&Stock::step) step;
    decltype(&Stock::step_wrapped) step_wrapped;
    decltype(&Stock::rollout) rollout;
    decltype(&Stock::reset) reset;
};
const LaneLaunchers &lane_launchers(const mi_vecenv *v) {
    static const LaneLaunchers stock = {Stock::step, Stock::step_wrapped, Stock::rollout, Stock::reset};
    static const LaneLaunchers model = {mi_mjmodel::step, mi_mjmodel::step_wrapped, mi_mjmodel::rollout, Stock::reset};
    static const LaneLaunchers mass = {mi_mjmass::step, mi_mjmass::step_wrapped, mi_mjmass::rollout, mi_mjmass::reset};
    if (!v->d_model) return stock;
    return (v->model_mask & (1u << MI_MODEL_BODY_MASS_SCALE)) ? mass : model;
}
const char kNoLaneKernel[] = "no one-lane kernel for this MuJoCo kind";
// the cooperative physics runs: the robot has it, it is the faster one or forced (configure), and the env reads the compiled-in model
bool runs_coop(const mi_vecenv *v) { return v->mj_coop && !v->d_model; }

// f(env type) for a robot with a cooperative physics kernel (E::HAS_COOP; configure sets mj_coop for no other)
template <class F>
int dispatch_coop(int kind, F &&f) {
    bool held = false;
    int rc = MI_OK;
    Stock::dispatch(kind, [&](auto env) {
        if constexpr (decltype(env)::HAS_COOP) held = true, rc = f(env);
    });
    return held ? rc : fail(MI_ERR_UNSUPPORTED, "no cooperative physics kernel for this env kind");
}
// mj_physics_kernel for the rows whose `meta` word has none of `skip_mask` set (or for every row: !skip_resetting); leaves the glue's extras in d_extras
template <class E>
int launch_physics(mi_vecenv *v, const uint32_t *meta, uint32_t skip_mask, bool skip_resetting, const MjStepPtrs &mp) {
    mi_phys::Args pa;
    pa.state = v->d.state, pa.meta = meta, pa.needs_reset_mask = skip_mask, pa.N = v->d.N, pa.frame_skip = (int)v->d.P.p[4];
    pa.newton = v->d.solver_newton, pa.act_f64 = mp.act_f64;
    const bool ok = E::COOP_G == 16 ? mi_phys::launch16(v->cfg.kind, pa, skip_resetting, mp.actions, v->d_extras, v->stream)
                                    : mi_phys::launch32(v->cfg.kind, pa, skip_resetting, mp.actions, v->d_extras, v->stream);
    return ok ? (int)MI_OK : fail(MI_ERR_UNSUPPORTED, "no cooperative physics kernel for this env kind");
}

// One vector step of a MuJoCo env with RepeatAction / StickyAction on (mi_set_step_wrappers; mj_wrapped_kernels.h): the opening kernel, then per trip
// what the plain step launches -- [cooperative physics ->] glue, the wrapped instantiation -- all on the env's stream, nothing synchronised.  The physics
// launch of a trip takes the inner-step words as its meta (their skip bit as the mask: rows that finished inside the repeat, or that reset instead of
// stepping, retire) and the effective action rows as its actions.
int launch_mj_step_wrapped(mi_vecenv *v, MjStepPtrs mp) {
    const dim3 g(v->grid), b(kBlock);
    const int kind = v->cfg.kind, mode = v->cfg.autoreset_mode;
    const MjWrapDev w = {v->wrap.repeats, v->wrap.sticky_duration, v->wrap.sticky_p, v->wrap.last_action, v->wrap.sticky_word, v->d_wrap_acc, v->d_wrap_inner};
    hipLaunchKernelGGL(mj_wrap_open_kernel, g, b, 0, v->stream, v->d, w, mp.actions, v->lay.act_dim, mp.act_f64, mode);
    if (w.sticky_duration) mp.actions = w.last_action;
    const bool coop = runs_coop(v);
    mp.extras = coop ? v->d_extras : nullptr;
    const int trips = w.repeats > 0 ? w.repeats : 1;
    for (int trip = 0; trip < trips; trip++) {
        if (!coop) {
            if (!lane_launchers(v).step_wrapped(kind, mode, trip, v->grid, v->stream, v->d, &mp, w)) return fail(MI_ERR_UNSUPPORTED, kNoLaneKernel);
            continue;
        }
        const int rc = dispatch_coop(kind, [&](auto env) -> int {
            using E = decltype(env);
            if (const int rc = launch_physics<E>(v, w.inner, kMjInnerSkip, true, mp)) return rc;
            hipLaunchKernelGGL((mj_trip_kernel<E, true>), g, b, 0, v->stream, v->d, mp, w, mode, trip);
            return MI_OK;
        });
        if (rc) return rc;
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// One vector step of a MuJoCo env: [cooperative physics ->] per-lane glue (autoreset state machine, reward, observation, stats)
int launch_mj_step(mi_vecenv *v, MjStepPtrs mp) {
    if (v->wrap_on) return launch_mj_step_wrapped(v, mp);
    const int kind = v->cfg.kind, mode = v->cfg.autoreset_mode;
    mp.extras = nullptr;
    if (!runs_coop(v)) {  // the one-lane simulator inside the step kernel
        if (!lane_launchers(v).step(kind, mode, v->grid, v->stream, v->d, &mp)) return fail(MI_ERR_UNSUPPORTED, kNoLaneKernel);
        HIP_TRY(hipGetLastError());
        return MI_OK;
    }
    const int rc = dispatch_coop(kind, [&](auto env) -> int {
        using E = decltype(env);
        const dim3 g(v->grid), b(kBlock);
        if (const int rc = launch_physics<E>(v, v->d.meta, kNeedsReset << kFlagShift, mode != MI_AUTORESET_SAME_STEP, mp)) return rc;  // (SAME_STEP: every row steps)
        mp.extras = v->d_extras;
        switch (mode) {
        case MI_AUTORESET_NEXT_STEP: hipLaunchKernelGGL((mj_step_kernel<E, MI_AUTORESET_NEXT_STEP, true>), g, b, 0, v->stream, v->d, mp); break;
        case MI_AUTORESET_SAME_STEP: hipLaunchKernelGGL((mj_step_kernel<E, MI_AUTORESET_SAME_STEP, true>), g, b, 0, v->stream, v->d, mp); break;
        default: hipLaunchKernelGGL((mj_step_kernel<E, MI_AUTORESET_DISABLED, true>), g, b, 0, v->stream, v->d, mp); break;
        }
        return MI_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// T vector steps with the cooperative physics: per step [sample actions ->] physics -> glue, all on the env's stream.  Every MuJoCo kind's rollout
// takes this form while RepeatAction / StickyAction are on (launch_mj_step_wrapped): a sticky action then replaces the drawn one, whose draws are
// consumed either way.
int launch_mj_rollout_coop(mi_vecenv *v, const RolloutPtrs &p, const ActionStream &as, int T, bool sample, int in_f64, const RolloutExtra &ex) {
    const size_t N = (size_t)v->cfg.num_envs, nu = (size_t)v->lay.act_dim, info_dim = (size_t)v->lay.info_dim;
    // the glue kernel writes a final_obs / final_info row only where an episode ended (mi_step's contract): the other rows are zeros (mi_rollout_extra)
    if (ex.final_obs) HIP_TRY(hipMemsetAsync(ex.final_obs, 0, (size_t)T * N * v->lay.obs_dim * sizeof(double), v->stream));
    if (ex.final_info) HIP_TRY(hipMemsetAsync(ex.final_info, 0, (size_t)T * N * info_dim * sizeof(double), v->stream));
    for (int t = 0; t < T; t++) {
        const void *act;
        if (sample) {
            float *dst = p.actions_out ? static_cast<float *>(p.actions_out) + (size_t)t * N * nu : v->d_act_scratch;
            if (!Stock::dispatch(v->cfg.kind, [&](auto env) {
                    hipLaunchKernelGGL((mj_sample_kernel<decltype(env)>), dim3(v->grid), dim3(kBlock), 0, v->stream, v->d, as, t, dst);
                }))
                return fail(MI_ERR_UNSUPPORTED, kNoLaneKernel);
            act = dst;
        } else if (in_f64) {
            act = static_cast<const double *>(p.actions_in) + (size_t)t * N * nu;
        } else {
            act = static_cast<const float *>(p.actions_in) + (size_t)t * N * nu;
        }
        MjStepPtrs mp;
        memset(&mp, 0, sizeof mp);
        mp.actions = act, mp.act_f64 = !sample && in_f64;
        mp.obs = p.obs ? static_cast<double *>(p.obs) + (size_t)t * N * v->lay.obs_dim : static_cast<double *>(v->d_obs_scratch);
        mp.reward = p.reward ? p.reward + (size_t)t * N : nullptr;
        mp.terminated = p.terminated ? p.terminated + (size_t)t * N : nullptr;
        mp.truncated = p.truncated ? p.truncated + (size_t)t * N : nullptr;
        mp.obs_dim = v->lay.obs_dim;
        mp.final_obs = ex.final_obs ? static_cast<double *>(ex.final_obs) + (size_t)t * N * v->lay.obs_dim : nullptr;
        mp.ep_ret = ex.ep_ret ? ex.ep_ret + (size_t)t * N : nullptr;
        mp.ep_len = ex.ep_len ? ex.ep_len + (size_t)t * N : nullptr;
        // (the finishing step's info reaches final_info through the info row: without a caller's array the env's own staging row serves)
        mp.info = ex.info ? ex.info + (size_t)t * N * info_dim : (ex.final_info ? v->d_info : nullptr);
        mp.final_info = ex.final_info ? ex.final_info + (size_t)t * N * info_dim : nullptr;
        if (const int rc = launch_mj_step(v, mp)) return rc;
    }
    return MI_OK;
}

const double kUnitMassScale[32] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};

}  // namespace

namespace mi_mujoco {

bool configure(mi_vecenv *v) {
    const mi_config &cfg = v->cfg;
    mi::EnvParams P;
    for (int k = 0; k < 16; k++) P.p[k] = cfg.params[k];
    return Stock::dispatch(cfg.kind, [&](auto env) {
        using E = decltype(env);
        const mi_layout l = {E::obs_dim_host(P), MI_F64, E::NU, MI_F32, E::S, E::INFO, {0, 0}};
        v->lay = l;
        v->extras_dim = mjx::coop::Sim<typename E::Model, E::COOP_G>::EX_TOTAL;
        // Which physics kernel: the cooperative one (mjx_coop.h) wins where the robot fills its 16 / 32 lanes (Ant 2.4M vs 1.4M env-steps/s, Humanoid 0.76M
        // vs 0.23M; at 65536 envs HalfCheetah 22.0 M vs 18.8 M one-lane, Walker2d 8.4 M vs 6.6 M) -- not for Hopper: 9.7 M vs 17.2 M.
        // MI355ENV_MJ_SERIAL=1 / MI355ENV_MJ_COOP=1 force either one (cross-check tests).
        const char *serial = getenv("MI355ENV_MJ_SERIAL"), *coop = getenv("MI355ENV_MJ_COOP");
        v->mj_coop = cfg.kind != MI_ENV_HOPPER;
        if (serial && serial[0] == '1') v->mj_coop = false;
        if (coop && coop[0] == '1') v->mj_coop = true;
        if (!E::HAS_COOP) v->mj_coop = false;  // the other small robots: one-lane kernel only (cylinder geoms, fluid forces, two-dof arms)
    });
}

bool model_field_info(int kind, ModelFieldInfo &out) {
    return Stock::dispatch(kind, [&](auto env) {
        typedef typename decltype(env)::Model M;
        typedef mjx::MassLaneFields<M> V;
        static_assert(M::NBODY <= 32, "kUnitMassScale");
        static const double kMeanInertia = M::MEANINERTIA;  // (one per robot: the lambda is instantiated per env type)
        const ModelFieldInfo f = {{3, M::NU, M::NV, M::NPAIR, M::NBODY}, {V::OFF_GRAVITY, V::OFF_GEAR, V::OFF_DAMPING, V::OFF_FRICTION, V::OFF_MASS_SCALE}, V::WIDTH,
                                  {M::gravity, M::actuator_gear, M::dof_damping, M::pair_friction, kUnitMassScale},
                                  {M::NV, 2 * M::NBODY, 1}, {V::OFF_DOF_INVWEIGHT, V::OFF_BODY_INVWEIGHT, V::OFF_MEANINERTIA},
                                  {M::dof_invweight0, &M::body_invweight0[0][0], &kMeanInertia}};
        out = f;
    });
}

bool action_bounds(int kind, double *lo, double *range) {
    return Stock::dispatch(kind, [&](auto env) {
        using E = decltype(env);
        for (int u = 0; u < E::NU; u++) {
            const double l = (double)(float)E::Model::actuator_ctrlrange[u][0], h = (double)(float)E::Model::actuator_ctrlrange[u][1];
            lo[u] = l, range[u] = h - l;
        }
    });
}

int reset(mi_vecenv *v, const uint8_t *device_mask, double *device_obs) {
    if (!lane_launchers(v).reset(v->cfg.kind, v->grid, v->stream, v->d, device_mask, device_obs, v->lay.obs_dim)) return fail(MI_ERR_UNSUPPORTED, kNoLaneKernel);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

int step(mi_vecenv *v, const StepPtrs &p, double *info, double *final_info, int act_kind) {
    const MjStepPtrs mp = {p.actions, (double *)p.obs, p.reward, p.terminated, p.truncated, (double *)p.final_obs,
                           p.ep_ret, p.ep_len, info, final_info, v->lay.obs_dim, nullptr, act_kind != MI_F32};
    if (!mp.obs) return fail(MI_ERR_INVALID_ARGUMENT, "obs is NULL");
    return launch_mj_step(v, mp);
}

int rollout(mi_vecenv *v, const RolloutPtrs &p, const ActionStream &as, int T, bool sample, int in_f64, const RolloutExtra *ex) {
    const RolloutExtra e = ex ? *ex : RolloutExtra{};
    if (v->wrap_on || runs_coop(v)) return launch_mj_rollout_coop(v, p, as, T, sample, in_f64, e);
    if (!lane_launchers(v).rollout(v->cfg.kind, v->cfg.autoreset_mode, sample, v->grid, v->stream, v->d, p, as, T, v->lay.obs_dim, in_f64, e))
        return fail(MI_ERR_UNSUPPORTED, kNoLaneKernel);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace mi_mujoco
