// mj_lane_launch.h -- the launchers of the one-lane MuJoCo kernels (mj_glue_kernels.h, mj_wrapped_kernels.h) over the env types of one per-lane model template:
// the stock model itself (mujoco.hip), mjx::LaneModel (mjx_model.hip, namespace mi_mjmodel) or mjx::MassLaneModel (mjx_mass_model.hip, namespace mi_mjmass).  Each of the three units
// instantiates the kernels it launches; engine_types.h declares the plain functions mujoco.hip calls for the other two.
#ifndef MI355ENV_MJ_LANE_LAUNCH_H
#define MI355ENV_MJ_LANE_LAUNCH_H
#include "mj_glue_kernels.h"
#include "mj_wrapped_kernels.h"

namespace {
template <template <class> class LM>
struct MjLaneLaunch {
    template <class M0, int KIND>
    using Env = mjx::MjEnv<LM<M0>, KIND>;
    template <class F>
    static bool dispatch(int kind, F &&f) {
        switch (kind) {
        case MI_ENV_HALF_CHEETAH: f(Env<mjx::HalfCheetahModel, mjx::kHalfCheetah>()); return true;
        case MI_ENV_ANT: f(Env<mjx::AntModel, mjx::kAnt>()); return true;
        case MI_ENV_HUMANOID: f(Env<mjx::HumanoidModel, mjx::kHumanoid>()); return true;
        case MI_ENV_HOPPER: f(Env<mjx::HopperModel, mjx::kHopper>()); return true;
        case MI_ENV_WALKER2D: f(Env<mjx::Walker2dModel, mjx::kWalker2d>()); return true;
        case MI_ENV_INVERTED_PENDULUM: f(Env<mjx::InvertedPendulumModel, mjx::kInvertedPendulum>()); return true;
        case MI_ENV_INVERTED_DOUBLE_PENDULUM: f(Env<mjx::InvertedDoublePendulumModel, mjx::kInvertedDoublePendulum>()); return true;
        case MI_ENV_REACHER: f(Env<mjx::ReacherModel, mjx::kReacher>()); return true;
        case MI_ENV_HUMANOID_STANDUP: f(Env<mjx::HumanoidStandupModel, mjx::kHumanoidStandup>()); return true;
        case MI_ENV_SWIMMER: f(Env<mjx::SwimmerModel, mjx::kSwimmer>()); return true;
        case MI_ENV_PUSHER: f(Env<mjx::PusherModel, mjx::kPusher>()); return true;
        }
        return false;
    }
    static bool preload(int kind) {
        hipError_t err = hipSuccess;
        const bool held = dispatch(kind, [&](auto env) {
            hipFuncAttributes attr;
            err = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&mj_step_kernel<decltype(env), MI_AUTORESET_NEXT_STEP, false>));
        });
        return held && err == hipSuccess;
    }
    static bool step(int kind, int mode, int grid, hipStream_t stream, const DevEnv &d, const void *mj_step_ptrs) {
        const MjStepPtrs mp = *static_cast<const MjStepPtrs *>(mj_step_ptrs);
        const dim3 g(grid), b(kBlock);
        return dispatch(kind, [&](auto env) {
            using E = decltype(env);
            switch (mode) {
            case MI_AUTORESET_NEXT_STEP: hipLaunchKernelGGL((mj_step_kernel<E, MI_AUTORESET_NEXT_STEP, false>), g, b, 0, stream, d, mp); break;
            case MI_AUTORESET_SAME_STEP: hipLaunchKernelGGL((mj_step_kernel<E, MI_AUTORESET_SAME_STEP, false>), g, b, 0, stream, d, mp); break;
            default: hipLaunchKernelGGL((mj_step_kernel<E, MI_AUTORESET_DISABLED, false>), g, b, 0, stream, d, mp); break;
            }
        });
    }
    // trip `trip` of an outer step with RepeatAction / StickyAction on (mj_wrapped_kernels.h)
    static bool step_wrapped(int kind, int mode, int trip, int grid, hipStream_t stream, const DevEnv &d, const void *mj_step_ptrs, const MjWrapDev &w) {
        const MjStepPtrs mp = *static_cast<const MjStepPtrs *>(mj_step_ptrs);
        return dispatch(kind, [&](auto env) { hipLaunchKernelGGL((mj_trip_kernel<decltype(env), false>), dim3(grid), dim3(kBlock), 0, stream, d, mp, w, mode, trip); });
    }
    static bool reset(int kind, int grid, hipStream_t stream, const DevEnv &d, const uint8_t *mask, double *obs, int obs_dim) {
        return dispatch(kind, [&](auto env) { hipLaunchKernelGGL((mj_reset_kernel<decltype(env)>), dim3(grid), dim3(kBlock), 0, stream, d, mask, obs, obs_dim); });
    }
    static bool rollout(int kind, int mode, bool sample, int grid, hipStream_t stream, const DevEnv &d, const RolloutPtrs &p, const ActionStream &as, int T, int obs_dim,
                 int in_f64, const RolloutExtra &ex) {
        const dim3 g(grid), b(kBlock);
        return dispatch(kind, [&](auto env) {
            using E = decltype(env);
            const bool next = mode == MI_AUTORESET_NEXT_STEP;  // (mi_rollout refuses a DISABLED env)
            if (next && sample)
                hipLaunchKernelGGL((mj_rollout_kernel<E, MI_AUTORESET_NEXT_STEP, true>), g, b, 0, stream, d, p, as, T, obs_dim, in_f64, ex);
            else if (next)
                hipLaunchKernelGGL((mj_rollout_kernel<E, MI_AUTORESET_NEXT_STEP, false>), g, b, 0, stream, d, p, as, T, obs_dim, in_f64, ex);
            else if (sample)
                hipLaunchKernelGGL((mj_rollout_kernel<E, MI_AUTORESET_SAME_STEP, true>), g, b, 0, stream, d, p, as, T, obs_dim, in_f64, ex);
            else
                hipLaunchKernelGGL((mj_rollout_kernel<E, MI_AUTORESET_SAME_STEP, false>), g, b, 0, stream, d, p, as, T, obs_dim, in_f64, ex);
        });
    }
};
}  // namespace
#endif  // MI355ENV_MJ_LANE_LAUNCH_H
