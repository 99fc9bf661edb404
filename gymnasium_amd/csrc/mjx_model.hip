// mjx_model.hip -- the one-lane MuJoCo kernels of an env with per-sub-environment model fields (mi_set_model_field) as a translation unit of their
// own: namespace mi_mjmodel, the launchers of mj_step_kernel / mj_rollout_kernel (mj_glue_kernels.h) over the mjx::LaneModel env types; engine_types.h
// declares them and says why.  A unit of its own so that its 77 kernels compile beside engine.o instead of after it.  Default flag set, like
// engine.hip's own one-lane kernels.
// As everywhere on this path the parity with `mujoco` is unpinned; the CPU oracle is the reference for these fields.
#include "mj_glue_kernels.h"

namespace mi_mjmodel {
template <class M0, int KIND>
using Env = mjx::MjEnv<mjx::LaneModel<M0>, KIND>;
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
bool preload(int kind) {
    hipError_t err = hipSuccess;
    const bool held = dispatch(kind, [&](auto env) {
        hipFuncAttributes attr;
        err = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&mj_step_kernel<decltype(env), MI_AUTORESET_NEXT_STEP, false>));
    });
    return held && err == hipSuccess;
}
bool step(int kind, int mode, int grid, hipStream_t stream, const DevEnv &d, const void *mj_step_ptrs) {
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
bool rollout(int kind, int mode, bool sample, int grid, hipStream_t stream, const DevEnv &d, const RolloutPtrs &p, const ActionStream &as, int T, int obs_dim,
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
}  // namespace mi_mjmodel
