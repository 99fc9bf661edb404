// mjx_mass_model.hip -- the one-lane MuJoCo kernels of an env with a per-sub-environment body mass scale (mi_set_model_field MI_MODEL_BODY_MASS_SCALE):
// namespace mi_mjmass, the launchers of mj_step_kernel / mj_rollout_kernel / mj_reset_kernel (mj_glue_kernels.h, through mj_lane_launch.h) over the
// mjx::MassLaneModel env types, and mj_model_constants_kernel, which derives dof_invweight0, body_invweight0 and meaninertia of every sub-environment.
// A unit and a model type of their own: the kernels of mjx_model.hip, which an env with only the other four fields runs, neither load nor carry the
// mass rows.  Default flag set.  As everywhere on this path the parity with `mujoco` is unpinned; the CPU oracle is the reference.
#include "mj_lane_launch.h"

namespace {
// The constants a model compiler derives from the body masses, for every sub-environment from its body mass scale: one lane per sub-environment runs the
// simulator's own position stage and factorisation at qpos0 through the lane's view (mjx_core.h derive_mass_constants) and writes its column of the
// derived rows.  rows = the env's [MassLaneFields::WIDTH][N] block, component-major: every load and store of a wavefront is one contiguous run.
template <class M0>
__global__ __launch_bounds__(kBlock) void mj_model_constants_kernel(double *rows, int N) {
    typedef mjx::MassLaneModel<M0> M;
    typedef mjx::MassLaneFields<M0> F;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    F fields;
    fields.load_mass_scale(rows, (size_t)N, (size_t)i);
    mjx::Data<M> d;
    d.bind(&fields);
    double dof[M0::NV], body[M0::NBODY][2], mean;
    mjx::derive_mass_constants<M>(d, dof, body, mean);
    for (int k = 0; k < M0::NV; k++) rows[(size_t)(F::OFF_DOF_INVWEIGHT + k) * N + i] = dof[k];
    for (int k = 0; k < 2 * M0::NBODY; k++) rows[(size_t)(F::OFF_BODY_INVWEIGHT + k) * N + i] = body[k / 2][k % 2];
    rows[(size_t)F::OFF_MEANINERTIA * N + i] = mean;
}
}  // namespace

namespace mi_mjmass {
typedef MjLaneLaunch<mjx::MassLaneModel> Launch;
bool preload(int kind) {  // the step kernel and the constants kernel: both sit in this unit's code object
    hipError_t err = hipSuccess;
    const bool held = Launch::dispatch(kind, [&](auto env) {
        hipFuncAttributes attr;
        err = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&mj_model_constants_kernel<typename decltype(env)::Model::Stock>));
    });
    return held && err == hipSuccess && Launch::preload(kind);
}
bool step(int kind, int mode, int grid, hipStream_t stream, const DevEnv &d, const void *mj_step_ptrs) { return Launch::step(kind, mode, grid, stream, d, mj_step_ptrs); }
bool step_wrapped(int kind, int mode, int trip, int grid, hipStream_t stream, const DevEnv &d, const void *mj_step_ptrs, const MjWrapDev &w) {
    return Launch::step_wrapped(kind, mode, trip, grid, stream, d, mj_step_ptrs, w);
}
bool rollout(int kind, int mode, bool sample, int grid, hipStream_t stream, const DevEnv &d, const RolloutPtrs &p, const ActionStream &as, int T, int obs_dim,
             int in_f64, const RolloutExtra &ex) {
    return Launch::rollout(kind, mode, sample, grid, stream, d, p, as, T, obs_dim, in_f64, ex);
}
bool reset(int kind, int grid, hipStream_t stream, const DevEnv &d, const uint8_t *mask, double *obs, int obs_dim) {
    return Launch::reset(kind, grid, stream, d, mask, obs, obs_dim);
}
bool derive_constants(int kind, int grid, hipStream_t stream, double *rows, int N) {
    return Launch::dispatch(kind, [&](auto env) {
        typedef typename decltype(env)::Model::Stock M0;
        hipLaunchKernelGGL((mj_model_constants_kernel<M0>), dim3(grid), dim3(kBlock), 0, stream, rows, N);
    });
}
}  // namespace mi_mjmass
