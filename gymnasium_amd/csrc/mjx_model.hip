// mjx_model.hip -- the one-lane MuJoCo kernels of an env with per-sub-environment model fields (mi_set_model_field) as a translation unit of their
// own: namespace mi_mjmodel, the launchers of mj_step_kernel / mj_rollout_kernel (mj_glue_kernels.h, through mj_lane_launch.h) over the mjx::LaneModel
// env types; engine_types.h declares them and says why.  A unit of its own so that its 77 kernels compile beside the stock models' (mujoco.hip) instead of after them.  Default
// flag set, like mujoco.hip's one-lane kernels.  (An env with a body mass scale runs the kernels of mjx_mass_model.hip instead.)
// As everywhere on this path the parity with `mujoco` is unpinned; the CPU oracle is the reference for these fields.
#include "mj_lane_launch.h"

namespace mi_mjmodel {
typedef MjLaneLaunch<mjx::LaneModel> Launch;
bool preload(int kind) { return Launch::preload(kind); }
bool step(int kind, int mode, int grid, hipStream_t stream, const DevEnv &d, const void *mj_step_ptrs) { return Launch::step(kind, mode, grid, stream, d, mj_step_ptrs); }
bool step_wrapped(int kind, int mode, int trip, int grid, hipStream_t stream, const DevEnv &d, const void *mj_step_ptrs, const MjWrapDev &w) {
    return Launch::step_wrapped(kind, mode, trip, grid, stream, d, mj_step_ptrs, w);
}
bool rollout(int kind, int mode, bool sample, int grid, hipStream_t stream, const DevEnv &d, const RolloutPtrs &p, const ActionStream &as, int T, int obs_dim,
             int in_f64, const RolloutExtra &ex) {
    return Launch::rollout(kind, mode, sample, grid, stream, d, p, as, T, obs_dim, in_f64, ex);
}
}  // namespace mi_mjmodel
