// mjx_model.hip -- the one-lane MuJoCo kernels of an env with per-sub-environment model fields (mi_set_model_field) as a translation unit of their
// own: engine.hip compiled with MI_MJ_MODEL_TU defines ONLY namespace mi_mjmodel (the launchers of mj_step_kernel / mj_rollout_kernel over the
// mjx::LaneModel env types; the head of that namespace in engine.hip says why).  Default flag set, like engine.hip's own one-lane kernels.
// As everywhere on this path the parity with `mujoco` is unpinned; the CPU oracle is the reference for these fields.
#define MI_MJ_MODEL_TU 1
#include "engine.hip"
