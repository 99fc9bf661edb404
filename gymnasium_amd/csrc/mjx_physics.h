// mjx_physics.h -- the cooperative physics kernel (mjx_coop.h) behind a plain launch function, so that it can live in its own
// translation units: physics16.hip (16-lane groups: Ant, HalfCheetah) and physics32.hip (32-lane groups: Humanoid, HumanoidStandup) are
// compiled with different instruction-scheduler settings than mujoco.hip, which launches them (gymnasium_amd/csrc/build.py TU_FLAGS).
//
// Reference call sites replaced: gymnasium/envs/mujoco/mujoco_env.py:150 (mj_step(nstep = frame_skip)) and :155 (mj_rnePostConstraint),
// for every sub-environment that takes a real step in this vector step.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "../../include/mi355env.h"
#include "envs_classic.h"
#include "pcg64_dev.h"
#include "mjx_kernels.h"
#include "mjx_coop.h"

namespace mi_phys {

// what the kernel needs of the engine's device state (engine_types.h DevEnv): the component-major state rows [S][N] (qpos, qvel, the
// qacc_warmstart slot), the per-env meta word whose `needs_reset_mask` bits mark a sub-environment that resets instead of stepping
struct Args {
    double *state;
    const uint32_t *meta;
    uint32_t needs_reset_mask;
    int N, frame_skip;
    int newton;          // MI_CFG_SOLVER_NEWTON: run the Newton instantiation although the model's MJCF asks for PGS
    int act_f64;         // the action rows are float64 (taken un-rounded: mujoco_env.py:148 data.ctrl[:] = ctrl), not float32
};

// Advances qpos / qvel of every sub-environment that takes a real step this call by frame_skip sub-steps, in place, and leaves what
// the reward / observation code needs in `extras`.  Sub-environments in their NEXT_STEP autoreset step (or finished ones under DISABLED)
// are skipped: the step kernel that follows resets them / reports the error.
// PGS: the constraint solver of the model's MJCF (M::SOLVER == 1: humanoid.xml:8 `solver="PGS" iterations="50"`) or, false, the converged
// primal Newton solver (every other robot's MJCF default; opt-in for the humanoids, MI_CFG_SOLVER_NEWTON).
// MJX_MIN_WAVES_PER_EU (experiment switch, default 1): 2 caps the kernel at 256 registers (VGPRs + AGPRs) so that two wavefronts fit one SIMD --
// measured in round 4 (profiles/r04_two_waves.txt); the shipped kernels use the whole register file of a SIMD for one wavefront.
#ifndef MJX_MIN_WAVES_PER_EU
#define MJX_MIN_WAVES_PER_EU 1
#endif
template <class E, bool SKIP_RESETTING, bool PGS>
__global__ __launch_bounds__(64, MJX_MIN_WAVES_PER_EU) void mj_physics_kernel(Args d, const void *actions, double *extras) {
    typedef typename E::Model M;
    constexpr int G = E::COOP_G, EPW = 64 / G;
    typedef mjx::coop::Sim<M, G, PGS> S;
    __shared__ typename S::B boards[EPW];
    const int grp = threadIdx.x / G, lane = threadIdx.x % G;
    const int env = blockIdx.x * EPW + grp;
    // A sub-environment that does not step in this call (past the end of the batch, or in its NEXT_STEP autoreset step) retires its lanes.
    const bool steps = env < d.N && !(SKIP_RESETTING && (d.meta[env < d.N ? env : 0] & d.needs_reset_mask));
    if (!steps) return;
    typename S::B &bb = boards[grp];
    typename S::R r;
    r.grp = grp;
    S::init(bb, lane);
    const size_t N = (size_t)d.N;
    for (int k = lane; k < M::NQ; k += G) bb.qpos[k] = d.state[(size_t)k * N + env];
    for (int k = lane; k < M::NV; k += G) bb.qvel[k] = d.state[(size_t)(M::NQ + k) * N + env];
    if (d.act_f64) {  // (grid-uniform)
        for (int k = lane; k < M::NU; k += G) bb.ctrl[k] = static_cast<const double *>(actions)[(size_t)env * M::NU + k];
    } else {
        for (int k = lane; k < M::NU; k += G) bb.ctrl[k] = (double)static_cast<const float *>(actions)[(size_t)env * M::NU + k];
    }
    r.warm = lane < M::NV ? d.state[(size_t)(M::NQ + M::NV + lane) * N + env] : 0.0;  // qacc_warmstart slot of the state row
    mjx::coop::coop_sync();
    for (int f = 0; f < d.frame_skip; f++) S::step(bb, r, lane);
    mjx::coop::coop_sync();
    for (int k = lane; k < M::NQ; k += G) d.state[(size_t)k * N + env] = bb.qpos[k];
    for (int k = lane; k < M::NV; k += G) d.state[(size_t)(M::NQ + k) * N + env] = bb.qvel[k];
    if (lane < M::NV) d.state[(size_t)(M::NQ + M::NV + lane) * N + env] = r.warm;
    constexpr int WHAT = E::HUMANOID_LIKE ? 3 : (E::KIND_ID == mjx::kAnt ? 1 : 0);  // what the glue of this robot reads (mjx_kernels.h)
    S::template write_extras<WHAT>(bb, r, lane, extras + (size_t)env * S::EX_TOTAL);
}

// MI355ENV_PHYS_EXTRA_LDS=<bytes> (experiment switch): dynamic LDS added to every launch -- a way to LOWER the number of resident workgroups per CU
// without touching the kernel (round 4: the two-wavefronts-per-SIMD build measured at one wavefront per SIMD, profiles/r04_two_waves.txt)
inline unsigned extra_lds() {
    static const unsigned v = getenv("MI355ENV_PHYS_EXTRA_LDS") ? (unsigned)atoi(getenv("MI355ENV_PHYS_EXTRA_LDS")) : 0u;
    return v;
}
template <class E>
inline void launch_kind(const Args &a, bool skip_resetting, const void *actions, double *extras, hipStream_t stream) {
    constexpr int EPW = 64 / E::COOP_G;
    const dim3 grid((a.N + EPW - 1) / EPW), block(64);
    const unsigned dyn = extra_lds();
    if constexpr (E::Model::SOLVER == 1) {
        if (!a.newton) {
            if (skip_resetting)
                hipLaunchKernelGGL((mj_physics_kernel<E, true, true>), grid, block, dyn, stream, a, actions, extras);
            else
                hipLaunchKernelGGL((mj_physics_kernel<E, false, true>), grid, block, dyn, stream, a, actions, extras);
            return;
        }
    }
    if (skip_resetting)
        hipLaunchKernelGGL((mj_physics_kernel<E, true, false>), grid, block, dyn, stream, a, actions, extras);
    else
        hipLaunchKernelGGL((mj_physics_kernel<E, false, false>), grid, block, dyn, stream, a, actions, extras);
}

// defined in physics16.hip / physics32.hip; `kind` is an mi_env_kind; returns false for a kind the unit does not hold
bool launch16(int kind, const Args &a, bool skip_resetting, const void *actions, double *extras, hipStream_t stream);
bool launch32(int kind, const Args &a, bool skip_resetting, const void *actions, double *extras, hipStream_t stream);

}  // namespace mi_phys
