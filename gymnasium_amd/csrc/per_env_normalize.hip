// per_env_normalize.hip -- gymnasium.wrappers.NormalizeObservation / NormalizeReward around every SCALAR env of a vector env
// (mi_per_env_normalize_step, mi_per_env_normalize_steps; include/mi355env.h): one set of running statistics per sub-environment, updated from
// a batch of one -- what SyncVectorEnv over wrapped scalar envs computes (gymnasium v1.4.0):
//   gymnasium/wrappers/stateful_observation.py:464-561   NormalizeObservation.observation
//   gymnasium/wrappers/stateful_reward.py:20-142         NormalizeReward.step
//   gymnasium/wrappers/utils.py:33-71                    RunningMeanStd
//   gymnasium/vector/sync_vector_env.py:266-337          which rows step, which rows reset, final_obs
//
// Nothing here reduces over the batch: a lane's recurrence is sequential and every operation is an IEEE add / multiply / divide / sqrt, written out
// in per_env_normalize_internal.h as the host compiles it too.  This unit is built with the default flag set (-ffp-contract=off, no fast-math) and
// relies on hipcc's default correctly rounded float32 division and sqrtf for HIP.
//
// Layout of both kernels: the first obs_blocks workgroups hold one thread per (row, column) of the observation block -- consecutive threads read
// consecutive elements, so a step's reads and writes are coalesced --, the other workgroups one thread per row for the reward (behind the observation
// workgroups in step_kernel, in front of them in steps_kernel).  A wavefront is never split between the two.  A row's count and first-update flag are read by the D threads of the row and rewritten by the thread of column 0;
// they are double-buffered (read half `phase`, write the other) so that no thread can read what another has already replaced.
//
// step_kernel: what one reset() / step() returns.  Optionally the SAME_STEP final observations of the rows that just finished go through first
// (update, normalise), then the rows' own observations: two updates in one launch.  Rows outside row_mask (a masked reset) keep their statistics
// and get the value they were given last.
// steps_kernel: the T steps of a rollout.  A thread loads its statistics once, walks t = 0 .. T-1 over obs[t][row][column] with them in registers
// and stores them once; the traffic is one read and one write of the trajectory.  T calls of step_kernel leave the same values and the same state.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mi355env.h"
#include "per_env_normalize_internal.h"

namespace mi_internal {
int set_error(int code, const char *msg);
}

namespace {

constexpr int kBlock = 256;

struct Args {
    // observation half (mean == nullptr: absent)
    void *mean, *var;
    const double *count_in;
    double *count_out;
    const uint8_t *first_in;
    uint8_t *first_out;
    const void *obs;
    float *obs_out;
    const uint8_t *row_mask;
    const float *prev_out;
    const void *final_obs;
    float *final_out;
    const uint8_t *final_mask;
    double obs_epsilon;
    int64_t obs_elements;  // N * D
    int obs_dim, obs_update, obs_blocks, reward_blocks;
    // reward half (reward == nullptr: absent)
    int reward_update, next_step, num_envs, steps;
    double *acc, *ret_mean, *ret_var, *ret_count;
    uint8_t *was_done;
    const double *reward;
    const uint8_t *terminated, *truncated;
    double *reward_out;
    double gamma, reward_epsilon;
};

// one step of one sub-environment's reward; `wd`: the row finished in the previous step
__device__ __forceinline__ double reward_of_step(const Args &a, double r, bool terminated, bool wd, double &acc, double &mean, double &var, double &count) {
    if (a.next_step && wd) return 0.0;  // the autoreset step: the vector env's 0.0, the scalar wrapper is not stepped
    mi_per_env::reward_step(r, terminated, a.gamma, a.reward_update != 0, acc, mean, var, count);
    return mi_per_env::normalize_reward(r, var, a.reward_epsilon);
}

template <class T>
__global__ __launch_bounds__(kBlock) void step_kernel(const Args a) {
    if ((int)blockIdx.x < a.obs_blocks) {
        const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (e >= a.obs_elements) return;
        const int row = (int)(e / a.obs_dim);
        const bool col0 = e - (int64_t)row * a.obs_dim == 0;
        double count = a.count_in[row];
        bool first = a.first_in[row] != 0;
        const bool finished = a.final_mask && a.final_mask[row];
        if (a.final_mask && !finished) a.final_out[e] = 0.0f;
        if (!a.row_mask || a.row_mask[row]) {
            T *mean = (T *)a.mean, *var = (T *)a.var;
            T m = mean[e], v = var[e];
            const bool update = a.obs_update != 0;
            if (finished) {
                const T x = ((const T *)a.final_obs)[e];
                if (update) mi_per_env::update(x, m, v, count, first), first = false;
                a.final_out[e] = mi_per_env::normalize(x, m, v, a.obs_epsilon);
            }
            const T x = ((const T *)a.obs)[e];
            if (update) {
                mi_per_env::update(x, m, v, count, first), first = false;
                mean[e] = m, var[e] = v;
            }
            a.obs_out[e] = mi_per_env::normalize(x, m, v, a.obs_epsilon);
        } else if (a.prev_out) {
            a.obs_out[e] = a.prev_out[e];
        }
        if (col0) a.count_out[row] = count, a.first_out[row] = first ? 1 : 0;
        return;
    }
    const int row = ((int)blockIdx.x - a.obs_blocks) * kBlock + threadIdx.x;
    if (row >= a.num_envs) return;
    const bool wd = a.was_done[row] != 0, te = a.terminated[row] != 0, tr = a.truncated[row] != 0;
    double acc = a.acc[row], mean = a.ret_mean[row], var = a.ret_var[row], count = a.ret_count[row];
    a.reward_out[row] = reward_of_step(a, a.reward[row], te, wd, acc, mean, var, count);
    a.acc[row] = acc, a.ret_mean[row] = mean, a.ret_var[row] = var, a.ret_count[row] = count;
    a.was_done[row] = (te || tr) ? 1 : 0;
}

// steps_kernel reads kAhead steps ahead: the loads of the next group are issued before the current group's chain of divisions and square roots,
// whose latency would otherwise sit between two loads (the compiler cannot move them itself: out may alias in).  A thread owns its (row, column)
// for all t, so a load of step t + kAhead never meets a store of step t.
constexpr int kAhead = 4;

template <class T>
__global__ __launch_bounds__(kBlock) void steps_kernel(const Args a) {
    // the reward rows first: one thread per row walks T float64 divisions and square roots, the longest chain of the launch -- it starts with the grid
    if ((int)blockIdx.x >= a.reward_blocks) {
        const int64_t e = (int64_t)((int)blockIdx.x - a.reward_blocks) * kBlock + threadIdx.x;
        if (e >= a.obs_elements) return;
        const int row = (int)(e / a.obs_dim);
        const bool col0 = e - (int64_t)row * a.obs_dim == 0;
        double count = a.count_in[row];
        bool first = a.first_in[row] != 0;
        T *mean = (T *)a.mean, *var = (T *)a.var;
        T m = mean[e], v = var[e];
        const bool update = a.obs_update != 0;
        const T *in = (const T *)a.obs + e;
        float *out = a.obs_out + e;
        T next[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; k++) next[k] = k < a.steps ? in[(int64_t)k * a.obs_elements] : T(0);
        for (int t = 0; t < a.steps; t += kAhead) {
            T x[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; k++) x[k] = next[k];
#pragma unroll
            for (int k = 0; k < kAhead; k++) next[k] = t + kAhead + k < a.steps ? in[(int64_t)(t + kAhead + k) * a.obs_elements] : T(0);
#pragma unroll
            for (int k = 0; k < kAhead; k++) {
                if (t + k < a.steps) {
                    if (update) mi_per_env::update(x[k], m, v, count, first), first = false;
                    out[(int64_t)(t + k) * a.obs_elements] = mi_per_env::normalize(x[k], m, v, a.obs_epsilon);
                }
            }
        }
        if (update) mean[e] = m, var[e] = v;
        if (col0) a.count_out[row] = count, a.first_out[row] = first ? 1 : 0;
        return;
    }
    const int row = (int)blockIdx.x * kBlock + threadIdx.x;
    if (row >= a.num_envs) return;
    bool wd = a.was_done[row] != 0;
    double acc = a.acc[row], mean = a.ret_mean[row], var = a.ret_var[row], count = a.ret_count[row];
    double nr[kAhead];
    uint8_t nte[kAhead], ntr[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; k++) {
        const int64_t i = (int64_t)k * a.num_envs + row;
        const bool in_range = k < a.steps;
        nr[k] = in_range ? a.reward[i] : 0.0, nte[k] = in_range ? a.terminated[i] : 0, ntr[k] = in_range ? a.truncated[i] : 0;
    }
    for (int t = 0; t < a.steps; t += kAhead) {
        double r[kAhead];
        uint8_t te[kAhead], tr[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; k++) r[k] = nr[k], te[k] = nte[k], tr[k] = ntr[k];
#pragma unroll
        for (int k = 0; k < kAhead; k++) {
            const int64_t i = (int64_t)(t + kAhead + k) * a.num_envs + row;
            const bool in_range = t + kAhead + k < a.steps;
            nr[k] = in_range ? a.reward[i] : 0.0, nte[k] = in_range ? a.terminated[i] : 0, ntr[k] = in_range ? a.truncated[i] : 0;
        }
#pragma unroll
        for (int k = 0; k < kAhead; k++) {
            if (t + k < a.steps) {
                a.reward_out[(int64_t)(t + k) * a.num_envs + row] = reward_of_step(a, r[k], te[k] != 0, wd, acc, mean, var, count);
                wd = te[k] != 0 || tr[k] != 0;
            }
        }
    }
    a.acc[row] = acc, a.ret_mean[row] = mean, a.ret_var[row] = var, a.ret_count[row] = count;
    a.was_done[row] = wd ? 1 : 0;
}

int invalid(const char *msg) { return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, msg); }

// the parts of Args both entry points share; 0 or an mi_status
int fill(Args &a, const mi_per_env_state *s, int num_envs, const void *obs, void *obs_out, const double *reward, const uint8_t *terminated,
         const uint8_t *truncated, double *reward_out, const char *who) {
    char buf[200];
    a = Args{};
    if (!s || num_envs < 1 || (!obs && !reward)) {
        snprintf(buf, sizeof buf, "%s: needs a state, num_envs >= 1 and an observation or a reward block", who);
        return invalid(buf);
    }
    a.num_envs = num_envs;
    if (obs) {
        if (!s->obs_mean || !s->obs_var || !s->obs_count || !s->obs_first || !obs_out || s->obs_dim < 1 || (s->obs_phase != 0 && s->obs_phase != 1) ||
            (s->obs_dtype != MI_F32 && s->obs_dtype != MI_F64) || !(s->obs_epsilon > 0)) {
            snprintf(buf, sizeof buf, "%s: an observation block needs obs_mean / obs_var / obs_count / obs_first, obs_out, obs_dim >= 1, obs_phase 0 / 1, "
                                      "obs_dtype MI_F32 / MI_F64 and obs_epsilon > 0", who);
            return invalid(buf);
        }
        const int64_t elements = (int64_t)num_envs * s->obs_dim;
        if (elements >= ((int64_t)1 << 31)) {
            snprintf(buf, sizeof buf, "%s: num_envs * obs_dim must stay below 2^31", who);
            return invalid(buf);
        }
        const uintptr_t size = s->obs_dtype == MI_F32 ? 4 : 8;
        if ((uintptr_t)obs % size || (uintptr_t)s->obs_mean % size || (uintptr_t)s->obs_var % size || (uintptr_t)obs_out % 4 || (uintptr_t)s->obs_count % 8) {
            snprintf(buf, sizeof buf, "%s: a pointer of the observation block is not aligned to its element type", who);
            return invalid(buf);
        }
        a.mean = s->obs_mean, a.var = s->obs_var;
        a.count_in = s->obs_count + (int64_t)s->obs_phase * num_envs, a.count_out = s->obs_count + (int64_t)(1 - s->obs_phase) * num_envs;
        a.first_in = s->obs_first + (int64_t)s->obs_phase * num_envs, a.first_out = s->obs_first + (int64_t)(1 - s->obs_phase) * num_envs;
        a.obs = obs, a.obs_out = (float *)obs_out;
        a.obs_epsilon = s->obs_epsilon, a.obs_elements = elements, a.obs_dim = s->obs_dim, a.obs_update = s->obs_update;
        a.obs_blocks = (int)((elements + kBlock - 1) / kBlock);
    }
    if (reward) {
        if (!s->ret_mean || !s->ret_var || !s->ret_count || !s->acc || !s->was_done || !terminated || !truncated || !reward_out ||
            !(s->gamma >= 0 && s->gamma <= 1) || !(s->reward_epsilon > 0) || s->autoreset_mode < MI_AUTORESET_NEXT_STEP ||
            s->autoreset_mode > MI_AUTORESET_DISABLED) {
            snprintf(buf, sizeof buf, "%s: a reward block needs acc / ret_mean / ret_var / ret_count / was_done, terminated, truncated, reward_out, gamma in "
                                      "[0, 1], reward_epsilon > 0 and an autoreset mode", who);
            return invalid(buf);
        }
        if ((uintptr_t)reward % 8 || (uintptr_t)reward_out % 8 || (uintptr_t)s->acc % 8 || (uintptr_t)s->ret_mean % 8 || (uintptr_t)s->ret_var % 8 ||
            (uintptr_t)s->ret_count % 8) {
            snprintf(buf, sizeof buf, "%s: a pointer of the reward block is not aligned to float64", who);
            return invalid(buf);
        }
        a.acc = s->acc, a.ret_mean = s->ret_mean, a.ret_var = s->ret_var, a.ret_count = s->ret_count, a.was_done = s->was_done;
        a.reward = reward, a.terminated = terminated, a.truncated = truncated, a.reward_out = reward_out;
        a.gamma = s->gamma, a.reward_epsilon = s->reward_epsilon, a.reward_update = s->reward_update;
        a.next_step = s->autoreset_mode == MI_AUTORESET_NEXT_STEP;
        a.reward_blocks = (num_envs + kBlock - 1) / kBlock;
    }
    return MI_OK;
}

template <class T>
hipError_t launch(bool trajectory, hipStream_t st, const Args &a) {
    const unsigned blocks = (unsigned)a.obs_blocks + (unsigned)a.reward_blocks;
    if (trajectory)
        hipLaunchKernelGGL(steps_kernel<T>, dim3(blocks), dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL(step_kernel<T>, dim3(blocks), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

int enqueue(bool trajectory, int device, void *hip_stream, const Args &a, int obs_dtype, const char *who) {
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess)
        e = (a.obs && obs_dtype == MI_F64) ? launch<double>(trajectory, (hipStream_t)hip_stream, a) : launch<float>(trajectory, (hipStream_t)hip_stream, a);
    if (e == hipSuccess) return MI_OK;
    char buf[300];
    snprintf(buf, sizeof buf, "%s failed: %s", who, hipGetErrorString(e));
    return mi_internal::set_error(MI_ERR_HIP, buf);
}

}  // namespace

#pragma GCC visibility push(default)

int mi_per_env_normalize_step(int device, void *hip_stream, const mi_per_env_state *state, int num_envs, const void *obs, void *obs_out,
                              const uint8_t *row_mask, const void *prev_out, const void *final_obs, void *final_out, const uint8_t *final_mask,
                              const double *reward, const uint8_t *terminated, const uint8_t *truncated, double *reward_out) {
    const char *who = "mi_per_env_normalize_step";
    Args a;
    const int rc = fill(a, state, num_envs, obs, obs_out, reward, terminated, truncated, reward_out, who);
    if (rc != MI_OK) return rc;
    const bool any_final = final_obs || final_out || final_mask, all_final = final_obs && final_out && final_mask;
    if (any_final && (!all_final || !obs))
        return invalid("mi_per_env_normalize_step: final_obs, final_out and final_mask come together, with an observation block");
    if (!obs && (row_mask || prev_out)) return invalid("mi_per_env_normalize_step: row_mask / prev_out belong to an observation block");
    if (all_final && ((uintptr_t)final_obs % (state->obs_dtype == MI_F32 ? 4 : 8) || (uintptr_t)final_out % 4))
        return invalid("mi_per_env_normalize_step: final_obs / final_out are not aligned to their element types");
    if (prev_out && (uintptr_t)prev_out % 4) return invalid("mi_per_env_normalize_step: prev_out is not aligned to float32");
    a.row_mask = row_mask, a.prev_out = (const float *)prev_out;
    a.final_obs = final_obs, a.final_out = (float *)final_out, a.final_mask = final_mask;
    a.steps = 1;
    return enqueue(false, device, hip_stream, a, state->obs_dtype, who);
}

int mi_per_env_normalize_steps(int device, void *hip_stream, const mi_per_env_state *state, int T, int num_envs, const void *obs, void *obs_out,
                               const double *reward, const uint8_t *terminated, const uint8_t *truncated, double *reward_out) {
    const char *who = "mi_per_env_normalize_steps";
    Args a;
    const int rc = fill(a, state, num_envs, obs, obs_out, reward, terminated, truncated, reward_out, who);
    if (rc != MI_OK) return rc;
    if (T < 1) return invalid("mi_per_env_normalize_steps: T must be at least 1");
    if (state->autoreset_mode == MI_AUTORESET_SAME_STEP)
        return mi_internal::set_error(MI_ERR_UNSUPPORTED, "mi_per_env_normalize_steps: under SAME_STEP the final observations of the rows that finish update "
                                                          "the statistics between two steps; run the steps through mi_per_env_normalize_step");
    a.steps = T;
    return enqueue(true, device, hip_stream, a, state->obs_dtype, who);
}

#pragma GCC visibility pop
