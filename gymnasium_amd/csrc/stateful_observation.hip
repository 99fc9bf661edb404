// stateful_observation.hip -- gymnasium.wrappers.FrameStackObservation / DelayObservation / TimeAwareObservation around every SCALAR env of a
// vector env (mi_stateful_observation_step, mi_stateful_observation_steps; include/mi355env.h): what SyncVectorEnv over wrapped scalar envs
// returns (gymnasium v1.4.0):
//   gymnasium/wrappers/stateful_observation.py:35-103    DelayObservation
//   gymnasium/wrappers/stateful_observation.py:106-301   TimeAwareObservation
//   gymnasium/wrappers/stateful_observation.py:304-461   FrameStackObservation
//   gymnasium/vector/sync_vector_env.py:207-337          which rows step, which rows reset, final_obs
//
// The three wrappers move data; the only arithmetic is the normalised time (one float64 division rounded once to float32) and the exact
// widenings float32 -> float64 / int32 -> float64.  Which source feeds an output element is decided in stateful_observation_internal.h, which
// the host compiles too.  Every launch READS the carried state (the last stack, the delay history, the counters, the pending-autoreset flags)
// from one set of arrays and WRITES the new state to another: nothing is shifted in place, so no lane can read what another has replaced.
//
// step_kernel (one reset() / step()): one thread per element of the larger of the output and the new state.
// stack_steps_kernel (FrameStack / Delay over a rollout [T][N][D]): a pure write stream, k times the input for FrameStack, parallel over all
//   T x N outputs.  A thread owns 16 bytes of a step's output (4 float32 / 2 float64: one 128-bit store) -- they may span frames and rows, so
//   D = 3 and D = 17 stay on the wide path whenever num_envs is a multiple of 4 -- and walks a chunk of 16 steps; chunks are the grid's y axis.
//   (row, slot, column) of its elements cost two 32-bit divisions per chunk; per step the addresses move by additions, the row's two flag bytes
//   are read once per distinct row among the thread's elements, and a chunk looks back through the k - 1 (or `delay`) steps in front of it, and
//   the carried pending flag, for the resets its outputs can still see.  No LDS.  The first chunk's workgroups behind the stream write the new
//   state (Delay's history and count, the pending flags).  Where a step's block does not start on a 16-byte boundary (an odd num_envs) the
//   same kernel runs with one element per thread; where D is a multiple of 4 (2 for float64) a thread's elements are columns of one frame and
//   it takes one decision and one 128-bit load for them.
// time_steps_kernel (TimeAware over a rollout): the distance to the last reset is unbounded, so one thread per (row, output column) walks the T
//   steps with the row's counter in a register -- consecutive threads write consecutive elements, the flag bytes of a step are one coalesced
//   read shared by the row's threads -- and copies / widens its column of the trajectory in the same pass.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mi355env.h"
#include "stateful_observation_internal.h"

namespace mi_internal {
int set_error(int code, const char *msg);
}

namespace {

using namespace mi_stateful;

constexpr int kBlock = 256;

struct Args {
    int kind, dim, depth, padding, normalize_time, max_timesteps, next_step, same_step;
    int num_envs, steps, is_reset;
    const void *obs;
    void *out;
    const uint8_t *terminated, *truncated;
    const void *padding_value, *carried_in;
    void *carried_out;
    const int32_t *count_in;
    int32_t *count_out;
    const uint8_t *pending_in;
    uint8_t *pending_out;
    // one step
    const uint8_t *row_mask, *final_mask;
    const void *prev_out, *final_obs;
    void *final_out;
    // the rollout stream
    int32_t row;  // elements of one output row: k * D (FrameStack), D (Delay)
    int stream_blocks;
};

template <class T>
__device__ __forceinline__ T fetch(const Args &a, Slot s, const T *current, int64_t current_step_stride, int n, int d) {
    // one load whatever the source (a zero reads the row's own current element and drops it): an address select, no branch around the load
    const int D = a.dim;
    const int64_t here = (int64_t)n * D + d;
    const T *p = current + here;
    if (s.source == SRC_TRAJECTORY || s.source == SRC_RESET_OBS) p = current + (int64_t)s.index * current_step_stride + here;
    if (s.source == SRC_CARRIED) p = (const T *)a.carried_in + ((int64_t)n * a.depth + s.index) * D + d;
    if (s.source == SRC_CUSTOM) p = (const T *)a.padding_value + d;
    const T v = *p;
    return s.source == SRC_ZERO ? T(0) : v;
}

template <class Out>
__device__ __forceinline__ Out time_value(const Args &a, int time) {
    return a.normalize_time ? (Out)time_normalized(time, a.max_timesteps) : (Out)time;
}

// ---- one reset() / step() ----------------------------------------------------------------------------------------------------------------
// A row that is outside row_mask (a masked reset) keeps its state and returns prev_out.  Otherwise it resets (is_reset; NEXT_STEP: pending) or
// steps; under SAME_STEP a row of final_mask first takes final_obs as a step (final_out), then resets with obs.
template <class In, class Out>
__global__ __launch_bounds__(kBlock) void step_kernel(const Args a) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int D = a.dim, depth = a.depth;
    const In *obs = (const In *)a.obs, *fin = (const In *)a.final_obs;
    Out *out = (Out *)a.out, *final_out = (Out *)a.final_out;
    const Out *prev_out = (const Out *)a.prev_out;
    if (a.kind == MI_SO_TIME_AWARE) {
        const int W = D + 1;
        if (e >= (int64_t)a.num_envs * W) return;
        const int n = (int)(e / W), c = (int)(e - (int64_t)n * W);
        const bool keep = a.is_reset && a.row_mask && !a.row_mask[n];
        const bool pending = a.pending_in[n] != 0, finished = !a.is_reset && a.final_mask && a.final_mask[n];
        int time = a.count_in[n];
        if (final_out) final_out[e] = finished ? (c < D ? (Out)fin[(int64_t)n * D + c] : time_value<Out>(a, time + 1)) : Out(0);
        if (keep) {
            out[e] = prev_out ? prev_out[e] : Out(0);
        } else {
            time = time_after(time, a.is_reset || finished || (a.next_step && pending));
            out[e] = c < D ? (Out)obs[(int64_t)n * D + c] : time_value<Out>(a, time);
        }
        if (c == D) {
            a.count_out[n] = time;
            a.pending_out[n] = a.is_reset ? (keep ? a.pending_in[n] : 0) : (a.same_step ? 0 : (a.terminated[n] | a.truncated[n]) != 0);
        }
        return;
    }
    // FrameStack: e over [N][k][D], the output; Delay: e over [N][max(delay, 1)][D], the new history, whose slot 0 also writes the output
    const int J = a.kind == MI_SO_FRAME_STACK ? depth : (depth > 0 ? depth : 1);
    if (e >= (int64_t)a.num_envs * J * D) return;
    const int n = (int)(e / ((int64_t)J * D)), rem = (int)(e - (int64_t)n * J * D), j = rem / D, d = rem - j * D;
    const bool keep = a.is_reset && a.row_mask && !a.row_mask[n];
    const bool pending = a.pending_in[n] != 0, finished = !a.is_reset && a.final_mask && a.final_mask[n];
    const bool resets = a.is_reset || finished || (a.next_step && pending);
    if (j == 0 && d == 0) a.pending_out[n] = a.is_reset ? (keep ? a.pending_in[n] : 0) : (a.same_step ? 0 : (a.terminated[n] | a.truncated[n]) != 0);
    if (a.kind == MI_SO_FRAME_STACK) {
        if (final_out) final_out[e] = finished ? (Out)fetch<In>(a, frame_stack_slot(depth, a.padding, 0, j, -1), fin, 0, n, d) : Out(0);
        if (keep)
            out[e] = prev_out ? prev_out[e] : Out(0);
        else
            out[e] = (Out)fetch<In>(a, frame_stack_slot(depth, a.padding, 0, j, resets ? 0 : -1), obs, 0, n, d);
        return;
    }
    const int count = a.count_in[n];
    const int64_t o = (int64_t)n * D + d;
    if (j == 0) {
        if (final_out) final_out[o] = finished ? (Out)fetch<In>(a, delay_slot(depth, 0, -1, count), fin, 0, n, d) : Out(0);
        if (keep)
            out[o] = prev_out ? prev_out[o] : Out(0);
        else
            out[o] = (Out)fetch<In>(a, delay_slot(depth, 0, resets && depth > 0 ? 0 : -1, count), obs, 0, n, d);
        if (d == 0) a.count_out[n] = keep ? count : delay_count(depth, 1, resets && depth > 0 ? 0 : -1, count);
    }
    if (depth > 0) {
        In *history = (In *)a.carried_out;
        history[e] = keep ? ((const In *)a.carried_in)[e] : fetch<In>(a, delay_history_slot(depth, 1, j), obs, 0, n, d);
    }
}

// ---- FrameStack / Delay over a rollout -----------------------------------------------------------------------------------------------------
// A thread owns V consecutive elements of a step's output -- the same (row, slot, column) in every step -- and walks a chunk of kChunk steps; the
// grid's y axis is the chunk.  Everything that depends on the element is computed once per chunk, and so are the flags: the chunk's 16 pairs of flag
// bytes (once per distinct row among the thread's elements) become a bit mask before the walk begins, and a chunk that does not start the rollout
// looks back through the depth - 1 (or delay) steps in front of it, the only ones that can still reach its outputs.  The walk itself keeps the row's
// latest reset in a register, takes each element's source from the header's decision, moves its addresses by additions and stores the V elements
// with one store; no load of a step depends on another load, so the loads of several steps are in flight together (the loop is unrolled by 4).
constexpr int kChunk = 16, kNever = -1, kDelayMode = 3;

template <class T, int V>
struct alignas(sizeof(T) * V) Vec {
    T v[V];
};

// MODE: the padding of a FrameStack (PAD_RESET / PAD_ZERO / PAD_CUSTOM) or kDelayMode -- compiled in, so that the walk has no branch in it
// UNIFORM: dim is a multiple of V and every block is 16-byte aligned, so a thread's V elements are columns of one frame
template <class T, int V, int MODE, bool UNIFORM>
__global__ __launch_bounds__(kBlock) void stack_steps_kernel(const Args a) {
    const int N = a.num_envs, D = a.dim, depth = a.depth, row = a.row, T_ = a.steps;
    const uint8_t *__restrict__ te = a.terminated;
    const uint8_t *__restrict__ tr = a.truncated;
    const T *__restrict__ obs = (const T *)a.obs;
    if ((int)blockIdx.x >= a.stream_blocks) {  // the new state (the first chunk's workgroups behind the stream)
        if (blockIdx.y != 0) return;
        const int64_t e = (int64_t)((int)blockIdx.x - a.stream_blocks) * kBlock + threadIdx.x;
        const int J = a.kind == MI_SO_DELAY && depth > 0 ? depth : 1;
        const int width = a.kind == MI_SO_DELAY && depth > 0 ? D : 1;  // (FrameStack: the new state is the last stack of the output, nothing to copy)
        if (e >= (int64_t)N * J * width) return;
        const int n = (int)(e / ((int64_t)J * width)), rem = (int)(e - (int64_t)n * J * width), j = rem / width, d = rem - j * width;
        if (j == 0 && d == 0) {
            a.pending_out[n] = (te[(int64_t)(T_ - 1) * N + n] | tr[(int64_t)(T_ - 1) * N + n]) != 0;
            if (a.kind == MI_SO_DELAY) {
                const int r = latest_reset(T_ - depth + 1, T_ - 1, a.next_step != 0, a.pending_in[n] != 0,
                                           [=](int s) { return (te[(int64_t)s * N + n] | tr[(int64_t)s * N + n]) != 0; });
                a.count_out[n] = delay_count(depth, T_, r, a.count_in[n]);
            }
        }
        if (a.kind == MI_SO_DELAY && depth > 0) ((T *)a.carried_out)[e] = fetch<T>(a, delay_history_slot(depth, T_, j), obs, (int64_t)N * D, n, d);
        return;
    }
    const int per_step = N * row;  // (below 2^31: the launcher's business)
    const int64_t first = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * V;
    if (first >= per_step) return;
    constexpr bool frames = MODE != kDelayMode;
    constexpr int padding = frames ? MODE : PAD_ZERO;
    const int t0 = (int)blockIdx.y * kChunk, t1 = t0 + kChunk < T_ ? t0 + kChunk : T_;
    const int64_t ND = (int64_t)N * D;
    const T *__restrict__ carried = (const T *)a.carried_in;
    const T *__restrict__ custom = (const T *)a.padding_value;
    T *__restrict__ out = (T *)a.out;
    // per element, for the whole chunk: its row, slot and column; where its sources lie relative to the current step; the row's resets
    int j[V], d[V], count[V], last[V];
    uint32_t resets[V];  // bit b: the row resets at step t0 + b
    int64_t here[V], behind[V], carried_at[V], reset_at[V];
    int before = -1;
#pragma unroll
    for (int i = 0; i < V; i++) {
        const int w = (int)first + i, n = w / row, rem = w - n * row;
        j[i] = frames ? rem / D : 0;
        d[i] = rem - j[i] * D;
        here[i] = (int64_t)n * D + d[i];                                          // this element in the step's input block
        behind[i] = here[i] - (int64_t)(frames ? depth - 1 - j[i] : depth) * ND;  // ... and in the block of its source step, relative to the current one
        carried_at[i] = (int64_t)n * depth * D + d[i];                            // slot 0 of the row's carried state
        count[i] = frames ? 0 : a.count_in[n];
        last[i] = kNever, resets[i] = 0;
        if (n == before) {
            last[i] = last[i - (i > 0)], resets[i] = resets[i - (i > 0)];
        } else if (a.next_step) {
            const bool pending = a.pending_in[n] != 0;
            // the resets in front of the chunk that its outputs can still see ...
            last[i] = latest_reset(t0 - (frames ? depth - 1 : depth) + 1, t0 - 1, true, pending, [=](int s) { return (te[(int64_t)s * N + n] | tr[(int64_t)s * N + n]) != 0; });
            // ... and the chunk's own, all read before the walk begins: no step waits for its flags
            uint32_t bits = 0;
#pragma unroll
            for (int b = 0; b < kChunk; b++) {
                const int t = t0 + b < T_ ? t0 + b : T_;  // (the steps behind the rollout's end repeat its last flags: their bits are never read)
                const int64_t at = (int64_t)(t > 0 ? t - 1 : 0) * N + n;
                const bool finished = (te[at] | tr[at]) != 0;
                bits |= (uint32_t)(t == 0 ? pending : finished) << b;
            }
            resets[i] = bits;
        }
        before = n;
        reset_at[i] = (int64_t)(last[i] >= 0 ? last[i] : 0) * ND + here[i];
    }
    int64_t current = (int64_t)t0 * ND, out_at = (int64_t)t0 * per_step + first;
#pragma unroll 4
    for (int t = t0; t < t1; t++, current += ND, out_at += per_step) {
        Vec<T, V> y;
        if constexpr (UNIFORM) {  // the thread's elements are V columns of ONE frame: one decision, one 128-bit load
            const bool now = (resets[0] >> (t - t0)) & 1;
            last[0] = now ? t : last[0];
            reset_at[0] = now ? current + here[0] : reset_at[0];
            const Slot s = frames ? frame_stack_slot(depth, padding, t, j[0], last[0]) : delay_slot(depth, t, last[0] > t - depth ? last[0] : -1, count[0]);
            const T *p = obs + current + here[0];
            if (s.source == SRC_TRAJECTORY) p = obs + current + behind[0];
            if (s.source == SRC_RESET_OBS) p = obs + reset_at[0];
            if (s.source == SRC_CARRIED) p = carried + carried_at[0] + s.index * D;
            if (s.source == SRC_CUSTOM) p = custom + d[0];
            const Vec<T, V> v = *reinterpret_cast<const Vec<T, V> *>(p);
#pragma unroll
            for (int i = 0; i < V; i++) y.v[i] = s.source == SRC_ZERO ? T(0) : v.v[i];
            *reinterpret_cast<Vec<T, V> *>(out + out_at) = y;
            continue;
        }
#pragma unroll
        for (int i = 0; i < V; i++) {
            const bool now = (resets[i] >> (t - t0)) & 1;
            last[i] = now ? t : last[i];
            reset_at[i] = now ? current + here[i] : reset_at[i];
            const Slot s = frames ? frame_stack_slot(depth, padding, t, j[i], last[i]) : delay_slot(depth, t, last[i] > t - depth ? last[i] : -1, count[i]);
            // one load whatever the source (a zero reads the element's own current value and drops it); the source steps are known relative to t
            const T *p = obs + current + here[i];
            if (s.source == SRC_TRAJECTORY) p = obs + current + behind[i];
            if (s.source == SRC_RESET_OBS) p = obs + reset_at[i];
            if (s.source == SRC_CARRIED) p = carried + carried_at[i] + s.index * D;
            if (s.source == SRC_CUSTOM) p = custom + d[i];
            const T v = *p;
            y.v[i] = s.source == SRC_ZERO ? T(0) : v;
        }
        *reinterpret_cast<Vec<T, V> *>(out + out_at) = y;
    }
}

// ---- TimeAware over a rollout ----------------------------------------------------------------------------------------------------------------
template <class In, class Out>
__global__ __launch_bounds__(kBlock) void time_steps_kernel(const Args a) {
    const int D = a.dim, W = D + 1, N = a.num_envs;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x, per_step = (int64_t)N * W;
    if (e >= per_step) return;
    const int n = (int)(e / W), c = (int)(e - (int64_t)n * W);
    const In *in = (const In *)a.obs + (int64_t)n * D + (c < D ? c : 0);
    Out *out = (Out *)a.out + e;
    int time = a.count_in[n];
    bool pending = a.pending_in[n] != 0;
#pragma unroll 4
    for (int t = 0; t < a.steps; t++) {
        time = time_after(time, a.next_step && pending);
        pending = (a.terminated[(int64_t)t * N + n] | a.truncated[(int64_t)t * N + n]) != 0;
        out[(int64_t)t * per_step] = c < D ? (Out)in[(int64_t)t * N * D] : time_value<Out>(a, time);
    }
    if (c == D) a.count_out[n] = time, a.pending_out[n] = pending ? 1 : 0;
}

int invalid(const char *msg) { return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, msg); }

int dtype_size(int dtype) { return dtype == MI_F32 || dtype == MI_I32 ? 4 : (dtype == MI_F64 ? 8 : 0); }

// what both entry points check and copy; 0 or an mi_status
int fill(Args &a, const mi_stateful_observation_state *s, int num_envs, const void *obs, void *out, const char *who) {
    char buf[320];
    a = Args{};
    if (!s || num_envs < 1 || !out || !s->pending_in || !s->pending_out || s->autoreset_mode < MI_AUTORESET_NEXT_STEP ||
        s->autoreset_mode > MI_AUTORESET_DISABLED || (s->in_dtype != MI_F32 && s->in_dtype != MI_F64) || s->dim < 0) {
        snprintf(buf, sizeof buf, "%s: needs a state with pending_in / pending_out, an autoreset mode and in_dtype MI_F32 / MI_F64, num_envs >= 1 and out", who);
        return invalid(buf);
    }
    bool ok = false;
    switch (s->kind) {
    case MI_SO_FRAME_STACK:
        ok = s->depth >= 1 && s->dim >= 1 && obs && s->carried_in && s->out_dtype == s->in_dtype && s->padding >= PAD_RESET && s->padding <= PAD_CUSTOM &&
             (s->padding != PAD_CUSTOM || s->padding_value);
        break;
    case MI_SO_DELAY:
        ok = s->depth >= 0 && s->dim >= 1 && obs && s->out_dtype == s->in_dtype && s->count_in && s->count_out &&
             (s->depth == 0 || (s->carried_in && s->carried_out));
        break;
    case MI_SO_TIME_AWARE:
        ok = s->count_in && s->count_out && (s->dim == 0 || obs) && (!s->normalize_time || s->max_timesteps >= 1) &&
             (s->out_dtype == MI_F64 || (s->out_dtype == MI_F32 && s->in_dtype == MI_F32 && (s->normalize_time || s->dim == 0)) ||
              (s->out_dtype == MI_I32 && s->dim == 0 && !s->normalize_time));
        break;
    }
    if (!ok) {
        snprintf(buf, sizeof buf, "%s: kind %d with depth %d, dim %d, dtypes %d -> %d, padding %d: a member of the state is missing or out of range "
                                  "(include/mi355env.h, mi_stateful_observation_state)", who, s->kind, s->depth, s->dim, s->in_dtype, s->out_dtype, s->padding);
        return invalid(buf);
    }
    const int64_t per_row = s->kind == MI_SO_TIME_AWARE ? (int64_t)s->dim + 1 : (int64_t)s->dim * (s->depth > 0 ? s->depth : 1);
    if ((int64_t)num_envs * per_row >= ((int64_t)1 << 31)) {
        snprintf(buf, sizeof buf, "%s: the elements of one step (num_envs * stack_size * dim) must stay below 2^31", who);
        return invalid(buf);
    }
    const uintptr_t in_size = (uintptr_t)dtype_size(s->in_dtype), out_size = (uintptr_t)dtype_size(s->out_dtype);
    if ((uintptr_t)obs % in_size || (uintptr_t)out % out_size || (uintptr_t)s->carried_in % in_size || (uintptr_t)s->carried_out % in_size ||
        (uintptr_t)s->padding_value % in_size || (uintptr_t)s->count_in % 4 || (uintptr_t)s->count_out % 4) {
        snprintf(buf, sizeof buf, "%s: a pointer is not aligned to its element type", who);
        return invalid(buf);
    }
    a.kind = s->kind, a.dim = s->dim, a.depth = s->depth, a.padding = s->padding, a.normalize_time = s->normalize_time, a.max_timesteps = s->max_timesteps;
    a.next_step = s->autoreset_mode == MI_AUTORESET_NEXT_STEP, a.same_step = s->autoreset_mode == MI_AUTORESET_SAME_STEP;
    a.num_envs = num_envs, a.obs = obs, a.out = out;
    a.padding_value = s->padding_value, a.carried_in = s->carried_in, a.carried_out = s->carried_out;
    a.count_in = s->count_in, a.count_out = s->count_out, a.pending_in = s->pending_in, a.pending_out = s->pending_out;
    return MI_OK;
}

template <class In, class Out>
void launch_step_or_time(bool trajectory, hipStream_t st, unsigned blocks, const Args &a) {
    if (trajectory)
        hipLaunchKernelGGL((time_steps_kernel<In, Out>), dim3(blocks), dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL((step_kernel<In, Out>), dim3(blocks), dim3(kBlock), 0, st, a);
}

template <class T, int MODE>
void launch_stream_mode(hipStream_t st, dim3 grid, bool wide, const Args &a) {
    constexpr int V = 16 / sizeof(T);
    const uintptr_t every = (uintptr_t)a.obs | (uintptr_t)a.carried_in | (uintptr_t)a.padding_value;
    if (wide && a.dim % V == 0 && every % 16 == 0)
        hipLaunchKernelGGL((stack_steps_kernel<T, V, MODE, true>), grid, dim3(kBlock), 0, st, a);
    else if (wide)
        hipLaunchKernelGGL((stack_steps_kernel<T, V, MODE, false>), grid, dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL((stack_steps_kernel<T, 1, MODE, false>), grid, dim3(kBlock), 0, st, a);
}

template <class T>
void launch_stream(hipStream_t st, dim3 grid, bool wide, const Args &a) {
    if (a.kind == MI_SO_DELAY)
        launch_stream_mode<T, kDelayMode>(st, grid, wide, a);
    else if (a.padding == PAD_RESET)
        launch_stream_mode<T, PAD_RESET>(st, grid, wide, a);
    else if (a.padding == PAD_ZERO)
        launch_stream_mode<T, PAD_ZERO>(st, grid, wide, a);
    else
        launch_stream_mode<T, PAD_CUSTOM>(st, grid, wide, a);
}

// wide: the rollout stream of FrameStack / Delay with 128-bit stores
int enqueue(bool trajectory, int device, void *hip_stream, dim3 grid, bool wide, const Args &a, const mi_stateful_observation_state *s, const char *who) {
    hipStream_t st = (hipStream_t)hip_stream;
    const unsigned blocks = grid.x;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) {
        if (trajectory && s->kind != MI_SO_TIME_AWARE) {
            if (s->in_dtype == MI_F32)
                launch_stream<float>(st, grid, wide, a);
            else
                launch_stream<double>(st, grid, wide, a);
        } else if (s->in_dtype == MI_F64) {
            launch_step_or_time<double, double>(trajectory, st, blocks, a);
        } else if (s->out_dtype == MI_F64) {
            launch_step_or_time<float, double>(trajectory, st, blocks, a);
        } else if (s->out_dtype == MI_I32) {
            launch_step_or_time<float, int32_t>(trajectory, st, blocks, a);
        } else {
            launch_step_or_time<float, float>(trajectory, st, blocks, a);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) return MI_OK;
    char buf[300];
    snprintf(buf, sizeof buf, "%s failed: %s", who, hipGetErrorString(e));
    return mi_internal::set_error(MI_ERR_HIP, buf);
}

}  // namespace

#pragma GCC visibility push(default)

int mi_stateful_observation_step(int device, void *hip_stream, const mi_stateful_observation_state *state, int num_envs, int is_reset, const void *obs,
                                 void *out, const uint8_t *row_mask, const void *prev_out, const void *final_obs, void *final_out,
                                 const uint8_t *final_mask, const uint8_t *terminated, const uint8_t *truncated) {
    const char *who = "mi_stateful_observation_step";
    Args a;
    const int rc = fill(a, state, num_envs, obs, out, who);
    if (rc != MI_OK) return rc;
    const bool any_final = final_obs || final_out || final_mask;
    const bool all_final = final_out && final_mask && (final_obs || (state->kind == MI_SO_TIME_AWARE && state->dim == 0));
    if (any_final && (!all_final || is_reset)) return invalid("mi_stateful_observation_step: final_obs, final_out and final_mask come together, in a step");
    if (!is_reset && (row_mask || prev_out)) return invalid("mi_stateful_observation_step: row_mask / prev_out belong to a reset");
    if (!is_reset && state->autoreset_mode != MI_AUTORESET_SAME_STEP && (!terminated || !truncated))
        return invalid("mi_stateful_observation_step: a step under NEXT_STEP / DISABLED needs terminated and truncated");
    const uintptr_t in_size = (uintptr_t)dtype_size(state->in_dtype), out_size = (uintptr_t)dtype_size(state->out_dtype);
    if ((uintptr_t)final_obs % in_size || (uintptr_t)final_out % out_size || (uintptr_t)prev_out % out_size)
        return invalid("mi_stateful_observation_step: final_obs / final_out / prev_out are not aligned to their element types");
    a.is_reset = is_reset != 0, a.steps = 1;
    a.row_mask = row_mask, a.prev_out = prev_out, a.final_obs = final_obs, a.final_out = final_out, a.final_mask = final_mask;
    a.terminated = terminated, a.truncated = truncated;
    const int64_t per_row = state->kind == MI_SO_TIME_AWARE ? (int64_t)state->dim + 1 : (int64_t)state->dim * (state->depth > 0 ? state->depth : 1);
    const int64_t work = (int64_t)num_envs * per_row;
    return enqueue(false, device, hip_stream, dim3((unsigned)((work + kBlock - 1) / kBlock)), false, a, state, who);
}

int mi_stateful_observation_steps(int device, void *hip_stream, const mi_stateful_observation_state *state, int T, int num_envs, const void *obs,
                                  void *out, const uint8_t *terminated, const uint8_t *truncated) {
    const char *who = "mi_stateful_observation_steps";
    Args a;
    const int rc = fill(a, state, num_envs, obs, out, who);
    if (rc != MI_OK) return rc;
    if (T < 1 || !terminated || !truncated) return invalid("mi_stateful_observation_steps: needs T >= 1, terminated and truncated");
    if (state->autoreset_mode == MI_AUTORESET_SAME_STEP)
        return mi_internal::set_error(MI_ERR_UNSUPPORTED, "mi_stateful_observation_steps: under SAME_STEP a row that finishes returns its reset observation and "
                                                          "its final one in the same step; run the steps through mi_stateful_observation_step");
    a.steps = T, a.terminated = terminated, a.truncated = truncated;
    if (state->kind == MI_SO_TIME_AWARE) {
        const int64_t work = (int64_t)num_envs * (state->dim + 1);
        return enqueue(true, device, hip_stream, dim3((unsigned)((work + kBlock - 1) / kBlock)), false, a, state, who);
    }
    // the stream: V elements per thread and step where every step's block starts on a 16-byte boundary (num_envs a multiple of 4 is enough,
    // whatever the row width), one element per thread otherwise -- still coalesced, a quarter of the width
    const int64_t size = dtype_size(state->in_dtype), V = 16 / size;
    a.row = state->kind == MI_SO_FRAME_STACK ? state->depth * state->dim : state->dim;
    const int64_t per_step = (int64_t)num_envs * a.row;
    const bool wide = (uintptr_t)out % 16 == 0 && per_step % V == 0;
    const int64_t threads = wide ? per_step / V : per_step, chunks = ((int64_t)T + kChunk - 1) / kChunk;
    if (chunks > 65535) return invalid("mi_stateful_observation_steps: at most 65535 * 16 steps per call");
    a.stream_blocks = (int)((threads + kBlock - 1) / kBlock);
    const int64_t state_work = state->kind == MI_SO_DELAY && state->depth > 0 ? (int64_t)num_envs * state->depth * state->dim : num_envs;
    return enqueue(true, device, hip_stream, dim3((unsigned)(a.stream_blocks + (state_work + kBlock - 1) / kBlock), (unsigned)chunks), wide, a, state, who);
}

#pragma GCC visibility pop
