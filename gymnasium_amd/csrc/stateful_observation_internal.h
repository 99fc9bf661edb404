// stateful_observation_internal.h -- the index arithmetic of FrameStackObservation / DelayObservation / TimeAwareObservation around every scalar env
// (csrc/stateful_observation.hip).  The wrappers only MOVE data (plus one exact division for the normalised time), so everything that can go wrong
// is a decision: which source step feeds an output element, whether the element is padding, carried state or a trajectory element, and the time
// value.  Those decisions are written here, once, for the step launch and the rollout launch alike, and compile for the host
// (tests/test_stateful_observation_host.py builds a stand-alone program from this header and compares it with the NumPy restatement).
//
// Conventions.  A launch covers steps t = 0 .. T-1 of one row (a step() or a reset() is T = 1).  The row RESETS at step s when its scalar env's
// reset() produced the observation of that step: reset() itself, a masked reset, the NEXT_STEP autoreset step (the row finished in step s - 1, or,
// for s = 0, before the launch: the carried `pending` flag), the SAME_STEP reset.  `r` below is the LATEST step <= t at which the row resets inside
// the window an output looks back through, or -1: a reset further back cannot reach the output.
#ifndef MI_STATEFUL_OBSERVATION_INTERNAL_H
#define MI_STATEFUL_OBSERVATION_INTERNAL_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MI_SO_HD __host__ __device__ inline
#define MI_SO_UNROLL _Pragma("unroll 4")
#else
#define MI_SO_HD inline
#define MI_SO_UNROLL
#endif

namespace mi_stateful {

enum Source : int32_t {
    SRC_TRAJECTORY = 0,  // index: the step of the launch whose observation is taken
    SRC_CARRIED = 1,     // index: the slot of the carried state (FrameStack: the last output [k][D]; Delay: the history [delay][D])
    SRC_RESET_OBS = 2,   // padding_type="reset": the reset observation, i.e. the trajectory at step `index`
    SRC_ZERO = 3,        // padding_type="zero", an empty or part-filled delay queue
    SRC_CUSTOM = 4       // the custom padding observation
};
enum Padding : int32_t { PAD_RESET = 0, PAD_ZERO = 1, PAD_CUSTOM = 2 };

struct Slot {
    int32_t source, index;
};

// The latest s in [max(lo, 0), t] at which the row resets, or -1.  done(s): the row finished (terminated | truncated) in step s of the launch.
// Only NEXT_STEP resets rows inside a launch of several steps; a single step passes its own decision as `pending`.
// Written without an early exit, ascending so that the latest reset wins: the flag reads of a window do not depend on one another, and on the
// device they are all in flight together instead of one round trip to memory per step looked back.
template <class Done>
MI_SO_HD int latest_reset(int lo, int t, bool next_step, bool pending, Done done) {
    if (!next_step || t < 0) return -1;
    int r = lo <= 0 && pending ? 0 : -1;
    MI_SO_UNROLL
    for (int s = lo > 1 ? lo : 1; s <= t; s++) r = done(s - 1) ? s : r;
    return r;
}

// FrameStackObservation (stateful_observation.py:419-461): slot j of the stack returned at step t holds the observation of step t - (k - 1 - j),
// unless the row reset after that step: then it is the padding of that reset.  r = latest_reset(t - (k - 1), t).
MI_SO_HD Slot frame_stack_slot(int k, int padding, int t, int j, int r) {
    const int s = t - (k - 1 - j);
    if (r >= 0 && s < r) return padding == PAD_RESET ? Slot{SRC_RESET_OBS, r} : Slot{padding == PAD_ZERO ? SRC_ZERO : SRC_CUSTOM, 0};
    if (s >= 0) return Slot{SRC_TRAJECTORY, s};
    return Slot{SRC_CARRIED, k + s};  // the last output held steps -k .. -1 in slots 0 .. k-1 (with their own padding)
}

// DelayObservation (stateful_observation.py:88-103): the observation of step t - delay once the queue, emptied by every reset, holds more than
// `delay` entries.  r = latest_reset(t - delay + 1, t): a reset after the source step means the queue is still filling.  carried_count: how many
// of the `delay` history slots (the LAST ones) were valid before the launch.
MI_SO_HD Slot delay_slot(int delay, int t, int r, int carried_count) {
    if (r >= 0) return Slot{SRC_ZERO, 0};
    const int s = t - delay;
    if (s >= 0) return Slot{SRC_TRAJECTORY, s};
    return -s <= carried_count ? Slot{SRC_CARRIED, delay + s} : Slot{SRC_ZERO, 0};
}

// The history after a launch of T steps: slot j holds step T - delay + j ...
MI_SO_HD Slot delay_history_slot(int delay, int T, int j) {
    const int s = T - delay + j;
    return s >= 0 ? Slot{SRC_TRAJECTORY, s} : Slot{SRC_CARRIED, delay + s};
}
// ... and the number of valid slots.  r = latest_reset(T - delay + 1, T - 1): with a reset at r the queue holds steps r .. T-1.
MI_SO_HD int delay_count(int delay, int T, int r, int carried_count) {
    if (r >= 0) return T - r;
    const int64_t n = (int64_t)carried_count + T;
    return n < delay ? (int)n : delay;
}

// TimeAwareObservation (stateful_observation.py:272-301): every reset zeroes the row's counter, every step increments it first.
MI_SO_HD int time_after(int time, bool resets) { return resets ? 0 : time + 1; }
// normalize_time=True: np.array([t / max_timesteps], dtype=np.float32) -- Python's true division (the float64 quotient, correctly rounded: both
// integers are far below 2^53), rounded once more to float32.
MI_SO_HD float time_normalized(int time, int max_timesteps) { return (float)((double)time / (double)max_timesteps); }

}  // namespace mi_stateful

#endif
