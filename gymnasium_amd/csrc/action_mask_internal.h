// action_mask_internal.h -- what action_mask.hip (the kernels of `action_space.sample(mask=...)` / `sample(probability=...)` on the action stream)
// and engine.hip (mi_action_sample_masked / _weighted / _get_buffered / _set_buffered, which own the buffers) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcg64_dev.h"

namespace mi_actmask {

constexpr int kMaxMaskActions = 64;     // a mask row is held as one 64-bit word
constexpr int kMaxWeightedActions = 7;  // np.sum is the plain left-to-right sum up to here (pairwise from 8 elements on)
constexpr int kErrInvalidSampleArg = 3; // the sticky device error word: a batch of masks / probabilities was refused

// The part of the action stream's position that lives in device memory besides the per-lane states: the pending 32-bit half of NumPy's PCG64
// (`has_uint32` / `uinteger` of bit_generator.state -- only 32-bit draws use or change it), and the scratch words of the batch in flight.
struct Ctl {
    uint64_t base_hi, base_lo;  // the generator's state before the batch's first draw (scan kernel: lane 0's state stepped back once)
    uint32_t has_uint32, uinteger;
    uint32_t bad;      // this batch has an invalid row: nothing is written, nothing moves
    uint32_t first;    // masked: the first row whose bounded draw was rejected (>= N: none)
    uint32_t total;    // masked: 32-bit values the batch consumes when no draw is rejected
    uint32_t outputs;  // masked: 64-bit outputs the batch took from the generator (repair kernel)
};

struct Work {
    Ctl *ctl;                // device
    uint32_t *partial;       // [ceil(N / 256)] device: per-workgroup counts, then their exclusive prefix
    uint32_t *slot;          // [N] device: a row's 32-bit slot in the batch (masked) / its action before the batch is known to be valid (weighted)
    uint64_t *lane;          // [2][N] device: the per-lane states of the action stream (engine.hip act_init_kernel)
    const mi::PcgJump *pow2; // [64] device: jump by 2^j draws
    mi::PcgJump jump_n;      // jump by N draws
    uint64_t inc_hi, inc_lo; // the generator's increment
    int *error;              // the sticky error word (device address of page-locked host memory)
    int N, A;
    int force_repair;        // MI355ENV_MASKED_FORCE_REPAIR=1: every masked batch is recomputed by the repair stage
    hipStream_t stream;
};

// Enqueue only: no allocation, no synchronisation.  mask [N][A] int8, prob [N][A] float64, out [N] int64 -- device pointers.
hipError_t sample_masked(const Work &w, const int8_t *mask, int64_t *out);
hipError_t sample_weighted(const Work &w, const double *prob, int64_t *out);
hipError_t set_buffered(const Work &w, uint32_t has_uint32, uint32_t uinteger);

}  // namespace mi_actmask
