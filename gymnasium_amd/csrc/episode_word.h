// episode_word.h -- the env role's episode bookkeeping of the two-role rollout (classic_kernels.h duo_env_step) in ONE 32-bit word per lane:
//   bit 31       the sub-environment finished an episode and its next step is the autoreset step (kNeedsReset of the lane's flag word)
//   bits 1 .. 30 TimeLimit's elapsed steps (the 30 bits `meta` keeps)
//   bit 0        the lane's reset queue holds draws (ResetQueue::have)
// so that every test of the step is one compare of the word and the update one add, one or and one select.  The flag word's other bits do not change
// during a launch and rejoin when `meta` is stored.  Plain integer functions: the header also compiles for the host (tests/test_episode_word.py
// drives it through tests/episode_word_host/harness.cpp against duo_env_step's three-register logic written out in Python).
#ifndef MI355ENV_EPISODE_WORD_H
#define MI355ENV_EPISODE_WORD_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MI_EW_FN __host__ __device__ __forceinline__
#else
#define MI_EW_FN inline
#endif

namespace mi_episode_word {

constexpr uint32_t kPending = 0x80000000u, kHave = 1u;
constexpr uint32_t kMetaFlagShift = 30, kMetaElapsedMask = (1u << kMetaFlagShift) - 1u, kMetaNeedsReset = 1u;  // engine_types.h, envs_classic.h (asserted equal in classic_kernels.h)

// from `meta` (elapsed | flags << 30) and the queue's state
MI_EW_FN uint32_t encode(uint32_t meta, uint32_t have) {
    return (((meta >> kMetaFlagShift) & kMetaNeedsReset) ? kPending : 0u) | ((meta & kMetaElapsedMask) << 1) | (have ? kHave : 0u);
}
// `meta` again; `other_flags`: the flag word's bits besides kNeedsReset, as the launch found them
MI_EW_FN uint32_t decode_meta(uint32_t w, uint32_t other_flags) {
    return ((w >> 1) & kMetaElapsedMask) | (((other_flags & ~kMetaNeedsReset) | (w >> 31)) << kMetaFlagShift);
}
MI_EW_FN uint32_t have(uint32_t w) { return w & kHave; }
MI_EW_FN uint32_t with_have(uint32_t w) { return w | kHave; }  // after ResetQueue::refill

// the "never" threshold of a TimeLimit that is off: no word reaches it (elapsed < 2^30 - 1)
MI_EW_FN int32_t truncation_threshold(int max_steps) { return max_steps > 0 ? (int32_t)(2u * (uint32_t)(max_steps < (1 << 30) ? max_steps : (1 << 30) - 1)) : INT32_MAX; }

// the four predicates of a step that starts from `w`
MI_EW_FN bool resetting(uint32_t w) { return (int32_t)w < 0; }                                          // this step is the autoreset step
MI_EW_FN bool refill(uint32_t w) { return (w & (kPending | kHave)) == kPending; }                       // ... and its queue is empty
MI_EW_FN bool truncated(uint32_t w, int32_t threshold) { return (int32_t)(w + 2u) >= threshold; }       // TimeLimit raises truncated (never in an autoreset step: the word is negative)
MI_EW_FN bool done(uint32_t w, bool terminated, int32_t threshold) { return !resetting(w) && (terminated || truncated(w, threshold)); }

// the word after the step: an autoreset step leaves elapsed 0, nothing pending and an empty queue; any other step counts and raises pending when
// the episode ended.  `terminated` is the env's own test of the stepped state (of no consequence in an autoreset step).
MI_EW_FN uint32_t advance(uint32_t w, bool ended) { return resetting(w) ? 0u : ((w + 2u) | (ended ? kPending : 0u)); }  // ended: terminated || truncated(w, threshold)
MI_EW_FN uint32_t step(uint32_t w, bool terminated, int32_t threshold) { return advance(w, terminated || truncated(w, threshold)); }

// What the env role hands the aux role when the latter masks the flags itself (E::DUO_RAW_FLAGS): terminated | truncated << 1 as the step raised them ...
MI_EW_FN uint32_t flag_bits(bool terminated, bool truncated) { return (terminated ? 1u : 0u) | (truncated ? 2u : 0u); }
MI_EW_FN uint32_t raw_flags(uint32_t w, bool terminated, int32_t threshold) { return flag_bits(terminated, truncated(w, threshold)); }
// ... and the aux role's side: `pending` is nonzero when this step is the autoreset step, whose flags are all clear; the result is both the step's flags
// (1 terminated, 2 truncated) and, as zero / nonzero, the next step's `pending`
MI_EW_FN uint32_t effective_flags(uint32_t pending, uint32_t raw) { return pending ? 0u : raw; }

}  // namespace mi_episode_word
#endif
