// TEST INFRASTRUCTURE: gymnasium_amd/csrc/episode_word.h compiled for the host, driven by tests/test_episode_word.py.
#include "../../gymnasium_amd/csrc/episode_word.h"

namespace W = mi_episode_word;
#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT uint32_t ew_encode(uint32_t meta, uint32_t have) { return W::encode(meta, have); }
EXPORT uint32_t ew_decode_meta(uint32_t w, uint32_t other_flags) { return W::decode_meta(w, other_flags); }
EXPORT uint32_t ew_have(uint32_t w) { return W::have(w); }
EXPORT uint32_t ew_with_have(uint32_t w) { return W::with_have(w); }
EXPORT int32_t ew_threshold(int max_steps) { return W::truncation_threshold(max_steps); }
EXPORT uint32_t ew_raw_flags(uint32_t w, int terminated, int max_steps) { return W::raw_flags(w, terminated != 0, W::truncation_threshold(max_steps)); }
EXPORT uint32_t ew_effective_flags(uint32_t pending, uint32_t raw) { return W::effective_flags(pending, raw); }
// one step from `w`, for n cases at once: the four predicates (bit 0 resetting, 1 refill, 2 truncated, 3 done) and the word after the step
EXPORT void ew_step_batch(const uint32_t *w, const uint8_t *terminated, const int32_t *max_steps, uint32_t *predicates, uint32_t *next, long n) {
    for (long i = 0; i < n; i++) {
        const int32_t thr = W::truncation_threshold(max_steps[i]);
        const bool te = terminated[i] != 0;
        predicates[i] = (W::resetting(w[i]) ? 1u : 0u) | (W::refill(w[i]) ? 2u : 0u) | (W::truncated(w[i], thr) ? 4u : 0u) | (W::done(w[i], te, thr) ? 8u : 0u);
        next[i] = W::step(w[i], te, thr);
    }
}
