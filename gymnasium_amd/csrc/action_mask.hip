// action_mask.hip -- `action_space.sample(mask=...)` and `sample(probability=...)` of the batched Discrete space on the engine's action stream
// (mi_action_sample_masked / mi_action_sample_weighted, include/mi355env.h).
//
// Reference behaviour reproduced (spaces/multi_discrete.py:180-249 `_apply_mask`, one generator, rows in index order):
//   mask         valid = where(row == 1); k = len(valid): k == 0 -> 0, k == 1 -> valid[0] (nothing drawn), else valid[j] with j = Generator.choice's
//                bounded integer: Lemire's method on 32-BIT values (numpy/random/src/distributions: buffered_bounded_lemire_uint32), which
//                come from PCG64's buffered half (pcg64_next32: low half of a 64-bit output first, the high half kept for the next call)
//   probability  valid = (p > 0) & (p <= 1); cdf = cumsum(p[valid] / sum(p)); cdf /= cdf[-1]; valid[searchsorted(cdf, random(), "right")]
//
// The weighted draw takes one 64-bit output per row, like the plain sampler: lane i's state is its draw.  The masked draw takes a DATA-DEPENDENT
// number of 32-bit values, so a row's place in the stream is the number of values the rows before it took: per-workgroup counts, an exclusive
// scan of them by one workgroup, then every row skips ahead to its value.  A rejected bounded draw (probability (2^32 mod k) / 2^32) takes one
// value more and moves every later row: the draw kernel only flags it, and one workgroup -- launched with every batch, idle unless the flag is
// set -- recomputes the rows behind it (docs/classic_kernels.md).  No workgroup ever waits for another: the dependencies are launch boundaries.
#include "action_mask_internal.h"

namespace mi_actmask {
namespace {

using mi::make_u128;
using mi::PcgJump;
using mi::u128;

constexpr int kBlock = 256;

__device__ __forceinline__ uint64_t pcg_output(u128 state) {  // XSL-RR of the state AFTER its step
    const uint64_t hi = (uint64_t)(state >> 64), lo = (uint64_t)state;
    const uint64_t x = hi ^ lo;
    const unsigned rot = (unsigned)(hi >> 58);
    return (x >> rot) | (x << ((0u - rot) & 63u));
}
// `delta` steps on from `s`: one affine map per set bit
__device__ __forceinline__ u128 skip_ahead(u128 s, uint64_t delta, const PcgJump *pow2) {
    for (int j = 0; delta; j++, delta >>= 1)
        if (delta & 1ull) s = pow2[j].mult * s + pow2[j].plus;
    return s;
}
// what the stream needs to hand out its v-th 32-bit value of the batch (pcg64_next32): the pending half first, then low / high halves of the outputs
struct Halves {
    u128 base;
    uint32_t has, uinteger;
    const PcgJump *pow2;
    __device__ __forceinline__ uint32_t value(uint32_t v) const {
        if (has && v == 0) return uinteger;
        const uint32_t w = v - has;
        const uint64_t o = pcg_output(skip_ahead(base, (uint64_t)(w >> 1) + 1ull, pow2));
        return (w & 1u) ? (uint32_t)(o >> 32) : (uint32_t)o;
    }
};
__device__ __forceinline__ Halves halves_of(const Ctl *ctl, const PcgJump *pow2) {
    Halves h;
    h.base = make_u128(ctl->base_hi, ctl->base_lo), h.has = ctl->has_uint32 ? 1u : 0u, h.uinteger = ctl->uinteger, h.pow2 = pow2;
    return h;
}

// one mask row: its ones as a bit set, their number, and whether a value other than 0 / 1 occurs
struct MaskRow {
    uint64_t bits;
    int k;
    bool bad;
};
__device__ __forceinline__ MaskRow read_row(const int8_t *mask, size_t i, int A) {
    MaskRow r = {0ull, 0, false};
    const int8_t *m = mask + i * (size_t)A;
    for (int a = 0; a < A; a++) {
        const int8_t x = m[a];
        r.bad |= (x != 0 && x != 1);
        r.bits |= (uint64_t)(x == 1) << a;
    }
    r.k = __popcll(r.bits);
    return r;
}
__device__ __forceinline__ int nth_one(uint64_t bits, uint32_t j) {
    for (; j; j--) bits &= bits - 1ull;
    return bits ? __builtin_ctzll(bits) : 0;
}
// Lemire's bounded draw on one 32-bit value: index j in [0, k), `rejected`: the reference draws again (leftover < (2^32 - k) mod k)
__device__ __forceinline__ uint32_t lemire(uint32_t x, uint32_t k, bool &rejected) {
    const uint64_t m = (uint64_t)x * k;
    rejected = (uint32_t)m < (0u - k) % k;
    return (uint32_t)(m >> 32);
}
// the action of a row whose first value is number v of the batch; `rejected` rows hold a provisional value
__device__ __forceinline__ int64_t masked_action(const MaskRow &r, const Halves &h, uint32_t v, bool &rejected) {
    rejected = false;
    if (r.k < 2) return r.k == 1 ? (int64_t)nth_one(r.bits, 0) : 0;
    return (int64_t)nth_one(r.bits, lemire(h.value(v), (uint32_t)r.k, rejected));
}

// ---- masked, stage 1: 32-bit values per row (k >= 2: one), summed per workgroup; bit 31 of a partial: the workgroup saw an invalid row ----------
__global__ __launch_bounds__(kBlock) void act_mask_count_kernel(const int8_t *mask, int N, int A, uint32_t *partial) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool need = false, bad = false;
    if (i < N) {
        const MaskRow r = read_row(mask, (size_t)i, A);
        need = r.k >= 2, bad = r.bad;
    }
    __shared__ uint32_t cnt[kBlock / 64], flag[kBlock / 64];
    const uint64_t nb = __ballot(need), bb = __ballot(bad);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = (uint32_t)__popcll(nb), flag[threadIdx.x >> 6] = bb ? 1u : 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0, f = 0;
        for (int w = 0; w < kBlock / 64; w++) c += cnt[w], f |= flag[w];
        partial[blockIdx.x] = c | (f << 31);
    }
}

// ---- stage 2 (both paths), ONE workgroup: the partials become their exclusive prefix; the batch's control words are set for the stages behind ----
__global__ __launch_bounds__(kBlock) void act_scan_kernel(uint32_t *partial, int nblocks, Ctl *ctl, const uint64_t *lane, int N, uint64_t inc_hi,
                                                          uint64_t inc_lo, int force_repair, int *error) {
    __shared__ uint32_t s[kBlock];
    const int t = threadIdx.x;
    uint32_t carry = 0;
    int bad = 0;
    for (int base = 0; base < nblocks; base += kBlock) {
        const int idx = base + t;
        uint32_t x = idx < nblocks ? partial[idx] : 0u;
        bad |= (int)(x >> 31);
        x &= 0x7fffffffu;
        s[t] = x;
        __syncthreads();
        for (int off = 1; off < kBlock; off <<= 1) {
            const uint32_t y = t >= off ? s[t - off] : 0u;
            __syncthreads();
            s[t] += y;
            __syncthreads();
        }
        if (idx < nblocks) partial[idx] = carry + s[t] - x;
        carry += s[kBlock - 1];
        __syncthreads();
    }
    bad = __syncthreads_or(bad);
    if (t == 0) {
        mi::Pcg64 g;  // lane 0 holds the state whose output is the next draw: the position itself is one step back
        g.state = make_u128(lane[0], lane[(size_t)N]), g.inc = make_u128(inc_hi, inc_lo);
        g.unstep();
        ctl->base_hi = (uint64_t)(g.state >> 64), ctl->base_lo = (uint64_t)g.state;
        ctl->bad = bad ? 1u : 0u;
        ctl->first = force_repair ? 0u : 0xffffffffu;
        ctl->total = carry;
        ctl->outputs = 0u;
        if (bad) *error = kErrInvalidSampleArg;
    }
}

// ---- masked, stage 3: every row finds its slot and draws; a rejected draw is flagged for the repair stage -----------------------------------------
__global__ __launch_bounds__(kBlock) void act_mask_draw_kernel(const int8_t *mask, int N, int A, const uint32_t *prefix, Ctl *ctl, const PcgJump *pow2,
                                                               uint32_t *slot, int64_t *out) {
    if (ctl->bad) return;  // (uniform: the whole batch is refused)
    const int i = blockIdx.x * kBlock + threadIdx.x;
    MaskRow r = {0ull, 0, false};
    if (i < N) r = read_row(mask, (size_t)i, A);
    const bool need = r.k >= 2;
    __shared__ uint32_t cnt[kBlock / 64];
    const uint64_t nb = __ballot(need);
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (ln == 0) cnt[wv] = (uint32_t)__popcll(nb);
    __syncthreads();
    uint32_t before = (uint32_t)__popcll(nb & ((1ull << ln) - 1ull));
    for (int w = 0; w < wv; w++) before += cnt[w];
    if (i >= N) return;
    const Halves h = halves_of(ctl, pow2);
    const uint32_t v = prefix[blockIdx.x] + before;
    slot[i] = v;
    bool rejected;
    out[i] = masked_action(r, h, v, rejected);
    if (rejected) atomicMin(&ctl->first, (uint32_t)i);
}

// ---- masked, stage 4, ONE workgroup: the rows behind a rejected draw, and the stream's new position -------------------------------------------------
// Row `r` (the first whose draw was rejected) is drawn the reference's way, value after value; it took `extra` values more than its one, so
// every later row's slot moves by that much: they are recomputed in parallel, which may reject again further on -- r strictly grows, so the
// loop ends after at most N rounds (in practice one: a rejection has probability <= 4 / 2^32 per row for k <= 6).
__global__ __launch_bounds__(kBlock) void act_mask_repair_kernel(const int8_t *mask, int N, int A, const uint32_t *slot, Ctl *ctl, const PcgJump *pow2,
                                                                 int64_t *out) {
    if (ctl->bad) return;
    __shared__ uint32_t s_shift, s_next;
    const Halves h = halves_of(ctl, pow2);
    uint32_t r = ctl->first, shift = 0;
    while (r < (uint32_t)N) {
        if (threadIdx.x == 0) {
            const MaskRow row = read_row(mask, (size_t)r, A);
            if (row.k >= 2) {
                uint32_t v = slot[r] + shift, j;
                bool rejected;
                do j = lemire(h.value(v++), (uint32_t)row.k, rejected);
                while (rejected);
                out[r] = (int64_t)nth_one(row.bits, j);
                shift = v - slot[r] - 1u;
            }
            s_shift = shift, s_next = 0xffffffffu;
        }
        __syncthreads();
        shift = s_shift;
        for (uint32_t i = r + 1u + threadIdx.x; i < (uint32_t)N; i += kBlock) {
            const MaskRow row = read_row(mask, (size_t)i, A);
            bool rejected;
            out[i] = masked_action(row, h, slot[i] + shift, rejected);
            if (rejected) {  // (this thread's later rows lie behind it: the next round recomputes them)
                atomicMin(&s_next, i);
                break;
            }
        }
        __syncthreads();
        r = s_next;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t values = ctl->total + shift;
        if (values) {  // pcg64_next32: an odd number of values taken from the outputs leaves the last output's high half pending
            const uint32_t w = values - h.has;
            if (w) ctl->uinteger = (uint32_t)(pcg_output(skip_ahead(h.base, (uint64_t)((w + 1u) >> 1), pow2)) >> 32);
            ctl->has_uint32 = w & 1u;
            ctl->outputs = (w + 1u) >> 1;
        }
    }
}

// ---- masked, stage 5: the per-lane states for the new position (lane i: the state whose output is draw i from there) ----------------------------------
__global__ __launch_bounds__(kBlock) void act_mask_lanes_kernel(const Ctl *ctl, const PcgJump *pow2, uint64_t *lane, int N) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N || ctl->bad || ctl->outputs == 0u) return;
    const u128 s = skip_ahead(make_u128(ctl->base_hi, ctl->base_lo), (uint64_t)ctl->outputs + (uint64_t)i + 1ull, pow2);
    lane[i] = (uint64_t)(s >> 64), lane[(size_t)N + i] = (uint64_t)s;
}

// ---- weighted, stage 1: validate the row and compute its action from the lane's draw; nothing of the stream moves yet -------------------------------
__global__ __launch_bounds__(kBlock) void act_weighted_kernel(const double *prob, int N, int A, const uint64_t *lane, uint32_t *action, uint32_t *partial) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    if (i < N) {
        const double *row = prob + (size_t)i * (size_t)A;
        double p[kMaxWeightedActions], cdf[kMaxWeightedActions];
        bool valid[kMaxWeightedActions];
        double sum = 0.0;
#pragma unroll
        for (int a = 0; a < kMaxWeightedActions; a++) {
            p[a] = a < A ? row[a] : 0.0;
            valid[a] = p[a] > 0.0 && p[a] <= 1.0;
            if (a < A) {
                bad |= !(p[a] == 0.0 || valid[a]);  // (NaN fails both)
                sum = a == 0 ? p[0] : sum + p[a];   // np.sum of up to 7 elements: left to right
            }
        }
        bad |= !(fabs(sum - 1.0) <= 1e-8 + 1e-5 * 1.0);  // np.isclose(sum, 1): atol + rtol * |1|
        double acc = 0.0;
        int nv = 0;
#pragma unroll
        for (int a = 0; a < kMaxWeightedActions; a++) {
            if (valid[a]) {
                const double q = p[a] / sum;
                acc = nv == 0 ? q : acc + q;  // np.cumsum: sequential
                nv++;
            }
            cdf[a] = acc;
        }
        const double u = (double)(pcg_output(make_u128(lane[i], lane[(size_t)N + i])) >> 11) * (1.0 / 9007199254740992.0);
        int le = 0;  // searchsorted(cdf / cdf[-1], u, side="right"): how many entries are <= u
#pragma unroll
        for (int a = 0; a < kMaxWeightedActions; a++)
            if (valid[a] && cdf[a] / acc <= u) le++;
        if (le >= nv) le = nv - 1;  // (cdf[-1] / cdf[-1] == 1 > u: not reached by a valid row)
        int act = 0, seen = 0;
#pragma unroll
        for (int a = 0; a < kMaxWeightedActions; a++)
            if (valid[a]) {
                if (seen == le) act = a;
                seen++;
            }
        action[i] = (uint32_t)act;
    }
    __shared__ uint32_t flag[kBlock / 64];
    const uint64_t bb = __ballot(bad);
    if ((threadIdx.x & 63) == 0) flag[threadIdx.x >> 6] = bb ? 1u : 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t f = 0;
        for (int w = 0; w < kBlock / 64; w++) f |= flag[w];
        partial[blockIdx.x] = f << 31;
    }
}

// ---- weighted, stage 3: a valid batch is handed out and every lane moves on by one batch, like act_sample_kernel ---------------------------------------
__global__ __launch_bounds__(kBlock) void act_weighted_commit_kernel(const uint32_t *action, const Ctl *ctl, uint64_t *lane, PcgJump jump_n, int64_t *out, int N) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N || ctl->bad) return;
    out[i] = (int64_t)action[i];
    const u128 s = jump_n.mult * make_u128(lane[i], lane[(size_t)N + i]) + jump_n.plus;
    lane[i] = (uint64_t)(s >> 64), lane[(size_t)N + i] = (uint64_t)s;
}

__global__ void act_set_buffered_kernel(Ctl *ctl, uint32_t has_uint32, uint32_t uinteger) { ctl->has_uint32 = has_uint32 ? 1u : 0u, ctl->uinteger = uinteger; }

}  // namespace

hipError_t sample_masked(const Work &w, const int8_t *mask, int64_t *out) {
    const dim3 grid((unsigned)((w.N + kBlock - 1) / kBlock)), block(kBlock), one(1);
    hipLaunchKernelGGL(act_mask_count_kernel, grid, block, 0, w.stream, mask, w.N, w.A, w.partial);
    hipLaunchKernelGGL(act_scan_kernel, one, block, 0, w.stream, w.partial, (int)grid.x, w.ctl, w.lane, w.N, w.inc_hi, w.inc_lo, w.force_repair, w.error);
    hipLaunchKernelGGL(act_mask_draw_kernel, grid, block, 0, w.stream, mask, w.N, w.A, w.partial, w.ctl, w.pow2, w.slot, out);
    hipLaunchKernelGGL(act_mask_repair_kernel, one, block, 0, w.stream, mask, w.N, w.A, w.slot, w.ctl, w.pow2, out);
    hipLaunchKernelGGL(act_mask_lanes_kernel, grid, block, 0, w.stream, w.ctl, w.pow2, w.lane, w.N);
    return hipGetLastError();
}

hipError_t sample_weighted(const Work &w, const double *prob, int64_t *out) {
    const dim3 grid((unsigned)((w.N + kBlock - 1) / kBlock)), block(kBlock), one(1);
    hipLaunchKernelGGL(act_weighted_kernel, grid, block, 0, w.stream, prob, w.N, w.A, w.lane, w.slot, w.partial);
    hipLaunchKernelGGL(act_scan_kernel, one, block, 0, w.stream, w.partial, (int)grid.x, w.ctl, w.lane, w.N, w.inc_hi, w.inc_lo, 0, w.error);
    hipLaunchKernelGGL(act_weighted_commit_kernel, grid, block, 0, w.stream, w.slot, w.ctl, w.lane, w.jump_n, out, w.N);
    return hipGetLastError();
}

hipError_t set_buffered(const Work &w, uint32_t has_uint32, uint32_t uinteger) {
    hipLaunchKernelGGL(act_set_buffered_kernel, dim3(1), dim3(1), 0, w.stream, w.ctl, has_uint32, uinteger);
    return hipGetLastError();
}

}  // namespace mi_actmask
