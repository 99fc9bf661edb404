// lookahead_policy.hip -- mi_lookahead_policy's kernels as their own translation unit: namespace mi_lookahead_policy_unit, the launch function engine.hip
// calls (engine_types.h declares it) and every instantiation of lookahead_policy_kernel.
//
// What it computes (include/mi355env.h mi_lookahead_policy): the candidate loop candidate_lane.h describes -- K candidates per sub-environment, each on
// a private copy of lane i, stopped after the first step that ends the episode, the env only read -- with the action of every step computed IN the lane
// from the float32 observation of the lane's current state: a linear map (hidden == 0) or one hidden layer of `hidden` ReLU units, candidate k using
// row k of `params`.  The arithmetic is fixed operation by operation (the header): float32, every product and every sum rounded on its own (this unit
// is built with -ffp-contract=off like its sibling and must stay so), hidden units in ascending order, each consumed by all outputs as soon as it
// exists -- so the kernel holds A accumulators and never an array of activations -- and the strict-greater scan for the Discrete kinds.
//
// The kernel's device text is its own, not candidate_lane.h's parts: built from them, at the same static counts, 9 of 24 measured configurations ran
// 0.1 - 2.1 % slower (docs/results_log.md), and no part alone left the step loops' instruction sequence as it was.  It shares the output struct and
// the host side: the dispatch to the env type, from which P comes too, and the grid.  The observation is needed every step here, so the loop is
// lane_step_fused's shape: advance, select, take the observation of the state the lane now holds -- which hands its sin / cos to the next step
// (envs_classic.h Trig) and, for Acrobot, to the terminal test (terminal_after_obs).  The observation after the loop IS final_obs.
//
// Parameters, two paths chosen on the host (policy_path, below):
//   LDS     a workgroup's 256 lanes span candidates k_lo .. k_hi, whose rows are one contiguous range of `params`; it is staged into LDS with
//           coalesced loads before tables_init's barrier, hidden layers permuted into per-unit records (W1 row, b1[u], column u of W2) so that a
//           unit is R = OBS + 1 + A consecutive floats at a compile-time stride.  With N >= 256 every lane of a wavefront reads the same address: a
//           broadcast.
//   global  the range does not fit kPolicyLdsBytes (many short rows' worth of candidates per workgroup, or a large hidden layer): each lane reads its
//           row from global memory in the caller's layout.
// Both evaluate the same operations on the same operands in the same order: identical bits (tests/test_gpu_lookahead_policy.py forces each).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "candidate_lane.h"

namespace {

struct PolicyPtrs {
    const float *params;  // [K][P]
    CandidateOut out;
    int H, KN, hidden, P;
    double gamma;
};

// the most parameter bytes a workgroup stages: next to the math tables (11 KB) two workgroups per CU stay far inside the 160 KB
constexpr int kPolicyLdsBytes = 32 * 1024;

// wavefronts per SIMD the kernels' registers are bounded for (lookahead.hip kLookWaves).  docs/results_log.md has the table of all 20 instantiations.
template <class E>
struct PolicyWaves {
    static constexpr int value = 2;
};
// Acrobot with per-lane attributes: lookahead_kernel's widest instantiation (241 registers) plus the observation, the accumulators and two unit
// records held across the step does not fit 256 -- 12 / 16 spilled registers (LDS / global path) at two wavefronts, none at one
template <class M>
struct PolicyWaves<AcrobotAttrT<M>> {
    static constexpr int value = 1;
};

template <class E>
struct PolicyDims {
    static constexpr int OBS = E::OBS;
    static constexpr int A = []() {
        if constexpr (E::DISCRETE)
            return E::N_ACTIONS;
        else
            return 1;  // act_dim of both Box kinds
    }();
    static constexpr int R = OBS + 1 + A;  // floats of one hidden unit's record
};

// one hidden unit: row u of W1, b1[u], column u of W2
template <class E>
struct PolicyUnit {
    float w1[PolicyDims<E>::OBS], b1, w2[PolicyDims<E>::A];
};
template <class E, bool LDS>
MI_DEV void fetch_unit(const float *row, int h, int u, PolicyUnit<E> &r) {
    constexpr int OBS = PolicyDims<E>::OBS, A = PolicyDims<E>::A, R = PolicyDims<E>::R;
    if constexpr (LDS) {
        const float *p = row + u * R;
#pragma unroll
        for (int j = 0; j < OBS; j++) r.w1[j] = p[j];
        r.b1 = p[OBS];
#pragma unroll
        for (int o = 0; o < A; o++) r.w2[o] = p[OBS + 1 + o];
    } else {
#pragma unroll
        for (int j = 0; j < OBS; j++) r.w1[j] = row[u * OBS + j];
        r.b1 = row[h * OBS + u];
#pragma unroll
        for (int o = 0; o < A; o++) r.w2[o] = row[h * (OBS + 1) + o * h + u];
    }
}

// The action of one step from the observation `x` (the header's contract; tests/lookahead_policy_cases.py policy_actions is the same text in NumPy).
template <class E, bool LDS>
MI_DEV typename E::Act policy_action(const float *row, int h, const float (&x)[E::OBS]) {
    constexpr int OBS = PolicyDims<E>::OBS, A = PolicyDims<E>::A, R = PolicyDims<E>::R;
    float y[A];
    if (h == 0) {  // W[A][OBS], b[A]: the same layout on both paths
#pragma unroll
        for (int o = 0; o < A; o++) y[o] = row[A * OBS + o];
#pragma unroll
        for (int o = 0; o < A; o++) {
#pragma unroll
            for (int j = 0; j < OBS; j++) y[o] = y[o] + row[o * OBS + j] * x[j];
        }
    } else {
        const float *b2 = LDS ? row + h * R : row + h * (OBS + 1) + A * h;
#pragma unroll
        for (int o = 0; o < A; o++) y[o] = b2[o];
        PolicyUnit<E> cur;
        fetch_unit<E, LDS>(row, h, 0, cur);
        for (int u = 0; u < h; u++) {
            PolicyUnit<E> nxt;  // the next unit is requested before this one is evaluated
            fetch_unit<E, LDS>(row, h, u + 1 < h ? u + 1 : u, nxt);
            float z = cur.b1;
#pragma unroll
            for (int j = 0; j < OBS; j++) z = z + cur.w1[j] * x[j];
            const float a = z > 0.0f ? z : 0.0f;  // (a NaN gives 0)
#pragma unroll
            for (int o = 0; o < A; o++) y[o] = y[o] + cur.w2[o] * a;
            cur = nxt;
        }
    }
    if constexpr (E::DISCRETE) {
        int best = 0;  // strict: the first maximum wins and no comparison with a NaN holds; always inside the space
#pragma unroll
        for (int o = 1; o < A; o++) {
            bool better = false;
#pragma unroll
            for (int b = 0; b < o; b++) better = best == b ? y[o] > y[b] : better;  // y[o] > y[best] without indexing registers
            best = better ? o : best;
        }
        return (typename E::Act)best;
    } else {
        return (typename E::Act)y[0];  // the float32 action row; the env's own clip applies
    }
}

extern __shared__ __align__(16) float g_policy_rows[];

// The rows of the candidates this workgroup's lanes belong to, params[k_lo .. k_hi], into LDS: straight for hidden == 0, per-unit records otherwise.
// Consecutive threads read consecutive floats.  The caller's barrier (tables_init) publishes them.
template <class E>
MI_DEV void stage_rows(const PolicyPtrs &io, int N, int k_lo, int k_hi) {
    constexpr int OBS = PolicyDims<E>::OBS, A = PolicyDims<E>::A, R = PolicyDims<E>::R;
    const int P = io.P, h = io.hidden;
    const int count = (k_hi - k_lo + 1) * P;
    const float *src = io.params + (size_t)k_lo * P;
    if (h == 0) {
        for (int q = threadIdx.x; q < count; q += kBlock) g_policy_rows[q] = src[q];
        return;
    }
    const int w1_end = h * OBS, b1_end = w1_end + h, w2_end = b1_end + A * h;
    for (int q = threadIdx.x; q < count; q += kBlock) {
        const float v = src[q];
        const int r = q / P, p = q - r * P;
        int dst;
        if (p < w1_end) {
            const int u = p / OBS;
            dst = u * R + (p - u * OBS);
        } else if (p < b1_end) {
            dst = (p - w1_end) * R + OBS;
        } else if (p < w2_end) {
            const int o = (p - b1_end) / h;
            dst = (p - b1_end - o * h) * R + OBS + 1 + o;
        } else {
            dst = h * R + (p - w2_end);
        }
        g_policy_rows[r * P + dst] = v;
    }
}

template <class E, bool LDS>
__global__ __launch_bounds__(kBlock, PolicyWaves<E>::value) void lookahead_policy_kernel(DevEnv d, PolicyPtrs io, AttrDev at) {
    typedef typename E::Act Act;
    const int j0 = (int)(blockIdx.x * (unsigned)kBlock);  // (< KN < 2^31)
    const bool live = (int64_t)j0 + threadIdx.x < io.KN;  // (the last workgroup's lanes may pass 2^31)
    const int j = live ? j0 + (int)threadIdx.x : 0;
    const int k = live ? j / d.N : 0;
    const int i = live ? j - k * d.N : 0;
    const int k_lo = j0 / d.N;
    // everything the lane reads before its first step -- state, elapsed | flags, attributes, generator (a type whose step draws) -- and the workgroup's
    // parameter rows are requested before the math tables are staged into LDS: one trip to memory, not two (CandidateStart's order)
    double s[E::S];
    uint32_t meta = 0;
    uint64_t g[4] = {0, 0, 0, 0};
    AttrRequest<E> ar;
    if (live) {
#pragma unroll
        for (int q = 0; q < E::S; q++) s[q] = d.state[(size_t)q * d.N + i];
        meta = d.meta[i];
        if constexpr (HasStepDraws<E>::value) {
#pragma unroll
            for (int q = 0; q < 4; q++) g[q] = d.rng[(size_t)q * d.N + i];
        }
        ar.request(at, d, i);
    }
    if constexpr (LDS) {
        const int j_last = io.KN - j0 > kBlock ? j0 + kBlock - 1 : io.KN - 1;
        stage_rows<E>(io, d.N, k_lo, j_last / d.N);
    }
    tables_init<E>();
    if (!live) return;
    const float *row;
    if constexpr (LDS)
        row = g_policy_rows + (k - k_lo) * io.P;
    else
        row = io.params + (size_t)k * io.P;
    Lane<E> L;
#pragma unroll
    for (int q = 0; q < E::S; q++) hold_opaque(s[q]), L.s[q] = s[q];
    hold_opaque(meta);
    L.elapsed = meta & kElapsedMask, L.flags = meta >> kFlagShift;
    trig_invalidate(L.trig);
    ar.arrive(L.trig);
    [[maybe_unused]] Pcg64 gen;  // the sub-environment's generator, copied: every candidate of i sees the draws the env would see next
    if constexpr (HasStepDraws<E>::value) {
#pragma unroll
        for (int q = 0; q < 4; q++) hold_opaque(g[q]);
        gen.state = make_u128(g[0], g[1]), gen.inc = make_u128(g[2], g[3]);
    }
    // a lane that waits for its reset (NEXT_STEP, DISABLED) has nothing to look ahead from: it starts finished
    // (integers, not bools, for what lives across the loop: ResetQueue::have's reason)
    uint32_t active = (L.flags & kNeedsReset) ? 0u : 1u, te_last = 0u, tr_last = 0u;
    int32_t steps = 0;
    double G = 0.0, disc = 1.0;
    float o[E::OBS];  // the observation of the state the lane holds: what step() would have returned
    E::obs(L.s, L.flags, o, L.trig);
    for (int t = 0; t < io.H; t++) {
        const Act a = policy_action<E, LDS>(row, io.hidden, o);
        const bool go = active != 0u;
        if constexpr (HasStepDraws<E>::value) {
            if (go && E::step_draws(L.trig)) E::step_drawn(L.trig, gen.next_double());
        }
        double s0[E::S];
#pragma unroll
        for (int q = 0; q < E::S; q++) s0[q] = L.s[q];
        uint32_t sflags = L.flags;
        double rew;
        bool te;
        if constexpr (E::SPLIT_TERMINAL) {
            // Acrobot (lane_step_fused): the terminal test needs cos(theta1) of the NEW state, which the observation evaluates anyway.  A finished
            // candidate's flag and reward are discarded below.
            E::integrate(L.s, sflags, a, L.trig);
#pragma unroll
            for (int q = 0; q < E::S; q++) L.s[q] = go ? L.s[q] : s0[q];
            L.flags = go ? sflags : L.flags;
            E::obs(L.s, L.flags, o, L.trig);
            E::terminal_after_obs(L.s, L.trig, rew, te);
        } else {
            E::step(L.s, sflags, a, d.P, rew, te, L.trig);
#pragma unroll
            for (int q = 0; q < E::S; q++) L.s[q] = go ? L.s[q] : s0[q];
            L.flags = go ? sflags : L.flags;
            E::obs(L.s, L.flags, o, L.trig);
        }
        const uint32_t elapsed = L.elapsed + 1u;  // TimeLimit.step (wrappers/common.py:129-133)
        const bool tr = d.max_steps > 0 && (int)elapsed >= d.max_steps;
        L.elapsed = go ? elapsed : L.elapsed;
        const double term = disc * rew;  // (rounded before the sum: -ffp-contract=off)
        G = go ? G + term : G;
        disc = go ? disc * io.gamma : disc;
        steps += go ? 1 : 0;
        te_last = go ? (te ? 1u : 0u) : te_last;
        tr_last = go ? (tr ? 1u : 0u) : tr_last;
        active = (go && (te || tr)) ? 0u : active;
    }
    if (io.out.returns) io.out.returns[j] = G;
    if (io.out.steps) io.out.steps[j] = steps;
    if (io.out.terminated) io.out.terminated[j] = (uint8_t)te_last;
    if (io.out.truncated) io.out.truncated[j] = (uint8_t)tr_last;
    if (io.out.final_obs) store_row<E::OBS>(io.out.final_obs + (size_t)j * E::OBS, o);
}

// Which path: MI355ENV_LOOKAHEAD_POLICY_PATH = "global" sends every call down the global path, "lds" refuses a call whose rows do not fit instead of
// falling back (tests, A/B: scripts/lookahead_policy_bench.py); otherwise LDS whenever the rows of the most candidates a workgroup can span fit.
// Read at every call: a test switches it between two calls of one process.
int policy_path(const mi_vecenv *v, const PolicyPtrs &p, int candidates, bool &lds, size_t &bytes) {
    const int N = v->cfg.num_envs;
    const int64_t span = (kBlock + N - 1) / N + 1;  // candidates k_lo .. k_hi of 256 consecutive lanes
    const int64_t rows = span < candidates ? span : candidates;
    const int64_t need = rows * p.P * (int64_t)sizeof(float);
    lds = need <= kPolicyLdsBytes;
    const char *force = getenv("MI355ENV_LOOKAHEAD_POLICY_PATH");
    if (force && !strcmp(force, "global")) lds = false;
    if (force && !strcmp(force, "lds") && !lds) return fail(MI_ERR_UNSUPPORTED, "mi_lookahead_policy: MI355ENV_LOOKAHEAD_POLICY_PATH=lds, but a workgroup's parameter rows exceed 32 KiB");
    bytes = lds ? (size_t)need : 0;
    return MI_OK;
}

template <class E>
int launch_for(mi_vecenv *v, const PolicyPtrs &p, int candidates) {
    bool lds;
    size_t bytes;
    if (int rc = policy_path(v, p, candidates, lds, bytes)) return rc;
    const AttrDev at = {v->d_attr, v->attr_mask};
    const dim3 grid(candidate_grid(p.KN));
    if (lds)
        hipLaunchKernelGGL((lookahead_policy_kernel<E, true>), grid, dim3(kBlock), bytes, v->stream, v->d, p, at);
    else
        hipLaunchKernelGGL((lookahead_policy_kernel<E, false>), grid, dim3(kBlock), 0, v->stream, v->d, p, at);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace

namespace mi_lookahead_policy_unit {
int params_per_candidate(int kind, int hidden) {
    int P = 0;
    for_candidate_env<false>(kind, false, MI_F32, [&](auto e) {
        typedef PolicyDims<typename decltype(e)::type> D;
        P = hidden == 0 ? D::A * (D::OBS + 1) : hidden * (D::OBS + 1) + D::A * (hidden + 1);
    });
    return P;
}

int launch(mi_vecenv *v, const float *params, int hidden, int horizon, int candidates, double gamma, double *returns, int32_t *steps, uint8_t *terminated,
           uint8_t *truncated, float *final_obs) {
    const PolicyPtrs p = {params, {returns, steps, terminated, truncated, final_obs}, horizon, candidates * v->cfg.num_envs, hidden,
                          params_per_candidate(v->cfg.kind, hidden), gamma};
    return dispatch_candidate_env<false>(v, MI_F32, "mi_lookahead_policy", [&](auto e) { return launch_for<typename decltype(e)::type>(v, p, candidates); });
}
}  // namespace mi_lookahead_policy_unit
