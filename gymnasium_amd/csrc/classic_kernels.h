// classic_kernels.h -- the kernels of the five classic-control kinds over the lane machinery of lane_step.h: the step epilogue (NormalizeObservation /
// NormalizeReward / ClipReward as the output stage of a step), step_kernel, step_wrapped_kernel and reset_kernel, the fused rollouts (rollout_kernel,
// rollout_infos_kernel, rollout_wrapped_kernel), the two-role rollout (rollout_duo_kernel) and the shared-generator kernels of MI_CFG_SHARED_RNG.
// Included by classic.hip only, which instantiates and launches them.
#ifndef MI355ENV_CLASSIC_KERNELS_H
#define MI355ENV_CLASSIC_KERNELS_H
#include "episode_word.h"
#include "lane_step.h"
#include "wrappers_internal.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// Step epilogue: gymnasium.wrappers.vector.{NormalizeObservation, NormalizeReward, ClipReward} as the output stage of step_kernel
// (mi_set_step_epilogue; the same arithmetic as the stand-alone passes of wrappers.hip, which cite the reference line by line).
//   phase 1, inside step_kernel: ClipReward placed before the normalisation, the discounted-return update, and this workgroup's column sums
//     of (obs - running mean), (return - running mean) and their squares: wavefront butterflies, four partials through LDS, one row of
//     doubles per workgroup in global memory.  No cross-workgroup traffic inside the kernel: a "last workgroup folds the rows" scheme
//     was measured first and cost 24 us per step -- a device-scope release on gfx950 writes back the whole XCD-local L2, which the step
//     has just filled with dirty state and observation lines.
//   phase 2, epilogue_finish: both normalisations need the UPDATED statistics of the whole batch (stateful_observation.py:146-152 updates
//     before it normalises), i.e. a grid-wide dependency, so they are one small second launch: every workgroup folds the rows (the same
//     sums in the same order -> the same bits everywhere), applies RunningMeanStd.update to a private copy and rewrites its obs / reward in
//     place, before the single device-to-host copy of the NumPy path; workgroup 0 also stores the new statistics -- into the handle's
//     SECOND buffer set, because the other workgroups are still reading the old one; the host swaps the two pointer sets after the launch.
//     Beyond kEpiFoldMax step workgroups the fold is a one-workgroup launch of its own (epilogue_combine) and phase 2 reads its result.
// Together: 2 launches per wrapped step (3 beyond 262144 sub-environments) instead of 1 + 4 + 5 + 1 with the stand-alone passes.
// ---------------------------------------------------------------------------------------------------------
MI_DEV double clip_to(double v, int flags, double lo, double hi) {  // np.clip(reward, min_reward, max_reward)
    if (flags & 1) v = v < lo ? lo : v;
    if (flags & 2) v = v > hi ? hi : v;
    return v;
}
__host__ __device__ inline bool epi_reduces(const EpiDev &e) { return (e.obs_on && e.obs_update) || (e.ret_on && e.ret_update); }

template <int NC>
MI_DEV void block_sum_columns(double (&v)[NC], double (*sh)[kEpiCols]) {  // result on threads < NC of the workgroup: v[0] = their column's total
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NC; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    }
    __syncthreads();  // sh may still be read from an earlier call
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NC; k++) sh[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < NC) {
        double t = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) t += sh[w][threadIdx.x];
        v[0] = t;
    }
}

// every thread of the workgroup calls this (valid = it owns a sub-environment); reward is rewritten with what the finish pass / the caller reads
template <class E>
MI_DEV void epilogue_phase1(const EpiDev &e, int i, bool valid, const float *obs, double &reward, bool terminated) {
    constexpr int OBS = E::OBS, NC = 2 * OBS + 3;
    static_assert(OBS <= kEpiObsMax, "epilogue rows are sized for the classic-control observations");
    double v[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) v[k] = 0;
    if (valid) {
        double r = clip_to(reward, e.clip_pre, e.pre_lo, e.pre_hi);
        if (e.ret_on) {  // stateful_reward.py:150-176 (wrappers.hip accumulate_return / update_stats)
            const bool pd = e.prev_done[i] != 0, active = e.same_step || !pd;
            float a = e.acc[i];
            if (active) {
                const float g = a * e.gamma;
                a = (float)((double)g * (terminated ? 0.0 : 1.0) + r);
                e.acc[i] = a;
            }
            if (e.ret_update && active) {
                const double d = (double)a - e.ret_mean[0];
                v[2 * OBS] = d, v[2 * OBS + 1] = d * d, v[2 * OBS + 2] = 1.0;
            }
        } else {
            r = clip_to(r, e.clip_post, e.post_lo, e.post_hi);  // no normalisation in between: both clips happen here
        }
        reward = r;
        if (e.obs_on && e.obs_update) {
#pragma unroll
            for (int c = 0; c < OBS; c++) {
                const double d = (double)obs[c] - e.obs_mean[c];
                v[c] = d, v[OBS + c] = d * d;
            }
        }
    }
    if (!epi_reduces(e)) return;  // grid-uniform
    __shared__ double sh[kBlock / 64][kEpiCols];
    block_sum_columns<NC>(v, sh);
    if (threadIdx.x < NC) e.partial[(size_t)blockIdx.x * kEpiCols + threadIdx.x] = v[0];
}

// The statistics after this step's update, for the whole workgroup: st[0..OBS) mean, st[OBS..2 OBS) var, st[2 OBS] return var, st[2 OBS + 1] return
// mean, st[2 OBS + 2] obs count, st[2 OBS + 3] return count.  fold = sum the step workgroups' rows first (else: the statistics as they are).
template <int OBS>
MI_DEV void epilogue_statistics(const EpiDev &e, int N, bool fold, double (*sh)[kEpiCols], double *st) {
    constexpr int NC = 2 * OBS + 3;
    if (threadIdx.x < OBS && e.obs_on) st[threadIdx.x] = e.obs_mean[threadIdx.x], st[OBS + threadIdx.x] = e.obs_var[threadIdx.x];
    if (threadIdx.x == 64) {
        st[2 * OBS] = e.ret_on ? e.ret_var[0] : 1.0, st[2 * OBS + 1] = e.ret_on ? e.ret_mean[0] : 0.0;
        st[2 * OBS + 2] = e.obs_on ? *e.obs_count : 0.0, st[2 * OBS + 3] = e.ret_on ? *e.ret_count : 0.0;
    }
    if (fold) {  // workgroup-uniform
        double v[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) v[k] = 0;
        for (int b = threadIdx.x; b < e.step_blocks; b += kBlock) {
#pragma unroll
            for (int k = 0; k < NC; k++) v[k] += e.partial[(size_t)b * kEpiCols + k];
        }
        block_sum_columns<NC>(v, sh);
        __syncthreads();
        if (threadIdx.x < NC) sh[0][threadIdx.x] = v[0];
        __syncthreads();
        if (e.obs_on && e.obs_update && (int)threadIdx.x < OBS) {  // float32 observations, float32 statistics (RunningMeanStd(dtype=float32))
            const int c = threadIdx.x;
            mi_wrap::update_column<float, float>(st[c], st[OBS + c], *e.obs_count, sh[0][c], sh[0][OBS + c], (double)N);
        }
        if (threadIdx.x == 64) {
            if (e.obs_on && e.obs_update) st[2 * OBS + 2] += (double)N;
            const double rows = sh[0][2 * OBS + 2];
            if (e.ret_on && e.ret_update && rows > 0) {  // float32 returns, float64 statistics; `if np.any(active)`
                mi_wrap::update_column<double, float>(st[2 * OBS + 1], st[2 * OBS], *e.ret_count, sh[0][2 * OBS], sh[0][2 * OBS + 1], rows);
                st[2 * OBS + 3] += rows;
            }
        }
    }
    __syncthreads();
}
template <int OBS>
MI_DEV void epilogue_store_statistics(const EpiDev &e, const double *st) {  // one workgroup: the updated statistics into the second buffer set
    if (e.obs_on && (int)threadIdx.x < OBS) e.obs_mean2[threadIdx.x] = st[threadIdx.x], e.obs_var2[threadIdx.x] = st[OBS + threadIdx.x];
    if (threadIdx.x == 64) {
        if (e.obs_on) *e.obs_count2 = st[2 * OBS + 2];
        if (e.ret_on) e.ret_var2[0] = st[2 * OBS], e.ret_mean2[0] = st[2 * OBS + 1], *e.ret_count2 = st[2 * OBS + 3];
    }
}
template <int OBS>
__global__ __launch_bounds__(kBlock) void epilogue_combine(EpiDev e, int N) {
    __shared__ double sh[kBlock / 64][kEpiCols];
    __shared__ double st[2 * OBS + 4];
    epilogue_statistics<OBS>(e, N, true, sh, st);
    epilogue_store_statistics<OBS>(e, st);
}

template <int OBS>
__global__ __launch_bounds__(kBlock) void epilogue_finish(EpiDev e, int N, float *obs, double *reward, const uint8_t *terminated, const uint8_t *truncated) {
    __shared__ double sh[kBlock / 64][kEpiCols];
    __shared__ double st[2 * OBS + 4];
    if (e.fold_in_finish) {
        epilogue_statistics<OBS>(e, N, epi_reduces(e), sh, st);
        if (blockIdx.x == 0 && epi_reduces(e)) epilogue_store_statistics<OBS>(e, st);
    } else {
        // epilogue_combine ran iff some statistic is being updated: then the second buffer set holds the statistics after this step.  With
        // frozen statistics (update_running_mean = False on both wrappers) nothing was folded or swapped: the primary set is the current one.
        const bool upd = epi_reduces(e);
        const double *om = upd ? e.obs_mean2 : e.obs_mean, *ov = upd ? e.obs_var2 : e.obs_var, *rv = upd ? e.ret_var2 : e.ret_var;
        if (threadIdx.x < OBS && e.obs_on) st[threadIdx.x] = om[threadIdx.x], st[OBS + threadIdx.x] = ov[threadIdx.x];
        if (threadIdx.x == 64 && e.ret_on) st[2 * OBS] = rv[0];
        __syncthreads();
    }
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    if (e.obs_on) {  // (obs - mean) / np.sqrt(var + epsilon), float32 throughout (wrappers.hip normalize_obs<float, float, float>)
        float o[OBS];
        load_row<OBS>(obs + (size_t)i * OBS, o);
#pragma unroll
        for (int c = 0; c < OBS; c++) {
            const float num = o[c] - (float)st[c];
            const float den = (float)sqrt((double)(float)((float)st[OBS + c] + (float)e.obs_eps));
            o[c] = num / den;
        }
        store_row<OBS>(obs + (size_t)i * OBS, o);
    }
    if (e.ret_on) {  // wrappers.hip finish_reward
        const uint8_t done = (terminated[i] || truncated[i]) ? 1 : 0;
        e.prev_done[i] = done;
        if (e.same_step && done) e.acc[i] = 0.0f;
        const double r = reward[i] / sqrt(st[2 * OBS] + e.ret_eps);
        reward[i] = clip_to(r, e.clip_post, e.post_lo, e.post_hi);
    }
}

// action_space.sample() of one lane from the state of the action stream whose output is the lane's draw
template <class E>
MI_DEV typename E::Act action_of_state(u128 astate) {
    if constexpr (E::SAMPLE_FROM_BITS) {
        return E::sample_state((uint64_t)(astate >> 64), (uint64_t)astate);
    } else {
        return E::sample((double)(pcg_output(astate) >> 11) * (1.0 / 9007199254740992.0));
    }
}

// SAMPLE: mi_step with actions == NULL -- `step(action_space.sample())` in one launch: the lane draws its own action from its state of the action
// stream (spaces/multi_discrete.py:176-178, spaces/box.py:463-465: draw number pos + i of the batched space's generator), which rides along with the
// lane's other loads, and leaves the state of its draw in the NEXT batch behind.  Nothing on the host changes from step to step: capturable.
template <class E, int MODE, bool EPI = false, bool SAMPLE = false>
__global__ __launch_bounds__(kBlock) void step_kernel(DevEnv d, StepPtrs io, EpiDev epi, AttrDev at) {
    // One step is ~200 instructions per lane between trips to memory that take a microsecond each: everything the step may read -- the lane's
    // state and action, its generator (consumed only by a reset, which some lane of a 64-CartPole wavefront needs on ~95 % of the steps) and the
    // workgroup's running totals -- is requested BEFORE the math tables are staged into LDS, so that all of it is ONE trip, not four in a row.
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    StepOut<E> o;
    LaneRequest<E> rq;
    AttrRequest<E> ar;
    constexpr bool GEN = MODE != MI_AUTORESET_DISABLED || HasStepDraws<E>::value;  // the lane's generator: consumed by a reset, or by the step itself
    if (i < d.N) rq.template request<SAMPLE>(d, io.actions, io.act_lane, i, GEN), ar.request(at, d, i);
    BlockTotals before = block_totals_load(d);
    tables_init<E>();
    hold_opaque(before.count), hold_opaque(before.ret);
    if (i < d.N) {
        Lane<E> L;
        Pcg64 gen;
        rq.arrive(L, gen);
        ar.arrive(L.trig);
        typename E::Act a = rq.a;
        if constexpr (SAMPLE) {
            const u128 astate = make_u128(rq.ag[0], rq.ag[1]);
            a = action_of_state<E>(astate);
            const u128 next = io.act_jump.mult * astate + io.act_jump.plus;
            io.act_lane[i] = (uint64_t)(next >> 64), io.act_lane[(size_t)d.N + i] = (uint64_t)next;
            if (io.actions_out) static_cast<typename E::Act *>(io.actions_out)[i] = a;
        }
        lane_step<E, MODE>(d, i, L, a, o, st, nullptr, GEN ? &gen : nullptr);
        store_lane<E>(d, i, L);
        if (io.obs) store_row<E::OBS>(io.obs + (size_t)i * E::OBS, o.obs);
        if (!EPI && io.reward) io.reward[i] = o.reward;
        if (io.terminated) io.terminated[i] = o.terminated;
        if (io.truncated) io.truncated[i] = o.truncated;
        if (MODE == MI_AUTORESET_SAME_STEP && io.final_obs && o.has_final)
            store_row<E::OBS>(io.final_obs + (size_t)i * E::OBS, o.final_obs);
        if (io.ep_ret) io.ep_ret[i] = o.ep_ret;
        if (io.ep_len) io.ep_len[i] = o.ep_len;
    }
    if (EPI) {  // the wrappers' statistics see what the step wrote; episode statistics (above) keep the raw reward, like the reference's order
        double r = i < d.N ? o.reward : 0.0;
        epilogue_phase1<E>(epi, i, i < d.N, o.obs, r, i < d.N && o.terminated);
        if (i < d.N && io.reward) io.reward[i] = r;
    }
    block_accumulate(d, st, before);
}

// mi_set_step_wrappers: step_kernel (without an epilogue) with RepeatAction / StickyAction around E::step -- lane_step_wrapped in place of lane_step, and
// StickyAction's two words per lane requested and stored with the rest of the lane.  The generator is always loaded: the sticky draw needs it.
// MAXSKIP (mi_set_max_and_skip): the lane's two frames are requested with them, before the barrier, and go back when the step wrote a slot.
template <class E, int MODE, bool SAMPLE, bool MAXSKIP = false>
__global__ __launch_bounds__(kBlock) void step_wrapped_kernel(DevEnv d, StepPtrs io, AttrDev at, WrapArg<MAXSKIP> w) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    StepOut<E> o;
    LaneRequest<E> rq;
    AttrRequest<E> ar;
    WrapLaneOf<E, MAXSKIP> sl;
    if (i < d.N) rq.template request<SAMPLE>(d, io.actions, io.act_lane, i, true), ar.request(at, d, i), load_wrap_lane(w, i, sl);
    if constexpr (MAXSKIP) {
        if (i < d.N) load_skip_lane(w, d, i, sl);
    }
    BlockTotals before = block_totals_load(d);
    tables_init<E>();
    hold_opaque(before.count), hold_opaque(before.ret);
    if (i < d.N) {
        Lane<E> L;
        Pcg64 gen;
        rq.arrive(L, gen);
        ar.arrive(L.trig);
        typename E::Act a = rq.a;
        if constexpr (SAMPLE) {
            const u128 astate = make_u128(rq.ag[0], rq.ag[1]);
            a = action_of_state<E>(astate);
            const u128 next = io.act_jump.mult * astate + io.act_jump.plus;
            io.act_lane[i] = (uint64_t)(next >> 64), io.act_lane[(size_t)d.N + i] = (uint64_t)next;
            if (io.actions_out) static_cast<typename E::Act *>(io.actions_out)[i] = a;  // the policy's action, not the effective one
        }
        if constexpr (MAXSKIP) arrive_skip_lane(sl);
        lane_step_wrapped<E, MODE, MAXSKIP>(d, w, sl, i, L, a, o, st, nullptr, &gen);
        store_lane<E>(d, i, L);
        store_wrap_lane(w, i, sl);
        if constexpr (MAXSKIP) store_skip_lane(w, d, i, sl);
        if (io.obs) store_row<E::OBS>(io.obs + (size_t)i * E::OBS, o.obs);
        if (io.reward) io.reward[i] = o.reward;
        if (io.terminated) io.terminated[i] = o.terminated;
        if (io.truncated) io.truncated[i] = o.truncated;
        if (MODE == MI_AUTORESET_SAME_STEP && io.final_obs && o.has_final)
            store_row<E::OBS>(io.final_obs + (size_t)i * E::OBS, o.final_obs);
        if (io.ep_ret) io.ep_ret[i] = o.ep_ret;
        if (io.ep_len) io.ep_len[i] = o.ep_len;
    }
    block_accumulate(d, st, before);
}

template <class E>
__global__ __launch_bounds__(kBlock) void reset_kernel(DevEnv d, const uint8_t *mask, int has_bounds, double b0, double b1,
                                                       float *obs) {
    tables_init<E>();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.N) return;
    if (mask && !mask[i]) return;
    Lane<E> L;
    load_lane<E>(d, i, L);
    double u[E::NDRAWS];
    draw_reset_values<E>(d, i, u);
    if (!has_bounds) E::default_bounds(b0, b1);
    L.flags &= ~kNeedsReset;
    E::reset_u(u, L.s, L.flags, b0, b1);
    L.elapsed = 0, L.ep_ret = 0.0, L.ep_len = 0;
    store_lane<E>(d, i, L);
    if (obs) {
        float o[E::OBS];
        E::obs(L.s, L.flags, o, L.trig);
        store_row<E::OBS>(obs + (size_t)i * E::OBS, o);
    }
}


// FULL: every trajectory output is materialised -- the per-store null checks (five taken branches per step for a
// wavefront that runs alone on its SIMD) disappear from the loop.
template <class E, int MODE, bool SAMPLE, bool FULL>
__global__ __launch_bounds__(kBlock) void rollout_kernel(DevEnv d, RolloutPtrs io, ActionStream as, int T, AttrDev at) {
    tables_init<E>();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    if (i < d.N) {
        Lane<E> L;
        load_lane<E>(d, i, L);
        {  // the lane's attributes and what they make invariant, once per launch (no-op for the types without attributes)
            AttrRequest<E> ar;
            ar.request(at, d, i);
            ar.arrive(L.trig);
        }
        u128 astate = 0;
        const u128 ainc = make_u128(as.inc_hi, as.inc_lo);
        if (SAMPLE) {
            if (as.lane_valid) {  // the lane's state from the last launch (or act_init_kernel)
                astate = make_u128(as.lane[i], as.lane[(size_t)d.N + i]);
            } else {  // skip ahead by (i + 1) draws: one affine map per set bit of (i + 1)
                astate = make_u128(as.state_hi, as.state_lo);
                uint32_t delta = (uint32_t)i + 1u;
                for (int j = 0; delta; j++, delta >>= 1)
                    if (delta & 1u) astate = as.pow2[j].mult * astate + as.pow2[j].plus;
            }
        }
        (void)ainc;
        const size_t N = (size_t)d.N;
        ResetQueue<E> q;
        q.have = 0u;
        q.rng = load_rng(d, i);
        // (per-kind unroll factor: 2 for Acrobot -- its long loop body schedules better as two steps, +4.6 %; 1 = none for the others, where 2 and 4
        //  measured +-0.1 %; Acrobot x4: -6 %.  profiles/r04_maxilp_classic.txt)
#pragma unroll E::ROLLOUT_UNROLL
        for (int t = 0; t < T; t++) {
            if (!HasStepDraws<E>::value && (t & (kRefillPeriod - 1)) == 0 && !q.have) q.refill();
            typename E::Act a;
            if (SAMPLE) {
                a = action_of_state<E>(astate);
                astate = as.jump_n.mult * astate + as.jump_n.plus;
                if (FULL || io.actions_out) static_cast<typename E::Act *>(io.actions_out)[t * N + i] = a;
            } else {
                a = static_cast<const typename E::Act *>(io.actions_in)[t * N + i];
            }
            StepOut<E> o;
            if (MODE == MI_AUTORESET_NEXT_STEP)
                lane_step_fused<E, !SAMPLE>(d, L, a, o, st, q);
            else
                lane_step<E, MODE>(d, i, L, a, o, st, &q);
            if (FULL || io.obs) store_row<E::OBS>(static_cast<float *>(io.obs) + (t * N + i) * E::OBS, o.obs);
            if (FULL || io.reward) io.reward[t * N + i] = o.reward;
            if (FULL || io.terminated) io.terminated[t * N + i] = o.terminated;
            if (FULL || io.truncated) io.truncated[t * N + i] = o.truncated;
        }
        store_lane<E>(d, i, L);
        if (q.have) {  // hand the unconsumed draws back to the env's generator
#pragma unroll
            for (int k = 0; k < E::NDRAWS; k++) q.rng.unstep();
        }
        store_rng_state(d, i, q.rng);
        if (SAMPLE && as.lane) {  // (the addresses from an opaque copy of i: the compiler otherwise keeps the load's 64-bit addresses live through the loop)
            int w = i;
            hold_opaque(w);
            as.lane[w] = (uint64_t)(astate >> 64), as.lane[(size_t)d.N + w] = (uint64_t)astate;
        }
    }
    block_accumulate(d, st);
}

// mi_rollout_infos: rollout_kernel's loop (FULL = false) that also stores, per step, what step() returns besides the trajectory -- the finished episodes'
// return / length rows and, under SAME_STEP, the final observations; zeros in the rows that finished nothing (RolloutExtra).  A kernel of its own, so that
// rollout_kernel's instantiations stay the code they are; the one-role kernel on purpose -- the two-role kernel's env role has no registers to spare for
// a second observation row, and its aux role would have to be handed it through the ring.  Any change to rollout_kernel's loop belongs here too
// (tests/test_gpu_rollout_infos.py compares the two through step()).
template <class E, int MODE, bool SAMPLE>
__global__ __launch_bounds__(kBlock) void rollout_infos_kernel(DevEnv d, RolloutPtrs io, ActionStream as, int T, AttrDev at, RolloutExtra ex) {
    constexpr bool FULL = false;
    tables_init<E>();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    if (i < d.N) {
        Lane<E> L;
        load_lane<E>(d, i, L);
        {  // the lane's attributes and what they make invariant, once per launch (no-op for the types without attributes)
            AttrRequest<E> ar;
            ar.request(at, d, i);
            ar.arrive(L.trig);
        }
        u128 astate = 0;
        const u128 ainc = make_u128(as.inc_hi, as.inc_lo);
        if (SAMPLE) {
            if (as.lane_valid) {  // the lane's state from the last launch (or act_init_kernel)
                astate = make_u128(as.lane[i], as.lane[(size_t)d.N + i]);
            } else {  // skip ahead by (i + 1) draws: one affine map per set bit of (i + 1)
                astate = make_u128(as.state_hi, as.state_lo);
                uint32_t delta = (uint32_t)i + 1u;
                for (int j = 0; delta; j++, delta >>= 1)
                    if (delta & 1u) astate = as.pow2[j].mult * astate + as.pow2[j].plus;
            }
        }
        (void)ainc;
        const size_t N = (size_t)d.N;
        ResetQueue<E> q;
        q.have = 0u;
        q.rng = load_rng(d, i);
        // (per-kind unroll factor: 2 for Acrobot -- its long loop body schedules better as two steps, +4.6 %; 1 = none for the others, where 2 and 4
        //  measured +-0.1 %; Acrobot x4: -6 %.  profiles/r04_maxilp_classic.txt)
#pragma unroll E::ROLLOUT_UNROLL
        for (int t = 0; t < T; t++) {
            if (!HasStepDraws<E>::value && (t & (kRefillPeriod - 1)) == 0 && !q.have) q.refill();
            typename E::Act a;
            if (SAMPLE) {
                a = action_of_state<E>(astate);
                astate = as.jump_n.mult * astate + as.jump_n.plus;
                if (FULL || io.actions_out) static_cast<typename E::Act *>(io.actions_out)[t * N + i] = a;
            } else {
                a = static_cast<const typename E::Act *>(io.actions_in)[t * N + i];
            }
            StepOut<E> o;
            if (MODE == MI_AUTORESET_SAME_STEP) {  // (lane_step writes the row only when the episode ended)
#pragma unroll
                for (int k = 0; k < E::OBS; k++) o.final_obs[k] = 0.0f;
            }
            if (MODE == MI_AUTORESET_NEXT_STEP)
                lane_step_fused<E, !SAMPLE>(d, L, a, o, st, q);
            else
                lane_step<E, MODE>(d, i, L, a, o, st, &q);
            if (FULL || io.obs) store_row<E::OBS>(static_cast<float *>(io.obs) + (t * N + i) * E::OBS, o.obs);
            if (FULL || io.reward) io.reward[t * N + i] = o.reward;
            if (FULL || io.terminated) io.terminated[t * N + i] = o.terminated;
            if (FULL || io.truncated) io.truncated[t * N + i] = o.truncated;
            // lanes are consecutive sub-environments: coalesced rows at [t * N + i], like the stores above
            if (ex.ep_ret) ex.ep_ret[t * N + i] = o.ep_ret;
            if (ex.ep_len) ex.ep_len[t * N + i] = o.ep_len;
            if (MODE == MI_AUTORESET_SAME_STEP && ex.final_obs) store_row<E::OBS>(static_cast<float *>(ex.final_obs) + (t * N + i) * E::OBS, o.final_obs);
        }
        store_lane<E>(d, i, L);
        if (q.have) {  // hand the unconsumed draws back to the env's generator
#pragma unroll
            for (int k = 0; k < E::NDRAWS; k++) q.rng.unstep();
        }
        store_rng_state(d, i, q.rng);
        if (SAMPLE && as.lane) {  // (the addresses from an opaque copy of i: the compiler otherwise keeps the load's 64-bit addresses live through the loop)
            int w = i;
            hold_opaque(w);
            as.lane[w] = (uint64_t)(astate >> 64), as.lane[(size_t)d.N + w] = (uint64_t)astate;
        }
    }
    block_accumulate(d, st);
}

// mi_set_step_wrappers: the loop of rollout_infos_kernel with lane_step_wrapped as its step, for mi_rollout (ex: all null) and mi_rollout_infos alike.
// The generator and StickyAction's state stay in registers for the launch; nothing is drawn ahead (lane_step_wrapped), so the generator that goes back
// to memory is at the reference's position.  actions_out are the policy's actions, not the effective ones.
// MAXSKIP (mi_set_max_and_skip): the lane's two frames are loaded once, live in registers across the T steps and are stored once.
template <class E, int MODE, bool SAMPLE, bool MAXSKIP = false>
__global__ __launch_bounds__(kBlock) void rollout_wrapped_kernel(DevEnv d, RolloutPtrs io, ActionStream as, int T, AttrDev at, RolloutExtra ex, WrapArg<MAXSKIP> w) {
    tables_init<E>();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    if (i < d.N) {
        Lane<E> L;
        load_lane<E>(d, i, L);
        {
            AttrRequest<E> ar;
            ar.request(at, d, i);
            ar.arrive(L.trig);
        }
        u128 astate = 0;
        if (SAMPLE) {
            if (as.lane_valid) {  // the lane's state from the last launch (or act_init_kernel)
                astate = make_u128(as.lane[i], as.lane[(size_t)d.N + i]);
            } else {  // skip ahead by (i + 1) draws: one affine map per set bit of (i + 1)
                astate = make_u128(as.state_hi, as.state_lo);
                uint32_t delta = (uint32_t)i + 1u;
                for (int j = 0; delta; j++, delta >>= 1)
                    if (delta & 1u) astate = as.pow2[j].mult * astate + as.pow2[j].plus;
            }
        }
        const size_t N = (size_t)d.N;
        ResetQueue<E> q;
        q.have = 0u;
        q.rng = load_rng(d, i);
        WrapLaneOf<E, MAXSKIP> sl;
        load_wrap_lane(w, i, sl);
        if constexpr (MAXSKIP) load_skip_lane(w, d, i, sl);
        for (int t = 0; t < T; t++) {
            typename E::Act a;
            if (SAMPLE) {
                a = action_of_state<E>(astate);
                astate = as.jump_n.mult * astate + as.jump_n.plus;
                if (io.actions_out) static_cast<typename E::Act *>(io.actions_out)[t * N + i] = a;
            } else {
                a = static_cast<const typename E::Act *>(io.actions_in)[t * N + i];
            }
            StepOut<E> o;
            if (MODE == MI_AUTORESET_SAME_STEP) {  // (lane_step_wrapped writes the row only when the episode ended)
#pragma unroll
                for (int k = 0; k < E::OBS; k++) o.final_obs[k] = 0.0f;
            }
            if constexpr (MAXSKIP) q.have = 0u;  // (nothing is drawn ahead here: said aloud, the queue's draws need no registers across the loop)
            lane_step_wrapped<E, MODE, MAXSKIP>(d, w, sl, i, L, a, o, st, &q, nullptr);
            if (io.obs) store_row<E::OBS>(static_cast<float *>(io.obs) + (t * N + i) * E::OBS, o.obs);
            if (io.reward) io.reward[t * N + i] = o.reward;
            if (io.terminated) io.terminated[t * N + i] = o.terminated;
            if (io.truncated) io.truncated[t * N + i] = o.truncated;
            if (ex.ep_ret) ex.ep_ret[t * N + i] = o.ep_ret;
            if (ex.ep_len) ex.ep_len[t * N + i] = o.ep_len;
            if (MODE == MI_AUTORESET_SAME_STEP && ex.final_obs) store_row<E::OBS>(static_cast<float *>(ex.final_obs) + (t * N + i) * E::OBS, o.final_obs);
        }
        if constexpr (MAXSKIP) {
            // the addresses of the launch's last stores from an opaque copy of i: the compiler otherwise keeps the 64-bit addresses of the loads at the
            // head of the kernel live through the loop (rollout_infos_kernel does the same for the action stream's rows).  With them Pendulum's sampled
            // rollout took 258 - 262 VGPRs -- past the 256 architectural ones values go to AGPRs, which the inline-asm Horner steps of ExactMath must
            // not sit next to (sincos_exact.h fma_k, tests/test_kernel_resources.py) --; without, 235 - 238.
            int wi = i;
            hold_opaque(wi);
            store_lane<E>(d, wi, L);
            store_wrap_lane(w, wi, sl);
            sl.written = 1u;  // (stored whether or not a slot was written: the rows it read, at worst)
            store_skip_lane(w, d, wi, sl);
            store_rng_state(d, wi, q.rng);  // (the queue is empty: nothing to hand back)
            if (SAMPLE && as.lane) as.lane[wi] = (uint64_t)(astate >> 64), as.lane[N + wi] = (uint64_t)astate;
        } else {
            store_lane<E>(d, i, L);
            store_wrap_lane(w, i, sl);
            if (q.have) {  // (a reset's refill is consumed by that reset: never taken, kept for the invariant)
#pragma unroll
                for (int k = 0; k < E::NDRAWS; k++) q.rng.unstep();
            }
            store_rng_state(d, i, q.rng);
            if (SAMPLE && as.lane) as.lane[i] = (uint64_t)(astate >> 64), as.lane[N + i] = (uint64_t)astate;
        }
    }
    block_accumulate(d, st);
}

// ---------------------------------------------------------------------------------------------------------
// The collector's rollout (NEXT_STEP, on-device policy, every output materialised) as TWO wavefronts per 64 sub-environments.
//
// At the benchmark's 65 536 sub-environments rollout_kernel puts ONE wavefront on every SIMD, and a wavefront that runs alone has nothing but
// its own independent instructions to cover a dependent instruction's latency: 0.63 of the issue slots are used (bench.py issue_bound), while
// the same kernel at 4 wavefronts per SIMD (262 144 lanes) reaches 0.6 of the HBM roofline instead of 0.43.  The sub-environments are the only
// parallelism the problem has, but a step is not one indivisible chain: the policy's action stream does not depend on the environment at all,
// and everything that happens to a step's results (episode return / length, the metric totals, five coalesced stores) is off the path that
// leads to the next state.  So a workgroup is 256 sub-environments and 512 lanes: wavefronts 0..3 ("env") integrate, decide termination /
// truncation / autoreset and produce the observation; wavefronts 4..7 ("aux"; wavefront w + 4 serves wavefront w and shares its SIMD: measured,
// the pairing (2j, 2j + 1) puts two env wavefronts on one SIMD and is 25 % slower) draw the actions ahead, keep the episode statistics and write
// the whole trajectory.  They meet through LDS rings, a chunk of DuoTraits::CHUNK steps at a time:
//   phase p:  aux draws the actions of chunk p -> A[p & 1] (and stores them);  env steps chunk p - 1 from A[(p - 1) & 1] -> O[(p - 1) & 1];
//             aux consumes O[p & 1] (chunk p - 2): bookkeeping and stores;  one workgroup barrier.
// The arithmetic of every value is the one of rollout_kernel / lane_step_fused (same operations on the same operands: bit-identical
// trajectories, tests/test_gpu_rollout_roles.py, tests/test_gpu_parity.py); only WHICH lane issues an instruction changed.  MI355ENV_ROLLOUT_DUO=0
// restores the one-role kernel.  The measurements behind every choice here: profiles/r04_two_role_rollout.txt, profiles/r04_ubench_valu_waves.txt.
constexpr int kDuoBlock = 2 * kBlock;
template <class E>
struct DuoTraits {
#ifdef MI_DUO_CHUNK_OVERRIDE  // (A/B builds: scripts/build_variant.py ... -DMI_DUO_CHUNK_OVERRIDE=8)
    static constexpr int CHUNK = MI_DUO_CHUNK_OVERRIDE;
#else
    static constexpr int CHUNK = E::DUO_CHUNK;  // steps per phase (envs_classic.h: measured per environment; 2 costs 10 .. 14 % in barriers)
#endif
};

// E::step_hooked (CartPole): the step's own rare branch also runs a caller's rare work (envs_classic.h)
template <class E, class = void>
struct HasRareHook : std::false_type {};
template <class E>
struct HasRareHook<E, std::void_t<decltype(E::RARE_HOOK)>> : std::integral_constant<bool, E::RARE_HOOK> {};

// The env role's bookkeeping cuts, measured per environment like DUO_ACT_AHEAD (envs_classic.h CartPoleT; an env type that does not name one keeps the
// parent's code): E::DUO_EPISODE_WORD, E::DUO_RAW_FLAGS, E::DUO_ENV_UNROLL
template <class E, class = void>
struct DuoEpisodeWord : std::false_type {};
template <class E>
struct DuoEpisodeWord<E, std::void_t<decltype(E::DUO_EPISODE_WORD)>> : std::integral_constant<bool, E::DUO_EPISODE_WORD> {};
template <class E, class = void>
struct DuoRawFlags : std::false_type {};
template <class E>
struct DuoRawFlags<E, std::void_t<decltype(E::DUO_RAW_FLAGS)>> : std::integral_constant<bool, E::DUO_RAW_FLAGS> {};
template <class E, class = void>
struct DuoEnvUnroll : std::integral_constant<int, 1> {};
template <class E>
struct DuoEnvUnroll<E, std::void_t<decltype(E::DUO_ENV_UNROLL)>> : std::integral_constant<int, E::DUO_ENV_UNROLL> {};
static_assert(mi_episode_word::kMetaFlagShift == kFlagShift && mi_episode_word::kMetaElapsedMask == kElapsedMask && mi_episode_word::kMetaNeedsReset == kNeedsReset,
              "episode_word.h restates the layout of `meta`");

// env role: lane_step_fused<E, false> without the episode statistics; `bits`: 1 terminated, 2 truncated, 4 this was the autoreset step
template <class E>
MI_DEV void duo_env_step(const DevEnv &d, Lane<E> &L, typename E::Act a, ResetQueue<E> &q, float obs[E::OBS], double &reward, uint32_t &bits) {
    const bool resetting = (L.flags & kNeedsReset) != 0;
    // rare: two episode ends within one refill period.  The refill only feeds the reset select after the step, so an environment with a rare
    // branch of its own takes it there, behind ONE exec-mask branch per step instead of two.
    const bool refill = resetting && !q.have;
    constexpr bool HOOK = HasRareHook<E>::value && !E::SPLIT_TERMINAL && !E::AUX_REWARD;
    if (!HOOK && __builtin_expect(refill, 0)) q.refill();
    const double (&rs)[E::S] = q.rs;
    const uint32_t rflags = ResetQueue<E>::reset_flags(L.flags & ~kNeedsReset);
    double rew;
    bool te;
    uint32_t sflags = L.flags;
    if constexpr (E::SPLIT_TERMINAL) {
        E::integrate(L.s, sflags, a, L.trig);
#pragma unroll
        for (int k = 0; k < E::S; k++) L.s[k] = resetting ? rs[k] : L.s[k];
        E::obs(L.s, sflags, obs, L.trig);
        E::terminal_after_obs(L.s, L.trig, rew, te);
    } else if constexpr (E::AUX_REWARD) {  // the aux role evaluates the reward (from E::aux_pre of the state before this step): the dynamics alone
        E::advance(L.s, a, d.P, L.trig);
        rew = 0.0, te = false;
    } else if constexpr (HOOK) {
        E::step_hooked(L.s, sflags, a, d.P, rew, te, L.trig, refill, [&]() __attribute__((always_inline)) {
            if (refill) q.refill();
        });
    } else {
        E::step(L.s, sflags, a, d.P, rew, te, L.trig);
    }
    const uint32_t elapsed = L.elapsed + 1u;  // TimeLimit.step (wrappers/common.py:129-133)
    const bool tr = d.max_steps > 0 && (int)elapsed >= d.max_steps;
    const bool done = !resetting && (te || tr);
    if constexpr (!E::SPLIT_TERMINAL) {
#pragma unroll
        for (int k = 0; k < E::S; k++) L.s[k] = resetting ? rs[k] : L.s[k];
    }
    L.flags = resetting ? rflags : (done ? (sflags | kNeedsReset) : sflags);
    L.elapsed = resetting ? 0u : elapsed;
    q.have = resetting ? 0u : q.have;
    if constexpr (!E::SPLIT_TERMINAL) E::obs(L.s, L.flags, obs, L.trig);
    reward = resetting ? 0.0 : rew;
    bits = (resetting ? 4u : 0u) | ((!resetting && te) ? 1u : 0u) | ((!resetting && tr) ? 2u : 0u);
}

// ... with the pending-autoreset flag, the TimeLimit counter and the queue's `have` in ONE word (E::DUO_EPISODE_WORD, episode_word.h): `ew` replaces
// L.flags' kNeedsReset (stripped by the caller for the launch), L.elapsed and q.have; `thr` is mi_episode_word::truncation_threshold(d.max_steps),
// computed once per launch.  The same decisions from the same integers: every test is one compare of the word (a TimeLimit that is off needs no
// `max_steps > 0` per step, and `truncated` needs no mask -- the word of an autoreset step is negative).  RAW (E::DUO_RAW_FLAGS): `bits` is the
// step's own terminated | truncated << 1, and the aux role masks an autoreset step's flags with the pending bit it carries itself.
template <class E, bool RAW>
MI_DEV void duo_env_step_word(const DevEnv &d, Lane<E> &L, typename E::Act a, ResetQueue<E> &q, uint32_t &ew, const int32_t thr, float obs[E::OBS], double &reward, uint32_t &bits) {
    namespace W = mi_episode_word;
    static_assert(!E::SPLIT_TERMINAL && !E::AUX_REWARD && !E::AUX_DERIVES_FLAGS, "measured for the plain env role only (CartPole)");
    const bool resetting = W::resetting(ew);
    const bool refill = W::refill(ew);  // (its `have` needs no update: the autoreset step that refills also empties the queue, step() below)
    constexpr bool HOOK = HasRareHook<E>::value;
    if (!HOOK && __builtin_expect(refill, 0)) q.refill();
    const double (&rs)[E::S] = q.rs;
    const uint32_t rflags = ResetQueue<E>::reset_flags(L.flags);
    double rew;
    bool te;
    uint32_t sflags = L.flags;
    if constexpr (HOOK) {
        E::step_hooked(L.s, sflags, a, d.P, rew, te, L.trig, refill, [&]() __attribute__((always_inline)) {
            if (refill) q.refill();
        });
    } else {
        E::step(L.s, sflags, a, d.P, rew, te, L.trig);
    }
    const bool tr = W::truncated(ew, thr);  // (ONE compare for the flag and for the word: W::raw_flags and W::step, with their common term shared)
#pragma unroll
    for (int k = 0; k < E::S; k++) L.s[k] = resetting ? rs[k] : L.s[k];
    L.flags = resetting ? rflags : sflags;
    ew = W::advance(ew, te || tr);
    E::obs(L.s, L.flags, obs, L.trig);
    reward = resetting ? 0.0 : rew;
    bits = RAW ? W::flag_bits(te, tr) : ((resetting ? 4u : 0u) | W::flag_bits(!resetting && te, tr));
}

// ... and the env role of an environment whose aux role derives the observation row and the flags from the state (E::AUX_DERIVES_FLAGS): the same
// step and autoreset select, then only the state words go over (E::aux_pack) -- no observation conversion, no flag word
template <class E>
MI_DEV void duo_env_step_state(const DevEnv &d, Lane<E> &L, typename E::Act a, ResetQueue<E> &q, double *w64, float *w32) {
    static_assert(!E::SPLIT_TERMINAL, "the split terminal test belongs to the observation, which this role does not take");
    const bool resetting = (L.flags & kNeedsReset) != 0;
    if (__builtin_expect(resetting && !q.have, 0)) q.refill();  // rare: two episode ends within one refill period
    const double (&rs)[E::S] = q.rs;
    const uint32_t rflags = ResetQueue<E>::reset_flags(L.flags & ~kNeedsReset);
    double rew;
    bool te;
    uint32_t sflags = L.flags;
    E::step(L.s, sflags, a, d.P, rew, te, L.trig);
    const uint32_t elapsed = L.elapsed + 1u;  // TimeLimit.step (wrappers/common.py:129-133)
    const bool tr = d.max_steps > 0 && (int)elapsed >= d.max_steps;
    const bool done = !resetting && (te || tr);
#pragma unroll
    for (int k = 0; k < E::S; k++) L.s[k] = resetting ? rs[k] : L.s[k];
    L.flags = resetting ? rflags : (done ? (sflags | kNeedsReset) : sflags);
    L.elapsed = resetting ? 0u : elapsed;
    q.have = resetting ? 0u : q.have;
    E::aux_pack(L.s, w64, w32);
}

// (Measured and not kept: the aux role split once more into "policy" and "book" wavefronts for three per SIMD: CartPole 78.9 us against 76.4 us --
//  more wavefronts do not help any more; s_setprio(3) for the env wavefronts: no change.  docs/classic_kernels.md)
template <class E>
__global__ __launch_bounds__(kDuoBlock) void rollout_duo_kernel(DevEnv d, RolloutPtrs io, ActionStream as, int T) {
    typedef typename E::Act Act;
    constexpr int ROLES = 2;
    constexpr int C = DuoTraits<E>::CHUNK;
    typedef Act ActLds;  // (a byte per Discrete action would save 28 KB of LDS at chunk 8 and costs 1 %: the widening on the env role)
    constexpr bool ACT_AHEAD = E::DUO_ACT_AHEAD;  // the env role requests step k + 1's action while step k runs (measured per environment, envs_classic.h)
    constexpr bool WORD = DuoEpisodeWord<E>::value, RAW = DuoRawFlags<E>::value;  // the env role's bookkeeping in one word; its flags unmasked (duo_env_step_word)
    static_assert(!RAW || WORD, "the unmasked flags are duo_env_step_word's");
    __shared__ ActLds sh_act[2][C + (ACT_AHEAD ? 1 : 0)][kBlock];  // (+ one row nobody writes: the env role's request for "the next step's action" after a chunk's last step)
    // what goes from the env role to the aux role: the observation row and a flag word -- or, for the environments whose aux role derives both from
    // the state (E::AUX_DERIVES_FLAGS, envs_classic.h), the state words
    constexpr bool DERIVE = E::AUX_DERIVES_FLAGS;
    static_assert(!DERIVE || E::REWARD_FROM_TERMINATED, "an aux role that derives the flags also derives the reward from them");
    constexpr int NF64 = E::AUX_F64 > 0 ? E::AUX_F64 : 1, NF32 = E::AUX_F32 > 0 ? E::AUX_F32 : 1;
    __shared__ double sh_w64[DERIVE ? 2 : 1][DERIVE ? C : 1][DERIVE ? kBlock : 1][NF64];
    __shared__ float sh_w32[(DERIVE && E::AUX_F32 > 0) ? 2 : 1][(DERIVE && E::AUX_F32 > 0) ? C : 1][(DERIVE && E::AUX_F32 > 0) ? kBlock : 1][NF32];
    __shared__ float sh_obs[DERIVE ? 1 : 2][DERIVE ? 1 : C][DERIVE ? 1 : kBlock][E::OBS];
    // (Measured and not kept: Pendulum with its reward -- three exact pow and an fmod, none of which feeds the next state -- evaluated by the aux role from
    //  the pre-step state passed through LDS: bit-identical, 168.7 us against 168.7 us for the one-role kernel.  Its instruction count is the limit.)
    constexpr bool AUXREW = E::AUX_REWARD;  // the aux role evaluates the reward from words about the state before the step (Pendulum)
    constexpr bool REW_OF_ACT = E::AUX_REWARD_OF_ACTION;  // ... or from the action it drew and the terminated flag (MountainCarContinuous)
    constexpr bool PASS_REWARD = !E::REWARD_FROM_TERMINATED && !AUXREW && !REW_OF_ACT;  // (not transferred when the aux role can compute it)
    __shared__ double sh_pre[AUXREW ? 2 : 1][AUXREW ? C : 1][AUXREW ? kBlock : 1][E::AUX_PRE];
    __shared__ double sh_rew[PASS_REWARD ? 2 : 1][PASS_REWARD ? C : 1][kBlock];
    // (the flag word's width is tuning, measured per environment at T = 128: CartPole +2.3 % with a dword, MountainCarContinuous +2.9 % with a byte)
    typedef typename std::conditional<E::REWARD_FROM_TERMINATED && E::OBS == 4, uint32_t, uint8_t>::type MI_DUO_FLAG_T;
    __shared__ MI_DUO_FLAG_T sh_bits[DERIVE ? 1 : 2][DERIVE ? 1 : C][DERIVE ? 1 : kBlock];
    __shared__ uint64_t sh_c[4][kBlock / 64];
    __shared__ double sh_r[kBlock / 64];
#ifdef MI_DUO_TIMING
    const unsigned long long t_begin = __builtin_readcyclecounter();  // (the prologue: tables, the roles' loads, the policy's start state)
#endif
    tables_init<E>();
    const int role = threadIdx.x / kBlock;  // wavefronts j (env), j + 4 (aux / policy) and j + 8 (book) share a SIMD and 64 sub-environments
    const bool is_env = role == 0, is_policy = role == 1, is_book = role == ROLES - 1;
    const int slot = threadIdx.x & (kBlock - 1);
    const int i = blockIdx.x * kBlock + slot;
    const bool active = i < d.N;
    const size_t N = (size_t)d.N;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    // env role
    Lane<E> L;
    ResetQueue<E> q;
    // WORD: pending | elapsed | have (episode_word.h) and the word's truncation threshold.  (Nothing of either for the other environments, not even a dead
    // `max_steps > 0`: it merges with the live ones of their step and moves them -- their kernels are the parent's, instruction for instruction.)
    uint32_t ew = 0u;
    const int32_t ew_thr = WORD ? mi_episode_word::truncation_threshold(d.max_steps) : 0;
    // aux role
    u128 astate = 0;
    double ep_ret = 0.0;
    int32_t ep_len = 0, ep_len_start = 0;  // (ep_len_start: 0 for a sub-environment whose first step is its autoreset step -- that episode was counted when it finished)
    uint32_t n_term = 0;
    uint32_t start_flags = 0;
    uint32_t aux_elapsed = 0, aux_needs_reset = 0;  // DERIVE: the aux role's own copy of the TimeLimit counter and of the pending-autoreset flag (RAW: of the flag)
    if (active) {
        if (is_env) {
            load_lane<E>(d, i, L);
            q.have = 0u;
            q.rng = load_rng(d, i);
            if constexpr (WORD) {  // (the flag word's other bits do not change during the launch: they rejoin when `meta` is stored)
                ew = mi_episode_word::encode((L.elapsed & kElapsedMask) | (L.flags << kFlagShift), 0u);
                L.flags &= ~kNeedsReset;
            }
        }
        if (is_book) {
            ep_ret = d.ep_ret[i], ep_len = d.ep_len[i];
            const uint32_t meta0 = d.meta[i];
            start_flags = meta0 >> kFlagShift;
            aux_elapsed = meta0 & kElapsedMask, aux_needs_reset = start_flags & kNeedsReset;
            ep_len_start = (start_flags & kNeedsReset) ? 0 : ep_len;
        }
        if (is_policy) {
            // The lane's state as the previous launch (or act_init_kernel) left it: two loads next to the book-keeping's.  Without it (the first
            // launch after mi_action_skip or after a seed or a launch inside a stream capture; a launch inside a capture) a skip-ahead by (i + 1)
            // draws, one affine map per set bit of (i + 1): 17 dependent trips to the pow2 table at 65 536 sub-environments, which the env role
            // waits for at the first barrier.
            if (as.lane_valid) {
                astate = make_u128(as.lane[i], as.lane[N + i]);
            } else {
                astate = make_u128(as.state_hi, as.state_lo);
                uint32_t delta = (uint32_t)i + 1u;
                for (int j = 0; delta; j++, delta >>= 1)
                    if (delta & 1u) astate = as.pow2[j].mult * astate + as.pow2[j].plus;
            }
        }
    }
    const int chunks = T / C;  // (the launcher sends a T that C does not divide to the one-role kernel)
#ifdef MI_DUO_TIMING
    unsigned long long t_work = 0, t_wait = 0, t_wait0 = 0, t_mark = __builtin_readcyclecounter();
    const unsigned long long t_prologue = t_mark - t_begin;
#endif
    // One phase of one role.  (Round 6, last cut: a loop per ROLE instead of one loop with both roles' code in it.  The values
    // a role keeps in scalar registers across the phases -- the env role's float64 constants, the aux role's pointers and multipliers -- were live through the
    // other role's code as well: Pendulum's bookkeeping loop reloaded 11 spilled scalars per step.  Both loops meet at the same number of barriers.)
    auto phase = [&](auto env_tag, const int p) __attribute__((always_inline)) {
        constexpr bool ENV = decltype(env_tag)::value;
        if (active) {
            if constexpr (ENV) {
                const int c = p - 1;
                if (c >= 0 && c < chunks) {
                    const int buf = c & 1;
                    // (rolled: with a partner wavefront on the SIMD the LDS read of the action at the top of a step is covered, and four copies
                    //  of the step body -- libm slow paths included -- are 30 KB of instruction cache: measured +5 % against the unrolled form)
                    // (the queue's periodic refill, rollout_kernel's `t % kRefillPeriod == 0`: with chunks that divide the period the test leaves the step loop)
                    constexpr bool REFILL_PER_CHUNK = kRefillPeriod % C == 0;
                    if constexpr (WORD) {
                        if (REFILL_PER_CHUNK && ((c * C) & (kRefillPeriod - 1)) == 0 && !mi_episode_word::have(ew)) q.refill(), ew = mi_episode_word::with_have(ew);
                    } else {
                        if (REFILL_PER_CHUNK && ((c * C) & (kRefillPeriod - 1)) == 0 && !q.have) q.refill();
                    }
                    // ACT_AHEAD: the action of step k + 1 is requested while step k runs -- the rolled loop otherwise starts every step with an LDS round trip
                    ActLds a_next = sh_act[buf][0][slot];
#ifdef MI_DUO_ENV_UNROLL  // (A/B builds: scripts/build_variant.py ... -DMI_DUO_ENV_UNROLL=2)
#pragma unroll MI_DUO_ENV_UNROLL
#else
#pragma unroll(DuoEnvUnroll<E>::value)  // (1 unless the environment measured otherwise, E::DUO_ENV_UNROLL: CartPole's 131-instruction step, whose rare paths are out of line, takes all 8)
#endif
                    for (int k = 0; k < C; k++) {
                        const int t = c * C + k;
                        if constexpr (WORD) {
                            if (!REFILL_PER_CHUNK && (t & (kRefillPeriod - 1)) == 0 && !mi_episode_word::have(ew)) q.refill(), ew = mi_episode_word::with_have(ew);
                        } else {
                            if (!REFILL_PER_CHUNK && (t & (kRefillPeriod - 1)) == 0 && !q.have) q.refill();
                        }
                        const Act a_k = ACT_AHEAD ? (Act)a_next : (Act)sh_act[buf][k][slot];
                        if (ACT_AHEAD) a_next = sh_act[buf][k + 1][slot];
                        if constexpr (DERIVE) {
                            double w64[NF64];
                            float w32[NF32];
                            duo_env_step_state<E>(d, L, a_k, q, w64, w32);
#pragma unroll
                            for (int j = 0; j < E::AUX_F64; j++) sh_w64[buf][k][slot][j] = w64[j];
#pragma unroll
                            for (int j = 0; j < E::AUX_F32; j++) sh_w32[buf][k][slot][j] = w32[j];
                        } else {
                            float o[E::OBS];
                            double rew;
                            uint32_t bits;
                            uint32_t pre_pending = 0u;  // E::AUX_PRE_SQUARES: which of pre[]'s leading entries are still arguments, not squares (bit j)
                            if constexpr (AUXREW) {  // (of a sub-environment in its autoreset step too: the aux role discards that reward)
                                double pre[E::AUX_PRE];
                                pre_pending = E::aux_pre(L.s, pre);
#pragma unroll
                                for (int j = 0; j < E::AUX_PRE; j++) sh_pre[buf][k][slot][j] = pre[j];
                            }
                            if constexpr (WORD)
                                duo_env_step_word<E, RAW>(d, L, a_k, q, ew, ew_thr, o, rew, bits);
                            else
                                duo_env_step<E>(d, L, a_k, q, o, rew, bits);
                            if constexpr (AUXREW && E::AUX_PRE_SQUARES > 0) bits |= pre_pending << 3;
#pragma unroll
                            for (int j = 0; j < E::OBS; j++) sh_obs[buf][k][slot][j] = o[j];
                            if constexpr (PASS_REWARD) sh_rew[buf][k][slot] = rew;
                            sh_bits[buf][k][slot] = (MI_DUO_FLAG_T)bits;
                        }
                    }
                }
            } else {
                const int c = p - 2;
                if (is_book && c >= 0) {  // what became of chunk c: episode statistics (RecordEpisodeStatistics order: the raw reward), totals, the trajectory rows
                    const int buf = c & 1;
                    if constexpr (AUXREW && E::AUX_PRE_SQUARES > 0) {
                        // The squares the env role could not take as plain products (flag bits 3 ..; 1 argument in 32): the exact pow routine, one pass per
                        // pending argument of this lane's chunk, all lanes of the wavefront side by side -- the wavefront runs as many passes as its
                        // unluckiest lane has pending arguments (2.7 on average for 2 x 8), not one per argument.  In place: a lane reads and writes
                        // only its own ring entries.
                        static_assert(E::AUX_PRE_SQUARES * C <= 32 && E::AUX_PRE_SQUARES <= 4 && sizeof(MI_DUO_FLAG_T) == 1, "pending bits: one word per chunk, bits 3 .. 6 of the flag byte");
                        uint32_t pend = 0u;
#pragma unroll
                        for (int k = 0; k < C; k++)
                            pend |= (((uint32_t)sh_bits[buf][k][slot] >> 3) & ((1u << E::AUX_PRE_SQUARES) - 1u)) << (E::AUX_PRE_SQUARES * k);
#pragma nounroll
                        while (pend) {
                            const int idx = __builtin_ctz(pend);
                            double *x = &sh_pre[buf][idx / E::AUX_PRE_SQUARES][slot][idx % E::AUX_PRE_SQUARES];
                            *x = E::aux_square(*x);
                            pend &= pend - 1u;
                        }
                    }
                    if constexpr (AUXREW) {
                        if constexpr (E::AUX_ACT_SQUARE) {
                            // ... and the float32 square of the (clipped) action the reward reads: the same scheme, in place in the action ring -- this chunk's
                            // actions were consumed by the env role a phase ago and the policy below refills this half only after the loop that follows
                            static_assert(C <= 32 && sizeof(ActLds) == sizeof(float), "one pending bit per step; the square takes the action's place");
                            uint32_t apend = 0u;
#pragma unroll
                            for (int k = 0; k < C; k++) {
                                const float u = E::act_square_arg((Act)sh_act[buf][k][slot]);
                                float h;
                                const bool plain = E::Math::sqf_is_plain(u, h);
                                sh_act[buf][k][slot] = (ActLds)(plain ? h : u);
                                apend |= plain ? 0u : 1u << k;
                            }
#pragma nounroll
                            while (apend) {
                                ActLds *x = &sh_act[buf][__builtin_ctz(apend)][slot];
                                *x = (ActLds)E::Math::sqf((float)*x);
                                apend &= apend - 1u;
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < C; k++) {
                        const size_t t = (size_t)c * C + k;
                        float o[E::OBS];
                        bool resetting, te, tr;
                        if constexpr (DERIVE) {
                            double w64[NF64];
                            float w32[NF32];
#pragma unroll
                            for (int j = 0; j < E::AUX_F64; j++) w64[j] = sh_w64[buf][k][slot][j];
#pragma unroll
                            for (int j = 0; j < E::AUX_F32; j++) w32[j] = sh_w32[buf][k][slot][j];
                            bool t0;
                            E::aux_unpack(w64, w32, d.P, o, t0);
                            // the vectoriser's state machine once more, on this role's own counters (sync_vector_env.py:277-329, wrappers/common.py:129-133):
                            // the same integers the env role holds, so the same flags
                            resetting = aux_needs_reset != 0;
                            const uint32_t el = aux_elapsed + 1u;
                            te = !resetting && t0;
                            tr = !resetting && d.max_steps > 0 && (int)el >= d.max_steps;
                            aux_elapsed = resetting ? 0u : el;
                            aux_needs_reset = (te || tr) ? 1u : 0u;
                        } else {
#pragma unroll
                            for (int j = 0; j < E::OBS; j++) o[j] = sh_obs[buf][k][slot][j];
                            const uint32_t bits = sh_bits[buf][k][slot];
                            if constexpr (RAW) {
                                // the env role's flags as its step raised them (terminated | truncated << 1; truncated is never raised in an autoreset
                                // step, terminated is the test of a state the reset replaced): this role's own pending bit masks them, and what is
                                // left is the next step's pending bit -- sync_vector_env.py:277-329 on the flags alone
                                resetting = aux_needs_reset != 0;
                                const uint32_t eff = mi_episode_word::effective_flags(aux_needs_reset, bits);
                                te = (eff & 1u) != 0, tr = (eff & 2u) != 0;
                                aux_needs_reset = eff;
                            } else {
                                resetting = (bits & 4u) != 0, te = (bits & 1u) != 0, tr = (bits & 2u) != 0;
                            }
                        }
                        double rew;
                        const bool done = te || tr;
                        if constexpr (E::REWARD_FROM_TERMINATED) {
                            // the reward is a function of the flags, so every total follows from three counters and the episode length (finish_totals,
                            // below): no float64 accumulation per step
                            rew = resetting ? 0.0 : E::reward_from_terminated(te, d.P);
                            // (an aux role that keeps its own TimeLimit counter needs no episode length per step: see the totals below.  Measured for
                            //  MountainCar: +3.8 %; for CartPole, with the counter handed over through LDS: -1 % -- profiles/r06_duo_three_changes_ab.txt)
                            if constexpr (!DERIVE) ep_len = resetting ? 0 : ep_len + 1;
                            st.reset_steps += resetting ? 1u : 0u;
                            st.episodes += done ? 1u : 0u;
                            n_term += te ? 1u : 0u;
                        } else {
                            if constexpr (AUXREW) {
                                double pre[E::AUX_PRE];
#pragma unroll
                                for (int j = 0; j < E::AUX_PRE; j++) pre[j] = sh_pre[buf][k][slot][j];
                                // (the action of this very step: chunk c was drawn two phases ago into the ring half the policy refills only AFTER this loop)
                                if constexpr (E::AUX_ACT_SQUARE)
                                    rew = resetting ? 0.0 : E::aux_reward_squared(pre, (float)sh_act[buf][k][slot]);  // (the ring holds the squares now, see above)
                                else
                                    rew = resetting ? 0.0 : E::aux_reward(pre, (Act)sh_act[buf][k][slot]);
                            } else if constexpr (REW_OF_ACT) {
                                rew = resetting ? 0.0 : E::reward_of_action(te, (Act)sh_act[buf][k][slot]);
                            } else {
                                rew = sh_rew[buf][k][slot];
                            }
                            const double ret = ep_ret + rew;
                            const int32_t len = ep_len + 1;
                            ep_ret = resetting ? 0.0 : ret;
                            ep_len = resetting ? 0 : len;
                            st.reset_steps += resetting ? 1u : 0u;
                            st.env_steps += resetting ? 0u : 1u;
                            st.episodes += done ? 1u : 0u;
                            st.return_sum += done ? ret : 0.0;
                            st.length_sum += done ? (uint64_t)len : 0ull;
                        }
                        store_row<E::OBS>(static_cast<float *>(io.obs) + (t * N + i) * E::OBS, o);
                        io.reward[t * N + i] = rew;
                        io.terminated[t * N + i] = te;
                        io.truncated[t * N + i] = tr;
                    }
                }
                if (is_policy && p < chunks) {  // the policy: action_space.sample() for chunk p (spaces/multi_discrete.py:176-178, spaces/box.py:463-465)
                    const int buf = p & 1;
#pragma unroll
                    for (int k = 0; k < C; k++) {
                        const size_t t = (size_t)p * C + k;
                        const Act a = action_of_state<E>(astate);
                        astate = as.jump_n.mult * astate + as.jump_n.plus;
                        sh_act[buf][k][slot] = (ActLds)a;
                        static_cast<Act *>(io.actions_out)[t * N + i] = a;
                    }
                }
            }
        }
#ifdef MI_DUO_TIMING
        {
            const unsigned long long now = __builtin_readcyclecounter();
            t_work += now - t_mark, t_mark = now;
        }
#endif
        __syncthreads();
#ifdef MI_DUO_TIMING
        {
            const unsigned long long now = __builtin_readcyclecounter();
            if (p == 0) t_wait0 = now - t_mark;  // phase 0: the env role has nothing to step and waits for the policy's first chunk
            t_wait += now - t_mark, t_mark = now;
        }
#endif
    };
    if (__builtin_amdgcn_readfirstlane((int)is_env)) {  // (a role is a whole number of wavefronts: the branch is uniform)
#pragma unroll 1
        for (int p = 0; p < chunks + 2; p++) phase(std::true_type(), p);
    } else {
#pragma unroll 1
        for (int p = 0; p < chunks + 2; p++) phase(std::false_type(), p);
    }
#ifdef MI_DUO_TIMING  // scripts/r04/duo_timing.py: where each role's time goes
    if (blockIdx.x == 7 && (threadIdx.x & 63) == 0)
        printf("duo timing: wave %d (role %d) prologue %llu work %llu wait-at-barrier %llu (phase 0: %llu) cycles over %d phases\n", (int)(threadIdx.x >> 6), role,
               t_prologue, t_work, t_wait, t_wait0, chunks + 2);
#endif
    if (active) {
        if (is_env) {
            // (ep_ret / ep_len belong to the aux role: store_lane without them)
#pragma unroll
            for (int k = 0; k < E::S; k++) d.state[(size_t)k * d.N + i] = L.s[k];
            if constexpr (WORD) d.meta[i] = mi_episode_word::decode_meta(ew, L.flags), q.have = mi_episode_word::have(ew);
            else d.meta[i] = (L.elapsed & kElapsedMask) | (L.flags << kFlagShift);
            if (q.have) {  // hand the unconsumed draws back to the env's generator
#pragma unroll
                for (int k = 0; k < E::NDRAWS; k++) q.rng.unstep();
            }
            store_rng_state(d, i, q.rng);
        } else if (is_book) {
            if constexpr (E::REWARD_FROM_TERMINATED) {
                // The totals of the launch from the counters.  Every env-step lengthens exactly one episode by one, so the lengths of the episodes
                // that FINISHED add up to the env-steps taken plus what the running episode had at the start minus what it has now; and with a
                // reward that is r_T on the terminating step and r_N on every other one (E::reward_from_terminated: +-1 / 0 -- sums of such values are
                // exact in float64 in any order) the finished episodes' returns are r_N (lengths - terminations) + r_T terminations, the running
                // episode's return r_N x its length.  Same numbers as the step-by-step accumulation of rollout_kernel, bit for bit.
                const double r_n = E::reward_from_terminated(false, d.P), r_t = E::reward_from_terminated(true, d.P);
                // how the LAST step ended: its flags are still in the ring (nothing is carried through the phases for this)
                bool last_done, last_te;
                if constexpr (DERIVE) {  // (this role's own flag; whether the finishing step terminated: the last state is still in the ring)
                    double w64[NF64];
                    float w32[NF32], o[E::OBS];
#pragma unroll
                    for (int j = 0; j < E::AUX_F64; j++) w64[j] = sh_w64[((chunks > 0 ? chunks : 1) - 1) & 1][C - 1][slot][j];
#pragma unroll
                    for (int j = 0; j < E::AUX_F32; j++) w32[j] = sh_w32[((chunks > 0 ? chunks : 1) - 1) & 1][C - 1][slot][j];
                    bool t0;
                    E::aux_unpack(w64, w32, d.P, o, t0);
                    last_done = aux_needs_reset != 0, last_te = last_done && t0;
                } else {
                    // (RAW: the ring holds the unmasked flags; the masked ones of the last step are this role's pending word)
                    const uint32_t last_bits = chunks > 0 ? (RAW ? aux_needs_reset : (uint32_t)sh_bits[(chunks - 1) & 1][C - 1][slot]) : ((start_flags & kNeedsReset) ? 2u : 0u);
                    last_done = (last_bits & 3u) != 0, last_te = (last_bits & 1u) != 0;
                }
                // DERIVE: the running episode's length is the TimeLimit counter once an autoreset step has zeroed both (they advance together from
                // there), and what it was plus the launch's steps otherwise
                if (DERIVE && chunks > 0) ep_len = st.reset_steps ? (int32_t)aux_elapsed : ep_len + chunks * C;
                st.env_steps = (uint32_t)(chunks * C) - st.reset_steps;
                // (an episode that finished in the very last step still sits in ep_len, waiting for its autoreset step: it IS among the finished ones)
                st.length_sum = (uint64_t)((int64_t)st.env_steps + (int64_t)ep_len_start - (last_done ? (int64_t)0 : (int64_t)ep_len));
                st.return_sum = r_n * (double)((int64_t)st.length_sum - (int64_t)n_term) + r_t * (double)n_term;
                st.return_sum = st.episodes ? st.return_sum : 0.0;  // (no finished episode: +0.0 like the accumulation, whatever the signs of r_n, r_t)
                ep_ret = (last_done && last_te) ? r_n * (double)(ep_len - 1) + r_t : r_n * (double)ep_len;
                if (chunks == 0) ep_ret = d.ep_ret[i];
            }
            d.ep_ret[i] = ep_ret, d.ep_len[i] = ep_len;
        }
        if (is_policy && as.lane) {  // after the last jump: the next launch's start (addresses from an opaque i, as in rollout_kernel)
            int w = i;
            hold_opaque(w);
            as.lane[w] = (uint64_t)(astate >> 64), as.lane[N + w] = (uint64_t)astate;
        }
    }
    // the workgroup's totals (block_accumulate for several roles: only the book-keeping wavefronts carry any)
    const int wave = slot >> 6, lane = threadIdx.x & 63;
    if (is_book) {
        const uint32_t c0 = wave_sum(st.env_steps), c1 = wave_sum(st.reset_steps), c2 = wave_sum(st.episodes);
        const uint64_t c3 = c2 ? wave_sum(st.length_sum) : 0;
        const double r = c2 ? wave_sum(st.return_sum) : 0.0;
        if (lane == 0) sh_c[0][wave] = c0, sh_c[1][wave] = c1, sh_c[2][wave] = c2, sh_c[3][wave] = c3, sh_r[wave] = r;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) t += sh_c[threadIdx.x][w];
        if (t) d.blk_count[(size_t)blockIdx.x * 4 + threadIdx.x] += t;
    } else if (threadIdx.x == 64) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) t += sh_r[w];
        if (t != 0.0) d.blk_ret[blockIdx.x] += t;
    }
}

// ---------------------------------------------------------------------------------------------------------
// MI_CFG_SHARED_RNG: the reference's NumPy vector environment CartPoleVectorEnv (cartpole.py:353-505) -- one generator for all sub-environments,
// drawn component-major over the sub-environments that reset (see include/mi355env.h).  Same dynamics (E::step), other bookkeeping.
// ---------------------------------------------------------------------------------------------------------
MI_DEV u128 shared_advance(const SharedRng &sr, u128 state, uint64_t n) {  // `state` n steps further along the base generator's sequence
    for (int j = 0; n; j++, n >>= 1)
        if (n & 1ull) state = sr.pow2[j].mult * state + sr.pow2[j].plus;
    return state;
}
// The draws of one workgroup start at a position every lane shares (the call's first draw + the component's stride + the workgroup's prefix) and differ by
// less than the workgroup size: threads 0..3 skip ahead to the four shared positions (tens of 128-bit multiply-adds, once per workgroup, through LDS) and a
// lane adds its own offset < 256 (at most eight).  Call from every thread, before a __syncthreads(); `stride` = draws between two components.
MI_DEV void shared_block_bases(const SharedRng &sr, uint64_t first, uint64_t stride, uint64_t (*sh)[2]) {
    if (threadIdx.x < 4) {
        const u128 s = shared_advance(sr, make_u128(sr.words[0], sr.words[1]), first + (uint64_t)threadIdx.x * stride);
        sh[threadIdx.x][0] = (uint64_t)(s >> 64), sh[threadIdx.x][1] = (uint64_t)s;
    }
}
MI_DEV double shared_draw_from(const SharedRng &sr, const uint64_t (*sh)[2], int c, uint32_t offset) {  // draw `offset` after the workgroup's base of component c
    Pcg64 g;
    g.state = shared_advance(sr, make_u128(sh[c][0], sh[c][1]), offset), g.inc = make_u128(sr.words[2], sr.words[3]);
    return g.next_double();
}

// One workgroup, before every reset (fixed_draws = 4 N) / step (fixed_draws = 0: 4 k, k = the sub-environments that finished in the previous step):
// exclusive scan of the per-workgroup counts, and the stream bookkeeping -- the call in flight draws from pos_base, the next one after it.
// CartPoleVectorEnv.step asserts `self.action_space.contains(action)` for the WHOLE batch before it touches a sub-environment or the generator
// (cartpole.py:424-426).  A device caller's batch is checked by this pre-pass: one bad action marks the batch refused, and the scan / step kernels
// of this and of every later call return at once (no draw consumed, no sub-environment stepped) until the host has raised the error (raise_device_error).
template <class E>
__global__ __launch_bounds__(kBlock) void shared_validate_kernel(DevEnv d, const typename E::Act *actions, SharedRng sr) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < d.N && !E::valid(actions[i])) {
        *d.error = kErrInvalidAction;
        sr.words[7] = 1;
    }
}

__global__ __launch_bounds__(kBlock) void shared_scan_kernel(SharedRng sr, int grid, uint64_t fixed_draws) {
    __shared__ uint32_t wave_total[kBlock / 64];
    if (!fixed_draws && sr.words[7]) return;  // a refused batch (uniform)
    const int per = (grid + kBlock - 1) / kBlock, lo = threadIdx.x * per, hi = min(grid, lo + per);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t sum = 0;
    if (!fixed_draws)
        for (int b = lo; b < hi; b++) sum += sr.blk_done[b];
    // inclusive scan of the threads' chunk totals: Hillis-Steele inside each wavefront (cross-lane reads, no LDS round trips), the four wavefront totals through LDS
    uint32_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; w++) {
        before += w < wave ? wave_total[w] : 0u;
        total += wave_total[w];
    }
    if (threadIdx.x == 0) {
        const uint64_t consumed = sr.words[4];
        sr.words[5] = consumed, sr.words[6] = total;
        sr.words[4] = consumed + (fixed_draws ? fixed_draws : 4ull * total);
    }
    if (!fixed_draws) {
        uint32_t run = before + incl - sum;  // exclusive prefix of this thread's chunk
        for (int b = lo; b < hi; b++) {
            const uint32_t c = sr.blk_done[b];
            sr.blk_prefix[b] = run, run += c;
        }
    }
}

MI_DEV void shared_store_done_count(const SharedRng &sr, bool done) {  // this workgroup's entry of blk_done for the next step's scan
    __shared__ uint32_t sh[kBlock / 64];
    const uint64_t bal = __ballot(done);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) t += sh[w];
        sr.blk_done[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kBlock) void shared_count_kernel(DevEnv d, SharedRng sr) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    shared_store_done_count(sr, i < d.N && ((d.meta[i] >> kFlagShift) & kNeedsReset));
}

// reset(): state[c][i] = uniform(low, high) from draw c * N + i (cartpole.py:493-500: size=(4, N))
template <class E>
__global__ __launch_bounds__(kBlock) void shared_reset_kernel(DevEnv d, SharedRng sr, float *obs) {
    __shared__ uint64_t sh_base[4][2];
    static_assert(E::NDRAWS == 4, "four state components: threads 0..3 prepare their bases");
    tables_init<E>();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    shared_block_bases(sr, sr.words[5] + (uint64_t)blockIdx.x * kBlock, (uint64_t)d.N, sh_base);
    __syncthreads();
    if (i < d.N) {
        Lane<E> L;
        load_lane<E>(d, i, L);
        double u[E::NDRAWS];
#pragma unroll
        for (int c = 0; c < E::NDRAWS; c++) u[c] = shared_draw_from(sr, sh_base, c, threadIdx.x);
        L.flags = 0;
        E::reset_u(u, L.s, L.flags, sr.low, sr.high);
        L.elapsed = 0, L.ep_ret = 0.0, L.ep_len = 0;
        store_lane<E>(d, i, L);
        if (obs) {
            float o[E::OBS];
            E::obs(L.s, L.flags, o, L.trig);
            store_row<E::OBS>(obs + (size_t)i * E::OBS, o);
        }
    }
    shared_store_done_count(sr, false);
}

// step() (cartpole.py:421-479): a sub-environment that finished in the PREVIOUS step takes the j-th column of uniform(low, high, size=(4, k)) --
// j = its rank among the k such sub-environments, in index order: workgroup prefix (scan kernel) + wavefront ballots -- with steps 0, reward 0, not
// done; every other one integrates.  `-np.array(terminated, dtype=np.float32)` makes the Sutton-Barto reward of a surviving pole -0.0 (:466).
template <class E>
__global__ __launch_bounds__(kBlock) void shared_step_kernel(DevEnv d, StepPtrs io, SharedRng sr) {
    __shared__ uint32_t sh_wave[kBlock / 64];
    __shared__ uint64_t sh_base[4][2];
    static_assert(E::NDRAWS == 4, "four state components: threads 0..3 prepare their bases");
    if (sr.words[7]) return;  // a refused batch (shared_validate_kernel): nothing is touched, blk_done keeps the previous step's counts
    tables_init<E>();
    const int i = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (sr.blk_done[blockIdx.x]) shared_block_bases(sr, sr.words[5] + (uint64_t)sr.blk_prefix[blockIdx.x], sr.words[6], sh_base);  // (workgroup-uniform test)
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    Lane<E> L;
    const bool active = i < d.N;
    if (active) load_lane<E>(d, i, L);
    const bool resetting = active && (L.flags & kNeedsReset);
    const uint64_t bal = __ballot(resetting);
    if (lane == 0) sh_wave[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) rank += sh_wave[w];
    bool done = false;
    if (active) {
        double rew = 0.0, ep_ret = 0.0;
        int32_t ep_len = 0;
        bool te = false, tr = false, untouched = false;
        if (resetting) {
            double u[E::NDRAWS];
#pragma unroll
            for (int c = 0; c < E::NDRAWS; c++) u[c] = shared_draw_from(sr, sh_base, c, rank);  // draw c * k + (workgroup prefix + rank) of this call
            L.flags = 0;
            E::reset_u(u, L.s, L.flags, sr.low, sr.high);
            L.elapsed = 0, L.ep_ret = 0.0, L.ep_len = 0;
            st.reset_steps++;
        } else {
            const typename E::Act a = static_cast<const typename E::Act *>(io.actions)[i];
            if (!E::valid(a)) {  // cartpole.py:424-426 asserts before it touches anything: the sticky error word, this sub-environment untouched
                *d.error = kErrInvalidAction;
                untouched = true;
            } else {
                E::step(L.s, L.flags, a, d.P, rew, te, L.trig);
                if (d.P.p[0] != 0.0 && !te) rew = -0.0;
                L.elapsed += 1;
                tr = d.max_steps > 0 && (int)L.elapsed >= d.max_steps;  // self.steps >= self.max_episode_steps (:461)
                L.ep_ret += rew, L.ep_len += 1;
                st.env_steps++;
                done = te || tr;
                if (done) {
                    ep_ret = L.ep_ret, ep_len = L.ep_len;
                    st.episodes++, st.return_sum += L.ep_ret, st.length_sum += (uint64_t)L.ep_len;
                    L.flags |= kNeedsReset;  // self.prev_done (:479)
                }
            }
        }
        if (!untouched) store_lane<E>(d, i, L);
        float o[E::OBS];
        E::obs(L.s, L.flags, o, L.trig);
        if (io.obs) store_row<E::OBS>(io.obs + (size_t)i * E::OBS, o);
        if (io.reward) io.reward[i] = rew;
        if (io.terminated) io.terminated[i] = te;
        if (io.truncated) io.truncated[i] = tr;
        if (io.ep_ret) io.ep_ret[i] = ep_ret;
        if (io.ep_len) io.ep_len[i] = ep_len;
    }
    shared_store_done_count(sr, done);
    block_accumulate(d, st);
}

// the policy of a shared-generator rollout's step t: draw t * N + i of the batched action space's stream (what rollout_kernel computes inline)
template <class E>
__global__ __launch_bounds__(kBlock) void shared_sample_kernel(DevEnv d, ActionStream as, int t, typename E::Act *out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.N) return;
    u128 s = make_u128(as.state_hi, as.state_lo);
    uint64_t n = (uint64_t)t * (uint64_t)d.N + (uint64_t)i + 1ull;
    for (int j = 0; n; j++, n >>= 1)
        if (n & 1ull) s = as.pow2[j].mult * s + as.pow2[j].plus;
    out[i] = action_of_state<E>(s);
}

}  // namespace
#endif  // MI355ENV_CLASSIC_KERNELS_H
