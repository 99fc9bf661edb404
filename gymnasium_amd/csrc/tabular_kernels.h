// tabular_kernels.h -- the ToyText family's device code: the finite MDPs (FrozenLake, CliffWalking, Taxi with and without the fickle passenger) and
// Blackjack, which rides on the same kernels.  The per-step kernels (tab_step_kernel, tab_reset_kernel), the fused rollouts (tab_rollout_kernel per
// kind, tab_rollout_lean_kernel with the table in LDS, bj_rollout_lean_kernel) and what their launch sites need (TabStepPtrs, TabLeanCell,
// tab_lean_lds_bytes).  Included by tabular.hip only, which holds the host code that launches them: they run on the default scheduler (max-ILP cost
// them 1 - 2 %, profiles/r04_maxilp_classic.txt).
#ifndef MI355ENV_TABULAR_KERNELS_H
#define MI355ENV_TABULAR_KERNELS_H
#include "engine_types.h"
#include "lane_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// ToyText: finite MDPs.  state row = {state index, probability of the last transition}; integer lookups only.
//   step:  i = argmax(cumsum(p) > rng.random()) (toy_text/utils.py:4-8), then P[s][a][i]  (frozen_lake.py:324-335)
//   reset: s = argmax(cumsum(initial_state_distrib) > rng.random())                        (frozen_lake.py:337-348)
// ---------------------------------------------------------------------------------------------------------
MI_DEV int tab_categorical(const double *csprob, int n, Pcg64 &rng) {
    const double u = rng.next_double();
    // first index with csprob[k] > u (np.argmax(np.cumsum(p) > u); 0 when there is none).  The first entries by scan -- transition rows
    // have <= 3 outcomes, FrozenLake / CliffWalking start in state 0 -- the rest of a long row (Taxi's 500-state initial distribution) by
    // bisection, valid because cumulative sums are non-decreasing: 8 probes instead of a scan that costs a wavefront its slowest lane.
    const int head = n < 4 ? n : 4;
    for (int k = 0; k < head; k++)
        if (csprob[k] > u) return k;
    int lo = head, hi = n;  // invariant: csprob[k] <= u for k < lo, csprob[k] > u for k >= hi
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (csprob[mid] > u)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo < n ? lo : 0;
}
struct TabLane {
    double s, prob;
    double aux;  // Taxi with fickle_passenger only: fickle_step | the generator's buffered 32-bit half << 1 (third state row)
    uint32_t elapsed, flags;
    double ep_ret;
    int32_t ep_len;
};
// Taxi's fickle passenger (taxi.py:436-451, :462-464): params[2] != 0 switches the rule on, params[3] = fickle_probability
MI_DEV bool tab_fickle(const DevEnv &d) { return d.tab_fickle_rows != 0; }
// The tabular kernels serve three kinds of environment (a plain transition table, Taxi with the fickle passenger, Blackjack) behind run-time tests; the
// fused rollout is instantiated per kind (TK: kTabPlain / kTabFickle / kTabBlackjack; kTabAny = decide at run time, the per-step kernels), so that a
// FrozenLake rollout carries neither Blackjack's dealer loop nor Taxi's re-draw (round 6: the kernel issues one instruction per ~5 cycles, profiles/r06_acrobot_toytext_root_cause.txt).
enum { kTabAny = -1, kTabPlain = 0, kTabFickle = 1, kTabBlackjack = 2 };
template <int TK>
MI_DEV bool tab_is_fickle(const DevEnv &d) { return TK == kTabAny ? d.tab_fickle_rows != 0 : TK == kTabFickle; }
template <int TK = kTabAny>
MI_DEV void tab_load(const DevEnv &d, int i, TabLane &L) {
    L.s = d.state[i], L.prob = d.state[(size_t)d.N + i];
    L.aux = tab_is_fickle<TK>(d) ? d.state[(size_t)2 * d.N + i] : 0.0;
    const uint32_t m = d.meta[i];
    L.elapsed = m & kElapsedMask, L.flags = m >> kFlagShift;
    L.ep_ret = d.ep_ret[i], L.ep_len = d.ep_len[i];
}
template <int TK = kTabAny>
MI_DEV void tab_store(const DevEnv &d, int i, const TabLane &L) {
    d.state[i] = L.s, d.state[(size_t)d.N + i] = L.prob;
    if (tab_is_fickle<TK>(d)) d.state[(size_t)2 * d.N + i] = L.aux;
    d.meta[i] = (L.elapsed & kElapsedMask) | (L.flags << kFlagShift);
    d.ep_ret[i] = L.ep_ret, d.ep_len[i] = L.ep_len;
}
// ---- Blackjack-v1 (gymnasium/envs/toy_text/blackjack.py:17-232) rides on the tabular kernels (d.tab.nS < 0) --------------
// state word  = player raw sum | has-ace << 6 | two-cards << 7 | dealer card 0 << 8 | dealer card 1 << 12
// second word = the generator's buffered 32-bit half (1 << 32 | value; 0 = empty): draw_card is np_random.choice(deck) =
// Lemire's bounded uint32 on next_uint32, and PCG64's next_uint32 hands out the low, then the high half of one 64-bit output.
MI_DEV bool is_blackjack(const DevEnv &d) { return d.tab.nS < 0; }
template <int TK>
MI_DEV bool tab_is_blackjack(const DevEnv &d) { return TK == kTabAny ? d.tab.nS < 0 : TK == kTabBlackjack; }
MI_DEV uint32_t bj_next32(Pcg64 &rng, double &aux_slot) {
    const uint64_t aux = (uint64_t)aux_slot;
    if (aux >> 32) {
        aux_slot = 0.0;
        return (uint32_t)aux;
    }
    const uint64_t x = rng.next64();
    aux_slot = (double)((1ull << 32) | (x >> 32));
    return (uint32_t)x;
}
MI_DEV uint32_t bj_bounded(Pcg64 &rng, double &aux, uint32_t n) {
    uint64_t m = (uint64_t)bj_next32(rng, aux) * n;
    uint32_t left = (uint32_t)m;
    if (left < n) {
        const uint32_t thr = (uint32_t)((0x100000000ull - n) % n);
        while (left < thr) m = (uint64_t)bj_next32(rng, aux) * n, left = (uint32_t)m;
    }
    return (uint32_t)(m >> 32);
}
MI_DEV int bj_card(Pcg64 &rng, double &aux) {  // deck = [1..10, 10, 10, 10]
    const uint32_t k = bj_bounded(rng, aux, 13);
    return k < 9 ? (int)k + 1 : 10;
}
MI_DEV int bj_sum_hand(int raw, int ace) { return (ace && raw + 10 <= 21) ? raw + 10 : raw; }
MI_DEV void bj_obs(double s, int64_t *o) {  // _get_obs: (player sum with a usable ace as 11, dealer's first card, usable ace)
    const int64_t p = (int64_t)s;
    const int psum = (int)(p & 63), pace = (int)((p >> 6) & 1);
    o[0] = bj_sum_hand(psum, pace), o[1] = (p >> 8) & 15, o[2] = pace && psum + 10 <= 21;
}
MI_DEV void bj_reset(Pcg64 &rng, double &s, double &aux) {  // blackjack.py:181-202 incl. the render-only suit / face draws
    const int d0 = bj_card(rng, aux), d1 = bj_card(rng, aux), p0 = bj_card(rng, aux), p1 = bj_card(rng, aux);
    (void)bj_bounded(rng, aux, 4);
    if (d0 == 10) (void)bj_bounded(rng, aux, 3);
    s = (double)((p0 + p1) | ((int)(p0 == 1 || p1 == 1) << 6) | (1 << 7) | (d0 << 8) | (d1 << 12));
}
MI_DEV void bj_step(Pcg64 &rng, double &s, double &aux, int64_t action, bool natural, bool sab, double &reward, bool &te) {  // :143-174
    const int64_t p = (int64_t)s;
    int psum = (int)(p & 63), pace = (int)((p >> 6) & 1), ptwo = (int)((p >> 7) & 1);
    const int d0 = (int)((p >> 8) & 15), d1 = (int)((p >> 12) & 15);
    if (action) {  // hit
        const int c = bj_card(rng, aux);
        psum += c, pace |= c == 1, ptwo = 0;
        te = bj_sum_hand(psum, pace) > 21;
        reward = te ? -1.0 : 0.0;
    } else {  // stick: the dealer draws to 17, then the hands are scored
        int dsum = d0 + d1, dace = d0 == 1 || d1 == 1, dtwo = 1;
        while (bj_sum_hand(dsum, dace) < 17) {
            const int c = bj_card(rng, aux);
            dsum += c, dace |= c == 1, dtwo = 0;
        }
        const int ph = bj_sum_hand(psum, pace), dh = bj_sum_hand(dsum, dace);
        const int ps = ph > 21 ? 0 : ph, ds = dh > 21 ? 0 : dh;
        te = true;
        reward = (double)(ps > ds) - (double)(ps < ds);
        const bool pnat = ptwo && pace && psum == 11, dnat = dtwo && dace && dsum == 11;  // sorted(hand) == [1, 10]
        if (sab && pnat && !dnat)
            reward = 1.0;
        else if (!sab && natural && pnat && reward == 1.0)
            reward = 1.5;
    }
    s = (double)(psum | (pace << 6) | (ptwo << 7) | (d0 << 8) | (d1 << 12));
}

// `held`: the lane's generator kept in registers by a fused rollout (loaded before its loop, stored after it); nullptr = the per-step
// kernels, which load and store the stream around every use.
template <int TK = kTabAny>
MI_DEV void tab_autoreset(const DevEnv &d, int i, TabLane &L, Pcg64 *held = nullptr) {
    Pcg64 local;
    if (!held) local = load_rng(d, i);
    Pcg64 &rng = held ? *held : local;
    if (tab_is_blackjack<TK>(d)) {
        bj_reset(rng, L.s, L.prob);
    } else {
        const size_t tb = d.tab.env_table ? (size_t)d.tab.env_table[i] : 0;  // the sub-environment's own table (its own random map, ...)
        L.s = (double)tab_categorical(d.tab.isd + tb * d.tab.nS, d.tab.nS, rng), L.prob = 1.0;
        if (tab_is_fickle<TK>(d)) {  // taxi.py:462-464: fickle_step = fickle_passenger and np_random.random() < fickle_probability -- one more draw
            const double flag = rng.next_double() < d.P.p[3] ? 1.0 : 0.0;
            L.aux = floor(L.aux * 0.5) * 2.0 + flag;
        }
    }
    if (!held) store_rng_state(d, i, rng);
    L.elapsed = 0, L.ep_ret = 0.0, L.ep_len = 0;
}
// observation row of a tabular lane: the state index, or Blackjack's three integers
template <int TK = kTabAny>
MI_DEV void tab_write_obs(const DevEnv &d, double s, int64_t *base, size_t row) {
    if (tab_is_blackjack<TK>(d))
        bj_obs(s, base + 3 * row);
    else
        base[row] = (int64_t)s;
}
template <int MODE, int TK = kTabAny>
MI_DEV void tab_lane_step(const DevEnv &d, int i, TabLane &L, int64_t a, int64_t &obs, int64_t &final_obs, bool &has_final, double &reward,
                          bool &te, bool &tr, double &out_ret, int32_t &out_len, LaneStats &st, Pcg64 *held = nullptr, double *final_prob = nullptr) {
    te = tr = false, reward = 0.0, has_final = false;
    if (MODE == MI_AUTORESET_NEXT_STEP && (L.flags & kNeedsReset)) {
        tab_autoreset<TK>(d, i, L, held);
        st.reset_steps++;
    } else if (MODE == MI_AUTORESET_DISABLED && (L.flags & kNeedsReset)) {
        *d.error = kErrDisabledStepped;
        obs = (int64_t)L.s, out_ret = 0.0, out_len = 0;
        return;
    } else {
        if (a < 0 || a >= d.tab.nA) {  // like the DISABLED case above: report, leave the lane untouched
            *d.error = kErrInvalidAction;
            obs = (int64_t)L.s, out_ret = 0.0, out_len = 0;
            return;
        }
        Pcg64 local;
        if (!held) local = load_rng(d, i);
        Pcg64 &rng = held ? *held : local;
        if (tab_is_blackjack<TK>(d)) {
            bj_step(rng, L.s, L.prob, a, d.P.p[0] != 0.0, d.P.p[1] != 0.0, reward, te);
            if (!held) store_rng_state(d, i, rng);
        } else {
            const size_t tb = d.tab.env_table ? (size_t)d.tab.env_table[i] : 0;
            const size_t cell = (tb * d.tab.nS + (size_t)L.s) * d.tab.nA + (size_t)a, row = cell * d.tab.K;
            const int k = tab_categorical(d.tab.csprob + row, d.tab.count[cell], rng);
            int next = d.tab.next[row + k];
            if (tab_is_fickle<TK>(d) && ((int64_t)L.aux & 1)) {
                // taxi.py:436-451: the passenger was in the taxi before this step (shadow pass_loc == 4) and the step moved the taxi: once per episode
                // the destination is re-drawn among the other three -- Generator.choice = a Lemire-bounded 32-bit draw on the buffered halves (bj_bounded)
                const int old = (int)L.s;
                const int srow = old / 100, scol = old / 20 % 5, spass = old / 4 % 5, sdest = old % 4;
                const int nrow = next / 100, ncol = next / 20 % 5, npass = next / 4 % 5;
                if (spass == 4 && (nrow != srow || ncol != scol)) {
                    double half = floor(L.aux * 0.5);
                    const int pick = (int)bj_bounded(rng, half, 3);
                    const int dest = pick + (pick >= sdest ? 1 : 0);  // possible_destinations = [i for i in range(4) if i != shadow_dest_idx]
                    L.aux = half * 2.0;                                // fickle_step = False
                    next = ((nrow * 5 + ncol) * 5 + npass) * 4 + dest;
                }
            }
            if (!held) store_rng_state(d, i, rng);
            L.s = (double)next, L.prob = d.tab.prob[row + k];
            reward = d.tab.reward[row + k], te = d.tab.term[row + k] != 0;
        }
        L.elapsed += 1;
        tr = d.max_steps > 0 && (int)L.elapsed >= d.max_steps;
        L.ep_ret += reward, L.ep_len += 1;
        st.env_steps++;
    }
    const bool done = te || tr;
    out_ret = done ? L.ep_ret : 0.0, out_len = done ? L.ep_len : 0;
    if (done) st.episodes++, st.return_sum += L.ep_ret, st.length_sum += (uint64_t)L.ep_len;
    if (MODE == MI_AUTORESET_SAME_STEP && done) {
        final_obs = (int64_t)L.s, has_final = true;
        if (final_prob) *final_prob = L.prob;  // info["prob"] of the finishing transition ("final_info"); the reset then reports prob = 1
        tab_autoreset<TK>(d, i, L, held);
    }
    obs = (int64_t)L.s;
    if (done && MODE != MI_AUTORESET_SAME_STEP)
        L.flags |= kNeedsReset;
    else
        L.flags &= ~kNeedsReset;
}

struct TabStepPtrs {
    const int64_t *actions;
    int64_t *obs;
    double *reward;
    uint8_t *terminated, *truncated;
    int64_t *final_obs;
    double *ep_ret;
    int32_t *ep_len;
    double *info, *final_info;
    uint64_t *act_lane;  // SAMPLE (mi_step with actions == NULL): as StepPtrs
    int64_t *actions_out;
    PcgJump act_jump;
};
template <int MODE, bool SAMPLE = false>
__global__ __launch_bounds__(kBlock) void tab_step_kernel(DevEnv d, TabStepPtrs io) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    if (i < d.N) {
        TabLane L;
        tab_load(d, i, L);
        int64_t obs, fin = 0;
        double reward, out_ret;
        int32_t out_len;
        bool te, tr, has_final;
        double fin_prob = 0.0;
        int64_t a;
        if constexpr (SAMPLE) {  // (random(N) * nvec).astype(int64): draw pos + i of the batched MultiDiscrete's generator (spaces/multi_discrete.py:176-178)
            const u128 astate = make_u128(io.act_lane[i], io.act_lane[(size_t)d.N + i]);
            a = (int64_t)((double)(pcg_output(astate) >> 11) * (1.0 / 9007199254740992.0) * (double)d.tab.nA);
            const u128 next = io.act_jump.mult * astate + io.act_jump.plus;
            io.act_lane[i] = (uint64_t)(next >> 64), io.act_lane[(size_t)d.N + i] = (uint64_t)next;
            if (io.actions_out) io.actions_out[i] = a;
        } else {
            a = io.actions[i];
        }
        tab_lane_step<MODE>(d, i, L, a, obs, fin, has_final, reward, te, tr, out_ret, out_len, st, nullptr, &fin_prob);
        tab_store(d, i, L);
        if (io.obs) tab_write_obs(d, (double)obs, io.obs, (size_t)i);
        if (io.reward) io.reward[i] = reward;
        if (io.terminated) io.terminated[i] = te;
        if (io.truncated) io.truncated[i] = tr;
        if (io.final_obs && has_final) tab_write_obs(d, (double)fin, io.final_obs, (size_t)i);
        if (io.ep_ret) io.ep_ret[i] = out_ret;
        if (io.ep_len) io.ep_len[i] = out_len;
        if (io.info && !is_blackjack(d)) io.info[i] = L.prob;
        if (io.final_info && has_final && !is_blackjack(d)) io.final_info[i] = fin_prob;
    }
    block_accumulate(d, st);
}
__global__ __launch_bounds__(kBlock) void tab_reset_kernel(DevEnv d, const uint8_t *mask, int64_t *obs) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.N || (mask && !mask[i])) return;
    TabLane L;
    tab_load(d, i, L);
    L.flags &= ~kNeedsReset;
    tab_autoreset(d, i, L);
    tab_store(d, i, L);
    if (obs) tab_write_obs(d, L.s, obs, (size_t)i);
}
// EX (mi_rollout_infos): the loop also stores the rows of `ex` -- info (the "prob" column; a reset's is 1), the finished episodes' return / length and,
// under SAME_STEP, the final state and the finishing transition's probability; zeros in the rows that finished nothing.  Without EX `ex` is not read.
template <int MODE, bool SAMPLE, bool LDS, int TK, bool EX = false>
__global__ __launch_bounds__(kBlock) void tab_rollout_kernel(DevEnv d, RolloutPtrs io, ActionStream as, int T, int lds_bytes, RolloutExtra ex) {
    // The transition table is read once per env-step through three levels of dependent loads (count / cumulative probabilities -> branch
    // -> successor, reward, flag); out of L2 that latency is the whole step (Taxi: 100 KB of tables).  When the launcher found that the
    // table fits (LDS) the workgroup first copies it into LDS -- layout: the f64 arrays, then the i32 arrays, then the flags --
    // and every lookup of the T steps is a 64-cycle LDS read instead.
    // LDS is a TEMPLATE parameter (round 6): chosen at run time, the table pointers were generic, the lookups FLAT loads -- 9 per env-step
    // (profiles/r06_frozenlake_rollout.txt: SQ_INSTS_VMEM_RD 1.19e6 per launch against 5e4 LDS instructions) -- and a flat load shares the
    // in-order vmcnt with the trajectory stores: every lookup waited for the stores before it to reach memory.
    extern __shared__ __align__(16) double tab_lds[];
    if constexpr (LDS) {
        const size_t cells = (size_t)d.tab.nS * d.tab.nA, rows = cells * d.tab.K;
        double *cs = tab_lds, *pr = cs + rows, *rw = pr + rows, *isd = rw + rows;
        int32_t *nx = reinterpret_cast<int32_t *>(isd + d.tab.nS), *cnt = nx + rows;
        uint8_t *tm = reinterpret_cast<uint8_t *>(cnt + cells);
        for (size_t k = threadIdx.x; k < rows; k += kBlock)
            cs[k] = d.tab.csprob[k], pr[k] = d.tab.prob[k], rw[k] = d.tab.reward[k], nx[k] = d.tab.next[k], tm[k] = d.tab.term[k];
        for (size_t k = threadIdx.x; k < cells; k += kBlock) cnt[k] = d.tab.count[k];
        for (int k = threadIdx.x; k < d.tab.nS; k += kBlock) isd[k] = d.tab.isd[k];
        __syncthreads();
        d.tab.csprob = cs, d.tab.prob = pr, d.tab.reward = rw, d.tab.isd = isd, d.tab.next = nx, d.tab.count = cnt, d.tab.term = tm;
    }
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    if (i < d.N) {
        TabLane L;
        tab_load<TK>(d, i, L);
        Pcg64 rng = load_rng(d, i);  // the lane's own stream stays in registers for the whole rollout
        u128 astate = 0;
        if (SAMPLE) {
            astate = make_u128(as.state_hi, as.state_lo);
            uint32_t delta = (uint32_t)i + 1u;
            for (int j = 0; delta; j++, delta >>= 1)
                if (delta & 1u) astate = as.pow2[j].mult * astate + as.pow2[j].plus;
        }
        const size_t N = (size_t)d.N;
        // (the policy's draw does not depend on the environment: step t + 1's action is drawn while step t's chain of table lookups is in flight)
        auto draw = [&]() {
            const uint64_t hi = (uint64_t)(astate >> 64), lo = (uint64_t)astate, x = hi ^ lo;
            const unsigned rot = (unsigned)(hi >> 58);
            const uint64_t out = (x >> rot) | (x << ((0u - rot) & 63u));
            astate = as.jump_n.mult * astate + as.jump_n.plus;
            return (int64_t)((double)(out >> 11) * (1.0 / 9007199254740992.0) * (double)d.tab.nA);  // (random(N) * nvec).astype(int64)
        };
        int64_t a_next = 0;
        if (SAMPLE && T > 0) a_next = draw();
        for (int t = 0; t < T; t++) {
            int64_t a;
            if (SAMPLE) {
                a = a_next;
                if (io.actions_out) static_cast<int64_t *>(io.actions_out)[t * N + i] = a;
                a_next = draw();  // (one draw past the last step: the stream's position is kept by the host, not by this state)
            } else {
                a = static_cast<const int64_t *>(io.actions_in)[t * N + i];
            }
            int64_t obs, fin = 0;
            double reward, out_ret;
            int32_t out_len;
            bool te, tr, has_final;
            double fin_prob = 0.0;
            tab_lane_step<MODE, TK>(d, i, L, a, obs, fin, has_final, reward, te, tr, out_ret, out_len, st, &rng, EX ? &fin_prob : nullptr);
            if (io.obs) tab_write_obs<TK>(d, (double)obs, static_cast<int64_t *>(io.obs), t * N + i);
            if (io.reward) io.reward[t * N + i] = reward;
            if (io.terminated) io.terminated[t * N + i] = te;
            if (io.truncated) io.truncated[t * N + i] = tr;
            if constexpr (EX) {
                if (ex.ep_ret) ex.ep_ret[t * N + i] = out_ret;
                if (ex.ep_len) ex.ep_len[t * N + i] = out_len;
                if (ex.info && TK != kTabBlackjack) ex.info[t * N + i] = L.prob;
                if (MODE == MI_AUTORESET_SAME_STEP && ex.final_obs) {
                    int64_t *fo = static_cast<int64_t *>(ex.final_obs);
                    if (has_final) {
                        tab_write_obs<TK>(d, (double)fin, fo, t * N + i);
                    } else if (TK == kTabBlackjack) {
                        fo[3 * (t * N + i)] = 0, fo[3 * (t * N + i) + 1] = 0, fo[3 * (t * N + i) + 2] = 0;
                    } else {
                        fo[t * N + i] = 0;
                    }
                }
                if (MODE == MI_AUTORESET_SAME_STEP && ex.final_info && TK != kTabBlackjack) ex.final_info[t * N + i] = has_final ? fin_prob : 0.0;
            }
        }
        tab_store<TK>(d, i, L);
        store_rng_state(d, i, rng);
    }
    block_accumulate(d, st);
}

// ---------------------------------------------------------------------------------------------------------
// The collector's rollout of a PLAIN transition table (FrozenLake, CliffWalking, Taxi without the fickle passenger): NEXT_STEP, on-device
// policy, one table for all sub-environments, at most three outcomes per (state, action).  Round 6, after the counters
// (profiles/r06_acrobot_toytext_root_cause.txt: 381 instructions per env-step from a lone wavefront, 39 branches in the loop body, three levels of
// dependent LDS reads): the same values as tab_rollout_kernel<NEXT_STEP, true, true, kTabPlain> from a loop body WITHOUT data-dependent control flow.
//   * A step and an autoreset step both take exactly ONE draw from the sub-environment's generator (utils.py:4-8 categorical_sample in
//     frozen_lake.py:330 and :345), so the draw is unconditional and the two cases are selects on its result, not two copies of the generator.
//   * The table is repacked into LDS as one record per (state, action) -- the cumulative probabilities with -1 behind the row's last outcome
//     ("first k with csprob[k] > u, 0 if none" then needs no count), the rewards, and successor | terminated << 31 -- so ONE level of reads
//     fetches every candidate and the outcome is selected in registers.
//   * The initial-state draw (first state whose cumulative probability exceeds u) starts from a 256-entry guide table -- guide[g] = first
//     state with isd_cs > g / 256, a lower bound of the answer for every u in [g / 256, (g + 1) / 256) because the sums are
//     non-decreasing -- and scans forward: one read for FrozenLake / CliffWalking, ~two for Taxi's 300 start states; under one
//     wavefront-uniform branch that only the steps with an autoreset in the wavefront take.
//   * info["prob"] of the last transition is looked up once, after the loop.
// KL: outcomes per record (1 or 3; a table with two outcomes uses 3).  FULL: all five trajectory arrays are present.
// ONE_START: every episode starts in `start_state` (FrozenLake, CliffWalking: the initial distribution is one state, mi_tabular_load found it) -- the
//   draw is taken and not looked at.  APOW2: the number of actions is a power of two -- (random() * nA).astype(int64) is the top bits of the output.
// ---------------------------------------------------------------------------------------------------------
template <int KL>
struct TabLeanCell;
template <>
struct TabLeanCell<1> {
    static constexpr int BYTES = 16;  // {reward, successor | terminated << 31, -}
};
template <>
struct TabLeanCell<3> {
    static constexpr int BYTES = 64;  // {cs0, cs1 | cs2, reward0 | reward1, reward2 | nt0, nt1, nt2, -}
};
constexpr int kTabGuide = 256;
static inline size_t tab_lean_lds_bytes(int nS, int nA, int KL) {
    return (size_t)nS * nA * (KL == 1 ? TabLeanCell<1>::BYTES : TabLeanCell<3>::BYTES) + (size_t)nS * sizeof(double) + kTabGuide * sizeof(uint32_t);
}
template <int KL, bool FULL, bool ONE_START, bool APOW2>
__global__ __launch_bounds__(kBlock) void tab_rollout_lean_kernel(DevEnv d, RolloutPtrs io, ActionStream as, int T, int start_state, int action_shift) {
    extern __shared__ __align__(16) double tab_lds[];
    constexpr int CELL = TabLeanCell<KL>::BYTES;
    const int nS = d.tab.nS, nA = d.tab.nA, K = d.tab.K;
    const int cells = nS * nA;
    char *const cell_base = reinterpret_cast<char *>(tab_lds);
    double *const isd = reinterpret_cast<double *>(cell_base + (size_t)cells * CELL);
    uint32_t *const guide = reinterpret_cast<uint32_t *>(isd + nS);
    for (int c = threadIdx.x; c < cells; c += kBlock) {
        const int n = d.tab.count[c];
        char *rec = cell_base + (size_t)c * CELL;
        if constexpr (KL == 1) {
            *reinterpret_cast<double *>(rec) = d.tab.reward[(size_t)c * K];
            *reinterpret_cast<uint32_t *>(rec + 8) = (uint32_t)d.tab.next[(size_t)c * K] | (d.tab.term[(size_t)c * K] ? 0x80000000u : 0u);
        } else {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const bool have = j < K && j < n;
                const size_t r = (size_t)c * K + (j < K ? j : 0);
                reinterpret_cast<double *>(rec)[j] = have ? d.tab.csprob[r] : -1.0;
                reinterpret_cast<double *>(rec)[3 + j] = d.tab.reward[r];
                reinterpret_cast<uint32_t *>(rec + 48)[j] = (uint32_t)d.tab.next[r] | (d.tab.term[r] ? 0x80000000u : 0u);
            }
        }
    }
    for (int k = threadIdx.x; !ONE_START && k < nS; k += kBlock) isd[k] = d.tab.isd[k];
    for (int g = threadIdx.x; !ONE_START && g < kTabGuide; g += kBlock) {  // first state with isd_cs > g / 256 (nS when there is none): bisection in the global array
        const double lim = (double)g * (1.0 / kTabGuide);
        int lo = 0, hi = nS;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (d.tab.isd[mid] > lim)
                hi = mid;
            else
                lo = mid + 1;
        }
        guide[g] = (uint32_t)lo;
    }
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    if (i < d.N) {
        const size_t N = (size_t)d.N;
        int s = (int)d.state[i];
        double prob = d.state[N + i];
        const uint32_t m = d.meta[i];
        uint32_t elapsed = m & kElapsedMask;
        const uint32_t flags0 = m >> kFlagShift;
        uint32_t need_reset = flags0 & kNeedsReset;
        double ep_ret = d.ep_ret[i];
        int32_t ep_len = d.ep_len[i];
        Pcg64 rng = load_rng(d, i);
        u128 astate = make_u128(as.state_hi, as.state_lo);
        {
            uint32_t delta = (uint32_t)i + 1u;
            for (int j = 0; delta; j++, delta >>= 1)
                if (delta & 1u) astate = as.pow2[j].mult * astate + as.pow2[j].plus;
        }
        const double dnA = (double)nA;
        auto draw = [&]() {  // (random(N) * nvec).astype(int64), spaces/multi_discrete.py:176-178
            const uint64_t hi = (uint64_t)(astate >> 64), lo = (uint64_t)astate, x = hi ^ lo;
            const unsigned rot = (unsigned)(hi >> 58);
            const uint64_t out = (x >> rot) | (x << ((0u - rot) & 63u));
            astate = pcg_muladd(astate, as.jump_n.mult, as.jump_n.plus);
            // (nA a power of two: random() * nA is exact, its integer part the output's top bits)
            if constexpr (APOW2) return (int32_t)(out >> action_shift);
            return (int32_t)((double)(out >> 11) * (1.0 / 9007199254740992.0) * dnA);
        };
        int32_t a_next = draw();
        int64_t *out_act = static_cast<int64_t *>(io.actions_out) + i, *out_obs = static_cast<int64_t *>(io.obs) + i;
        double *out_rew = io.reward + i;
        uint8_t *out_te = io.terminated + i, *out_tr = io.truncated + i;
        uint32_t last_rec = 0xffffffffu;  // record offset | outcome of the last step (0xffffffff: it was an autoreset step, or there was none)
#pragma unroll 2
        for (int t = 0; t < T; t++) {
            const int32_t a = a_next;
            a_next = draw();  // (one draw past the last step: the stream's position is kept by the host, not by this state)
            const bool resetting = need_reset != 0;
            // (ONE_START with one outcome per record: nothing reads u -- the generator still advances, its output function is dead code)
            const double u = rng.next_double();
            const uint32_t rec = (uint32_t)(s * nA + a) * (uint32_t)CELL;
            const char *p = cell_base + rec;
            double rew;
            uint32_t nt;
            uint32_t kk = 0;
            if constexpr (KL == 1) {
                const uint4 q = *reinterpret_cast<const uint4 *>(p);
                rew = __hiloint2double((int)q.y, (int)q.x);
                nt = q.z;
            } else {
                double2 q0 = *reinterpret_cast<const double2 *>(p), q1 = *reinterpret_cast<const double2 *>(p + 16),
                              q2 = *reinterpret_cast<const double2 *>(p + 32);
                uint4 q3 = *reinterpret_cast<const uint4 *>(p + 48);
                hold_opaque(q1.y), hold_opaque(q2.x), hold_opaque(q2.y), hold_opaque(q3.x), hold_opaque(q3.y), hold_opaque(q3.z);  // (all four reads are issued together: left alone the compiler sinks two of them behind a branch on c0)
                const bool c0 = q0.x > u, c1 = q0.y > u, c2 = q1.x > u;
                const bool take0 = c0 | !(c1 | c2);  // the first outcome, also when no cumulative sum exceeds u (np.argmax of all-False)
                rew = take0 ? q1.y : (c1 ? q2.x : q2.y);
                nt = take0 ? q3.x : (c1 ? q3.y : q3.z);
                kk = take0 ? 0u : (c1 ? 1u : 2u);
            }
            int rs = start_state;
            if (!ONE_START && resetting) {  // frozen_lake.py:345: categorical_sample(initial_state_distrib); only the steps with an autoreset in the wavefront come here
                int idx = (int)guide[(int)(u * (double)kTabGuide)];
                while (idx < nS && !(isd[idx] > u)) idx++;
                rs = idx < nS ? idx : 0;
            }
            const int s_new = resetting ? rs : (int)(nt & 0x7fffffffu);
            const bool te = !resetting && (nt >> 31) != 0;
            const double reward = resetting ? 0.0 : rew;
            const uint32_t el = elapsed + 1u;
            const bool tr = !resetting && d.max_steps > 0 && (int)el >= d.max_steps;
            const bool done = te || tr;
            const double ret = ep_ret + reward;
            const int32_t len = ep_len + 1;
            st.reset_steps += resetting ? 1u : 0u;
            st.episodes += done ? 1u : 0u;
            st.return_sum += done ? ret : 0.0;
            st.length_sum += done ? (uint64_t)len : 0ull;
            ep_ret = resetting ? 0.0 : ret;
            ep_len = resetting ? 0 : len;
            elapsed = resetting ? 0u : el;
            need_reset = done ? 1u : 0u;
            s = s_new;
            if (t == T - 1) last_rec = resetting ? 0xffffffffu : (rec / (uint32_t)CELL) * 4u + kk;
            if (FULL || io.actions_out) *out_act = (int64_t)a;
            if (FULL || io.obs) *out_obs = (int64_t)s_new;
            if (FULL || io.reward) *out_rew = reward;
            if (FULL || io.terminated) *out_te = te;
            if (FULL || io.truncated) *out_tr = tr;
            out_act += N, out_obs += N, out_rew += N, out_te += N, out_tr += N;
        }
        st.env_steps = (uint32_t)T - st.reset_steps;
        if (T > 0) prob = last_rec == 0xffffffffu ? 1.0 : d.tab.prob[(size_t)(last_rec >> 2) * K + (last_rec & 3u)];
        d.state[i] = (double)s, d.state[N + i] = prob;
        d.meta[i] = (elapsed & kElapsedMask) | (((flags0 & ~kNeedsReset) | need_reset) << kFlagShift);
        d.ep_ret[i] = ep_ret, d.ep_len[i] = ep_len;
        store_rng_state(d, i, rng);
    }
    block_accumulate(d, st);
}

// ---------------------------------------------------------------------------------------------------------
// Blackjack-v1's rollout (NEXT_STEP, on-device policy) without data-dependent control flow -- the values of tab_rollout_kernel<NEXT_STEP, true, false,
// kTabBlackjack>, which spends 784 instructions per env-step in three divergent branches (hit / stick with the dealer's loop / autoreset with its
// five or six draws), each with its own copies of the generator step and of Lemire's rejection loop.
//   * A step consumes a VARIABLE number of 32-bit values (np_random.choice = Lemire's bounded draw on PCG64's buffered halves): every lane produces the
//     next three 64-bit outputs unconditionally -- with the buffered half that is six or seven values, enough for an autoreset (5 - 6), a hit (1) and
//     a dealer who draws up to six cards -- evaluates all six as cards, and only COUNTS how many its case consumed: the generator's new state is
//     one of the four states it already has, the new buffered half one of the three high halves.
//   * hit, stick (the dealer's loop unrolled six times under a running `need` flag) and autoreset are evaluated side by side and selected.
//   * What does not fit -- a rejected draw (9 / 2^32 per card), a dealer who needs a seventh card -- is flagged per lane, and the flagged lanes redo
//     the step from the saved generator state through bj_step / bj_reset, behind one wavefront-uniform branch (`force_slow`: tests send every k-th
//     lane-step there).
// ---------------------------------------------------------------------------------------------------------
MI_DEV int bj_hand(int raw, int ace) { return (ace != 0 && raw + 10 <= 21) ? raw + 10 : raw; }
template <bool FULL>
__global__ __launch_bounds__(kBlock) void bj_rollout_lean_kernel(DevEnv d, RolloutPtrs io, ActionStream as, int T, int force_slow) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    if (i < d.N) {
        const size_t N = (size_t)d.N;
        const int64_t packed0 = (int64_t)d.state[i];
        int psum = (int)(packed0 & 63), pace = (int)((packed0 >> 6) & 1), ptwo = (int)((packed0 >> 7) & 1);
        int d0 = (int)((packed0 >> 8) & 15), d1 = (int)((packed0 >> 12) & 15);
        const uint64_t aux0 = (uint64_t)d.state[N + i];
        int hh = (aux0 >> 32) ? 1 : 0;  // a buffered 32-bit half is waiting
        uint32_t half = (uint32_t)aux0;
        const uint32_t m0 = d.meta[i];
        uint32_t elapsed = m0 & kElapsedMask;
        const uint32_t flags0 = m0 >> kFlagShift;
        uint32_t need_reset = flags0 & kNeedsReset;
        double ep_ret = d.ep_ret[i];
        int32_t ep_len = d.ep_len[i];
        Pcg64 rng = load_rng(d, i);
        const bool natural = d.P.p[0] != 0.0, sab = d.P.p[1] != 0.0;
        u128 astate = make_u128(as.state_hi, as.state_lo);
        {
            uint32_t delta = (uint32_t)i + 1u;
            for (int j = 0; delta; j++, delta >>= 1)
                if (delta & 1u) astate = as.pow2[j].mult * astate + as.pow2[j].plus;
        }
        auto draw = [&]() {  // Discrete(2): (random() * 2).astype(int64) is the output's top bit
            const int32_t a = (int32_t)(pcg_output(astate) >> 63);
            astate = pcg_muladd(astate, as.jump_n.mult, as.jump_n.plus);
            return a;
        };
        int32_t a_next = draw();
        int64_t *out_act = static_cast<int64_t *>(io.actions_out) + i, *out_obs = static_cast<int64_t *>(io.obs) + (size_t)3 * i;
        double *out_rew = io.reward + i;
        uint8_t *out_te = io.terminated + i, *out_tr = io.truncated + i;
        for (int t = 0; t < T; t++) {
            const int32_t a = a_next;
            a_next = draw();
            const bool resetting = need_reset != 0;
            // the next three outputs and the six values a step can consume
            const u128 s0 = rng.state;
            const u128 s1 = pcg_muladd(s0, pcg_mult(), rng.inc), s2 = pcg_muladd(s1, pcg_mult(), rng.inc), s3 = pcg_muladd(s2, pcg_mult(), rng.inc);
            const uint64_t o1 = pcg_output(s1), o2 = pcg_output(s2), o3 = pcg_output(s3);
            const uint32_t l1 = (uint32_t)o1, h1 = (uint32_t)(o1 >> 32), l2 = (uint32_t)o2, h2 = (uint32_t)(o2 >> 32), l3 = (uint32_t)o3, h3 = (uint32_t)(o3 >> 32);
            uint32_t x[6];
            x[0] = hh ? half : l1, x[1] = hh ? l1 : h1, x[2] = hh ? h1 : l2, x[3] = hh ? l2 : h2, x[4] = hh ? h2 : l3, x[5] = hh ? l3 : h3;
            int c[6];
            bool rej[6];
#pragma unroll
            for (int j = 0; j < 6; j++) {  // bj_card: deck[Lemire(13)], rejected when the product's low word is below 2^32 mod 13 = 9
                const uint32_t k = __umulhi(x[j], 13u);
                c[j] = k < 9u ? (int)k + 1 : 10;
                rej[j] = x[j] * 13u < 9u;
            }
            // autoreset (blackjack.py:181-202): dealer's hand, player's hand, the suit draw (n = 4: never rejected), the face draw when the dealer shows a ten (n = 3: rejects 0)
            const int r_cnt = 5 + (c[0] == 10 ? 1 : 0);
            const bool r_over = rej[0] | rej[1] | rej[2] | rej[3] | (c[0] == 10 && x[5] == 0u);
            const int r_psum = c[2] + c[3], r_pace = (c[2] == 1 || c[3] == 1) ? 1 : 0;
            // hit (:144-151)
            const int h_psum = psum + c[0], h_pace = pace | (c[0] == 1 ? 1 : 0);
            const bool h_te = bj_hand(h_psum, h_pace) > 21;
            // stick (:152-169): the dealer draws to 17
            int dsum = d0 + d1, dace = (d0 == 1 || d1 == 1) ? 1 : 0, dtwo = 1, s_cnt = 0;
            bool s_over = false, alive = true;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const bool need = alive && bj_hand(dsum, dace) < 17;
                s_cnt += need ? 1 : 0;
                dsum += need ? c[j] : 0;
                dace |= (need && c[j] == 1) ? 1 : 0;
                dtwo = need ? 0 : dtwo;
                s_over |= need && rej[j];
                alive = need;
            }
            s_over |= alive && bj_hand(dsum, dace) < 17;  // a seventh card
            const int ph = bj_hand(psum, pace), dh = bj_hand(dsum, dace);
            const int ps = ph > 21 ? 0 : ph, ds = dh > 21 ? 0 : dh;
            double s_rew = (double)(ps > ds) - (double)(ps < ds);
            const bool pnat = ptwo && pace && psum == 11, dnat = dtwo && dace && dsum == 11;  // sorted(hand) == [1, 10]
            s_rew = (sab && pnat && !dnat) ? 1.0 : ((!sab && natural && pnat && s_rew == 1.0) ? 1.5 : s_rew);
            // the lane's case
            const bool hit = a != 0;
            int cnt = resetting ? r_cnt : (hit ? 1 : s_cnt);
            bool over = resetting ? r_over : (hit ? rej[0] : s_over);
            if (force_slow) over |= (uint32_t)(i + t) % (uint32_t)force_slow == 0u;
            const int o_psum = psum, o_pace = pace, o_ptwo = ptwo, o_d0 = d0, o_d1 = d1;
            double rew = resetting ? 0.0 : (hit ? (h_te ? -1.0 : 0.0) : s_rew);
            bool te0 = !resetting && (hit ? h_te : true);
            psum = resetting ? r_psum : (hit ? h_psum : psum);
            pace = resetting ? r_pace : (hit ? h_pace : pace);
            ptwo = resetting ? 1 : (hit ? 0 : ptwo);
            d0 = resetting ? c[0] : d0, d1 = resetting ? c[1] : d1;
            // what the case consumed: `cnt` values = the buffered half first, then halves of new outputs
            const int m = cnt - hh, calls = (m + 1) >> 1;
            const int o_hh = hh;
            const uint32_t o_half = half;
            half = calls == 0 ? half : (calls == 1 ? h1 : (calls == 2 ? h2 : h3));
            hh = m & 1;
            rng.state = calls == 0 ? s0 : (calls == 1 ? s1 : (calls == 2 ? s2 : s3));
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(over) != 0ull, 0)) {
                if (over) {  // the general routines from the state before the step
                    Pcg64 r = {s0, rng.inc};
                    double aux = o_hh ? (double)((1ull << 32) | (uint64_t)o_half) : 0.0;
                    double sd = (double)(o_psum | (o_pace << 6) | (o_ptwo << 7) | (o_d0 << 8) | (o_d1 << 12));
                    if (resetting) {
                        bj_reset(r, sd, aux);
                        rew = 0.0, te0 = false;
                    } else {
                        bj_step(r, sd, aux, (int64_t)a, natural, sab, rew, te0);
                    }
                    const int64_t q = (int64_t)sd;
                    psum = (int)(q & 63), pace = (int)((q >> 6) & 1), ptwo = (int)((q >> 7) & 1), d0 = (int)((q >> 8) & 15), d1 = (int)((q >> 12) & 15);
                    const uint64_t ax = (uint64_t)aux;
                    hh = (ax >> 32) ? 1 : 0, half = (uint32_t)ax;
                    rng.state = r.state;
                }
            }
            const bool te = te0;
            const uint32_t el = elapsed + 1u;
            const bool tr = !resetting && d.max_steps > 0 && (int)el >= d.max_steps;
            const bool done = te || tr;
            const double ret = ep_ret + rew;
            const int32_t len = ep_len + 1;
            st.reset_steps += resetting ? 1u : 0u;
            st.episodes += done ? 1u : 0u;
            st.return_sum += done ? ret : 0.0;
            st.length_sum += done ? (uint64_t)len : 0ull;
            ep_ret = resetting ? 0.0 : ret;
            ep_len = resetting ? 0 : len;
            elapsed = resetting ? 0u : el;
            need_reset = done ? 1u : 0u;
            if (FULL || io.actions_out) *out_act = (int64_t)a;
            if (FULL || io.obs) {  // _get_obs: (player sum with a usable ace as 11, dealer's first card, usable ace)
                const int usable = (pace != 0 && psum + 10 <= 21) ? 1 : 0;
                out_obs[0] = (int64_t)(usable ? psum + 10 : psum), out_obs[1] = (int64_t)d0, out_obs[2] = (int64_t)usable;
            }
            if (FULL || io.reward) *out_rew = rew;
            if (FULL || io.terminated) *out_te = te;
            if (FULL || io.truncated) *out_tr = tr;
            out_act += N, out_obs += 3 * N, out_rew += N, out_te += N, out_tr += N;
        }
        st.env_steps = (uint32_t)T - st.reset_steps;
        d.state[i] = (double)(psum | (pace << 6) | (ptwo << 7) | (d0 << 8) | (d1 << 12));
        d.state[N + i] = hh ? (double)((1ull << 32) | (uint64_t)half) : 0.0;
        d.meta[i] = (elapsed & kElapsedMask) | (((flags0 & ~kNeedsReset) | need_reset) << kFlagShift);
        d.ep_ret[i] = ep_ret, d.ep_len[i] = ep_len;
        store_rng_state(d, i, rng);
    }
    block_accumulate(d, st);
}

}  // namespace
#endif  // MI355ENV_TABULAR_KERNELS_H
