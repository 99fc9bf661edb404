// lane_step.h -- one classic-control sub-environment in one lane: the lane's registers (Lane) and how they are requested from and stored to the
// struct-of-arrays state (LaneRequest, AttrRequest, load_lane / store_lane), the reset draws taken ahead (ResetQueue), one lockstep step of the
// lane with TimeLimit, the autoreset state machine and the episode statistics (lane_step; lane_step_fused, its branch-free NEXT_STEP form for the
// fused rollouts; lane_step_wrapped, with RepeatAction / StickyAction around the env's step), and the row stores.  Templates over the env types of
// envs_classic.h; the kernels that run them are in classic_kernels.h.  No kernel and no host code here.
#ifndef MI355ENV_LANE_STEP_H
#define MI355ENV_LANE_STEP_H
#include <type_traits>

#include "engine_types.h"
#include "lane_common.h"

namespace {

template <class E>
struct Lane {
    double s[E::S];
    uint32_t elapsed, flags;
    double ep_ret;
    int32_t ep_len;
    typename E::Trig trig;  // sin / cos of the state's angles from the last obs() (envs_classic.h), registers only
};

template <class E>
MI_DEV void load_lane(const DevEnv &d, int i, Lane<E> &L) {
#pragma unroll
    for (int k = 0; k < E::S; k++) L.s[k] = d.state[(size_t)k * d.N + i];
    const uint32_t m = d.meta[i];
    L.elapsed = m & kElapsedMask, L.flags = m >> kFlagShift;
    L.ep_ret = d.ep_ret[i], L.ep_len = d.ep_len[i];
    trig_invalidate(L.trig);
}
// E has per-lane attributes (envs_classic.h *AttrT: N_ATTR, attr_default, attrs_arrive)
template <class E, class = void>
struct HasAttrs : std::false_type {};
template <class E>
struct HasAttrs<E, std::void_t<decltype(E::N_ATTR)>> : std::true_type {};
// E::step() itself draws from the sub-environment's generator (envs_classic.h AcrobotAttrT: torque noise): E::step_draws(trig) says whether the lane
// takes its one next_double this step, E::step_drawn(trig, u) receives it.  Such a type's reset draws are never taken ahead (ResetQueue stays
// empty between steps), so the generator is always at the reference's position and the draws come in the reference's order.
template <class E, class = void>
struct HasStepDraws : std::false_type {};
template <class E>
struct HasStepDraws<E, std::void_t<decltype(E::STEP_DRAWS)>> : std::integral_constant<bool, E::STEP_DRAWS> {};
// The lane's attributes, requested with the rest of its loads and handed to its register struct (Lane::trig) on arrival; empty for the other types.
template <class E, bool = HasAttrs<E>::value>
struct AttrRequest {
    MI_DEV void request(const AttrDev &, const DevEnv &, int) {}
    template <class T>
    MI_DEV void arrive(T &) {}
};
template <class E>
struct AttrRequest<E, true> {
    double v[E::N_ATTR];
    MI_DEV void request(const AttrDev &at, const DevEnv &d, int i) {
#pragma unroll
        for (int a = 0; a < E::N_ATTR; a++) v[a] = (at.mask >> a) & 1u ? at.rows[(size_t)a * d.N + i] : E::attr_default(a, d.P);
    }
    MI_DEV void arrive(typename E::Trig &t) {
#pragma unroll
        for (int a = 0; a < E::N_ATTR; a++) hold_opaque(v[a]);
        E::attrs_arrive(v, t);
    }
};

template <class E>
struct LaneRequest {
    double s[E::S], ep_ret;
    uint32_t meta;
    int32_t ep_len;
    uint64_t g[4];
    uint64_t ag[2];  // SAMPLE: the lane's state of the action stream (mi_step with actions == NULL)
    typename E::Act a;
    template <bool SAMPLE>
    MI_DEV void request(const DevEnv &d, const void *actions, const uint64_t *act_lane, int i, bool with_generator) {
#pragma unroll
        for (int k = 0; k < E::S; k++) s[k] = d.state[(size_t)k * d.N + i];
        meta = d.meta[i], ep_ret = d.ep_ret[i], ep_len = d.ep_len[i];
        if constexpr (SAMPLE)
            ag[0] = act_lane[i], ag[1] = act_lane[(size_t)d.N + i], a = (typename E::Act)0;
        else
            ag[0] = ag[1] = 0, a = static_cast<const typename E::Act *>(actions)[i];
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = with_generator ? d.rng[(size_t)k * d.N + i] : 0;
    }
    MI_DEV void arrive(Lane<E> &L, Pcg64 &gen) {
#pragma unroll
        for (int k = 0; k < E::S; k++) hold_opaque(s[k]), L.s[k] = s[k];
        hold_opaque(meta), hold_opaque(ep_ret), hold_opaque(ep_len), hold_opaque(a), hold_opaque(ag[0]), hold_opaque(ag[1]);
#pragma unroll
        for (int k = 0; k < 4; k++) hold_opaque(g[k]);
        L.elapsed = meta & kElapsedMask, L.flags = meta >> kFlagShift;
        L.ep_ret = ep_ret, L.ep_len = ep_len;
        trig_invalidate(L.trig);
        gen.state = make_u128(g[0], g[1]), gen.inc = make_u128(g[2], g[3]);
    }
};
template <class E>
MI_DEV void store_lane(const DevEnv &d, int i, const Lane<E> &L) {
#pragma unroll
    for (int k = 0; k < E::S; k++) d.state[(size_t)k * d.N + i] = L.s[k];
    d.meta[i] = (L.elapsed & kElapsedMask) | (L.flags << kFlagShift);
    d.ep_ret[i] = L.ep_ret, d.ep_len[i] = L.ep_len;
}

// The next E::NDRAWS values of the lane's own stream, drawn AHEAD of the reset that will consume them.
// In a wavefront of 64 CartPoles some lane finishes an episode in ~95 % of the steps, so a reset path executed
// on demand costs every wavefront four 128-bit LCG steps (40 integer multiplies) on almost every
// step for the benefit of ~3 lanes.  A fused rollout instead refills all empty queues of a wavefront together
// every kRefillPeriod steps and a reset merely moves the queued values into the state.  The stream order is
// unchanged (the env's generator is consumed by resets only), and unconsumed draws are handed back at the end of
// the launch (Pcg64::unstep), so the generator state in HBM is always exactly the reference's.
// The generator itself is held in registers for the whole launch: a loop without global loads also keeps the
// compiler from draining the store queue (s_waitcnt vmcnt(0)) on every iteration -- loads and stores share one
// in-order counter on gfx950.
template <class E>
struct ResetQueue {
    double u[E::NDRAWS];
    double rs[E::S];  // the reset state those draws give under the default bounds (autoreset has no options): computed once per refill
    // (an integer, not a bool: a bool that lives across the role branches of rollout_duo_kernel is a lane mask in scalar registers, which the
    //  compiler merges with three scalar instructions at every join of every phase -- ~9 instructions per phase and flag, on every wavefront)
    uint32_t have;
    Pcg64 rng;
    MI_DEV void refill() {
#pragma unroll
        for (int k = 0; k < E::NDRAWS; k++) u[k] = rng.next_double();
        double b0, b1;
        uint32_t f = 0;
        E::default_bounds(b0, b1);
        E::reset_u(u, rs, f, b0, b1);
        have = 1u;
    }
    // what reset_u does to the flag word does not depend on the draws: it sets or clears kStateF32 (envs_classic.h)
    static MI_DEV uint32_t reset_flags(uint32_t flags) {
        const double zero[E::NDRAWS] = {};
        double tmp[E::S], b0, b1;
        E::default_bounds(b0, b1);
        E::reset_u(zero, tmp, flags, b0, b1);
        return flags;
    }
};
constexpr int kRefillPeriod = 8;

template <class E>
MI_DEV void draw_reset_values(const DevEnv &d, int i, double u[E::NDRAWS], const Pcg64 *preloaded = nullptr) {
    Pcg64 rng = preloaded ? *preloaded : load_rng(d, i);
#pragma unroll
    for (int k = 0; k < E::NDRAWS; k++) u[k] = rng.next_double();
    store_rng_state(d, i, rng);
}

// Reset of one lane from its own stream, with the reference's default bounds (autoreset: reset() has no options).
template <class E>
MI_DEV void lane_autoreset(const DevEnv &d, int i, Lane<E> &L, ResetQueue<E> *q, const Pcg64 *preloaded = nullptr) {
    double u[E::NDRAWS];
    if (q) {
        if (!q->have) q->refill();  // rare: two episode ends within one refill period
#pragma unroll
        for (int k = 0; k < E::NDRAWS; k++) u[k] = q->u[k];
        q->have = 0u;
    } else {
        draw_reset_values<E>(d, i, u, preloaded);
    }
    double b0, b1;
    E::default_bounds(b0, b1);
    E::reset_u(u, L.s, L.flags, b0, b1);
    L.elapsed = 0;  // TimeLimit.reset (wrappers/common.py:149)
    L.ep_ret = 0.0, L.ep_len = 0;
}

template <class E>
struct StepOut {
    float obs[E::OBS];
    float final_obs[E::OBS];
    double reward, ep_ret;
    int32_t ep_len;
    bool terminated, truncated, has_final;
};

// One lockstep step of one sub-environment: sync_vector_env.py:277-329 + TimeLimit + RecordEpisodeStatistics.
template <class E, int MODE>
MI_DEV void lane_step(const DevEnv &d, int i, Lane<E> &L, typename E::Act a, StepOut<E> &o, LaneStats &st,
                      ResetQueue<E> *q = nullptr, const Pcg64 *preloaded = nullptr) {
    bool te = false, tr = false;
    double rew = 0.0;
    o.has_final = false;
    [[maybe_unused]] Pcg64 stepped;  // HasStepDraws without a queue: the lane's generator, which the step's own draw moves before a reset reads it
    if constexpr (HasStepDraws<E>::value) {
        if (!q) stepped = preloaded ? *preloaded : load_rng(d, i), preloaded = &stepped;
    }
    if (MODE == MI_AUTORESET_NEXT_STEP && (L.flags & kNeedsReset)) {
        // :279-284 the step after a finished episode resets, ignores the action, returns reward 0 / not done
        lane_autoreset<E>(d, i, L, q, preloaded);
        st.reset_steps++;
    } else if (MODE == MI_AUTORESET_DISABLED && (L.flags & kNeedsReset)) {
        // :295 `assert not self._autoreset_envs[i]`: report through the sticky error word, leave the lane untouched
        *d.error = kErrDisabledStepped;
        E::obs(L.s, L.flags, o.obs, L.trig);
        o.reward = 0.0, o.terminated = false, o.truncated = false, o.ep_ret = 0.0, o.ep_len = 0;
        return;
    } else {
        if (!E::valid(a)) {
            // cartpole.py:165-167 asserts before it touches the state: report through the sticky error word, leave the lane untouched (host
            // callers never get here -- their actions are validated before the launch)
            *d.error = kErrInvalidAction;
            E::obs(L.s, L.flags, o.obs, L.trig);
            o.reward = 0.0, o.terminated = false, o.truncated = false, o.ep_ret = 0.0, o.ep_len = 0;
            return;
        }
        if constexpr (HasStepDraws<E>::value) {
            if (E::step_draws(L.trig)) {
                if (q) {
                    E::step_drawn(L.trig, q->rng.next_double());
                } else {  // the generator moves in memory now; a SAME_STEP reset below continues from there
                    E::step_drawn(L.trig, stepped.next_double());
                    store_rng_state(d, i, stepped);
                }
            }
        }
        E::step(L.s, L.flags, a, d.P, rew, te, L.trig);
        L.elapsed += 1;  // TimeLimit.step (wrappers/common.py:129-133)
        tr = d.max_steps > 0 && (int)L.elapsed >= d.max_steps;
        L.ep_ret += rew, L.ep_len += 1;
        st.env_steps++;
    }
    const bool done = te || tr;
    o.ep_ret = done ? L.ep_ret : 0.0;
    o.ep_len = done ? L.ep_len : 0;
    if (done) {
        st.episodes++;
        st.return_sum += L.ep_ret;
        st.length_sum += (uint64_t)L.ep_len;
    }
    if (MODE == MI_AUTORESET_SAME_STEP && done) {
        // :302-319 final_obs, then reset within the same step
        E::obs(L.s, L.flags, o.final_obs, L.trig);
        o.has_final = true;
        lane_autoreset<E>(d, i, L, q, preloaded);
    }
    E::obs(L.s, L.flags, o.obs, L.trig);
    o.reward = rew, o.terminated = te, o.truncated = tr;
    if (done && MODE != MI_AUTORESET_SAME_STEP)
        L.flags |= kNeedsReset;  // _autoreset_envs (:329)
    else
        L.flags &= ~kNeedsReset;
}

// NEXT_STEP step of one lane inside a fused rollout, written without divergent control flow: a wavefront that runs
// alone on its SIMD pays an issue slot for every s_and_saveexec / s_cbranch and a refetch for every taken branch,
// and with 64 CartPoles per wavefront some lane is in its autoreset step on ~95 % of the steps anyway.  So every
// lane integrates (a finished episode's state is finite; the result is discarded) and the autoreset lanes SELECT the
// queued reset values instead.  Same results as lane_step<E, NEXT_STEP>.
template <class E, bool CHECK_ACTION>
MI_DEV void lane_step_fused(const DevEnv &d, Lane<E> &L, typename E::Act a, StepOut<E> &o, LaneStats &st, ResetQueue<E> &q) {
    const bool resetting = (L.flags & kNeedsReset) != 0;
    if (__builtin_expect(resetting && !q.have, 0)) q.refill();  // rare: two episode ends within one refill period
    // cartpole.py:165-167 asserts before it touches the state: an action outside the space is reported through the sticky error word and
    // the lane is left untouched (lane_step's rule) -- it integrates a stand-in action like a resetting lane does and SELECTS its old state.
    bool invalid = false;
    double s0[E::S];
    if (CHECK_ACTION) {
#pragma unroll
        for (int k = 0; k < E::S; k++) s0[k] = L.s[k];
        invalid = !resetting && !E::valid(a);
        if (invalid) {
            *d.error = kErrInvalidAction;
            a = (typename E::Act)0;
        }
    }
    if constexpr (HasStepDraws<E>::value) {  // a lane that steps (not one that resets, or whose action is refused) takes its draw before the dynamics
        if (!resetting && !invalid && E::step_draws(L.trig)) E::step_drawn(L.trig, q.rng.next_double());
    }
    // the reset candidate (sync_vector_env.py:279-284): the state was formed from the queued draws when they were drawn
    const double (&rs)[E::S] = q.rs;
    const uint32_t rflags = ResetQueue<E>::reset_flags(L.flags & ~kNeedsReset);
    // the step candidate
    double rew;
    bool te;
    uint32_t sflags = L.flags;
    if constexpr (E::SPLIT_TERMINAL) {
        // Acrobot: the terminal test needs cos(theta1) of the NEW state, which the observation evaluates anyway.  Integrate, select the reset
        // lanes' state, take the observation, then test the terminal condition on it with the observation's trig values: for a stepping lane
        // the selected state IS its new state (same argument, same function, same bits); a resetting lane's flag is discarded below.
        E::integrate(L.s, sflags, a, L.trig);
        if (CHECK_ACTION && invalid) {
#pragma unroll
            for (int k = 0; k < E::S; k++) L.s[k] = s0[k];
            sflags = L.flags;
        }
#pragma unroll
        for (int k = 0; k < E::S; k++) L.s[k] = resetting ? rs[k] : L.s[k];
        E::obs(L.s, sflags, o.obs, L.trig);
        E::terminal_after_obs(L.s, L.trig, rew, te);
        if (CHECK_ACTION && invalid) rew = 0.0, te = false;
    } else {
        E::step(L.s, sflags, a, d.P, rew, te, L.trig);
        if (CHECK_ACTION && invalid) {  // rare, divergent: undo
#pragma unroll
            for (int k = 0; k < E::S; k++) L.s[k] = s0[k];
            sflags = L.flags, rew = 0.0, te = false;
            trig_invalidate(L.trig);
        }
    }
    const uint32_t moved = (CHECK_ACTION && invalid) ? 0u : 1u;
    const uint32_t elapsed = L.elapsed + moved;  // TimeLimit.step (wrappers/common.py:129-133)
    const bool tr = moved && d.max_steps > 0 && (int)elapsed >= d.max_steps;
    const double ep_ret = L.ep_ret + rew;
    const int32_t ep_len = L.ep_len + (int32_t)moved;
    const bool done = !resetting && (te || tr);
    if constexpr (!E::SPLIT_TERMINAL) {
#pragma unroll
        for (int k = 0; k < E::S; k++) L.s[k] = resetting ? rs[k] : L.s[k];
    }
    L.flags = resetting ? rflags : (done ? (sflags | kNeedsReset) : sflags);
    L.elapsed = resetting ? 0u : elapsed;
    L.ep_ret = resetting ? 0.0 : ep_ret;
    L.ep_len = resetting ? 0 : ep_len;
    q.have = resetting ? 0u : q.have;
    st.reset_steps += resetting ? 1u : 0u;
    st.env_steps += resetting ? 0u : moved;
    st.episodes += done ? 1u : 0u;
    st.return_sum += done ? ep_ret : 0.0;
    st.length_sum += done ? (uint64_t)ep_len : 0ull;
    if constexpr (!E::SPLIT_TERMINAL) E::obs(L.s, L.flags, o.obs, L.trig);
    o.reward = resetting ? 0.0 : rew;
    o.terminated = !resetting && te, o.truncated = !resetting && tr;
    o.ep_ret = done ? ep_ret : 0.0, o.ep_len = done ? ep_len : 0;
    o.has_final = false;
}

// ---- RepeatAction / StickyAction of the scalar envs (wrappers/stateful_action.py:16-220) inside the lane's step -----------------------------------
// The reference wraps every sub-environment: SyncVectorEnv(StickyAction(RepeatAction(TimeLimit(env), k), p, d)).  Both sit BELOW the vector level, so a
// finished lane stops repeating while its neighbours go on, and the sticky draw comes from the lane's own generator -- the one its resets consume --
// before the step.  The kernels that run it are their own (step_wrapped_kernel, rollout_wrapped_kernel): the others are the code they were.
// StickyAction's state of one lane, in registers for the launch
template <class E>
struct WrapLane {
    typename E::Act last;
    uint32_t word;
};
template <class A>
MI_DEV uint64_t action_bits(A a) {
    uint64_t b = 0;
    __builtin_memcpy(&b, &a, sizeof a);
    return b;
}
template <class E>
MI_DEV void load_wrap_lane(const WrapDev &w, int i, WrapLane<E> &s) {
    uint64_t b = 0;
    s.word = 0u;
    if (w.sticky_duration) b = w.last_action[i], s.word = w.sticky_word[i];
    __builtin_memcpy(&s.last, &b, sizeof s.last);
}
template <class E>
MI_DEV void store_wrap_lane(const WrapDev &w, int i, const WrapLane<E> &s) {
    if (w.sticky_duration) w.last_action[i] = action_bits(s.last), w.sticky_word[i] = s.word;
}
constexpr uint32_t kStickyHasLast = 1u << 31;
// ... and, for the MAXSKIP instantiations (mi_set_max_and_skip), MaxAndSkipObservation's _obs_buffer of the lane (WrapSkipDev::frames), in registers
// for the launch like the words above.  `written`: a slot was written since the load.  (load_skip_lane / store_skip_lane: behind the row stores below.)
template <class E>
struct SkipWrapLane : WrapLane<E> {
    float f[2][E::OBS];
    uint32_t written;
    // np.max(self._obs_buffer, axis=0): a plain comparison, which also hands a NaN on from either slot as np.max does (unreachable from the five
    // kinds).  Which zero comes out of +0 and -0 is not pinned by NumPy's reduction and not pinned here.
    MI_DEV void max_frame(float dst[E::OBS]) const {
#pragma unroll
        for (int k = 0; k < E::OBS; k++) dst[k] = (f[0][k] > f[1][k] || f[0][k] != f[0][k]) ? f[0][k] : f[1][k];
    }
};
template <class E, bool MAXSKIP>
using WrapLaneOf = std::conditional_t<MAXSKIP, SkipWrapLane<E>, WrapLane<E>>;

// lane_step with the two wrappers around E::step.  The plain form of lane_step (branches, not lane_step_fused's selects): the repeat loop has a
// wave-uniform trip count (w.repeats), and a lane whose episode ended inside it is masked off for the remaining trips (`active`), so the wavefront
// stays in step.  Order of the generator's draws, as in the reference: the sticky draw (StickyAction.action, :118-142), then each inner step's own
// draw (STEP_DRAWS), then a SAME_STEP reset's.  Nothing is drawn ahead: with a queue (rollouts) the generator is q->rng and the queue is filled
// only by the reset that empties it; without (step_kernel) it is a copy of `preloaded` that goes back to memory when it moved.
// MAXSKIP: MaxAndSkipObservation(env, skip) (wrappers/stateful_observation.py:623-649) in RepeatAction's place.  The loop is RepeatAction's -- the host
// hands the skip over as w.repeats --; the observation after inner step skip - 2 goes to frame slot 0, the one after skip - 1 to slot 1 (E::obs is
// evaluated at those two only), and what the step returns where RepeatAction returns the last inner observation is the element-wise maximum of the two
// slots AS THEY THEN STAND: nothing ever clears them (they are read and written here and nowhere else), so a step that ended before it wrote a slot
// returns what an earlier step -- of an earlier episode, or the constructor's zeros -- left there.  The other instantiations are, statement for
// statement, the function they were: everything added stands under `if constexpr (MAXSKIP)`.
template <class E, int MODE, bool MAXSKIP = false>
MI_DEV void lane_step_wrapped(const DevEnv &d, const WrapArg<MAXSKIP> &w, WrapLaneOf<E, MAXSKIP> &sl, int i, Lane<E> &L, typename E::Act a, StepOut<E> &o, LaneStats &st,
                              ResetQueue<E> *q, const Pcg64 *preloaded) {
    o.has_final = false;
    Pcg64 own;
    if (!q) own = preloaded ? *preloaded : load_rng(d, i);
    if (MODE == MI_AUTORESET_NEXT_STEP && (L.flags & kNeedsReset)) {
        // sync_vector_env.py:279-284: the step after a finished episode resets (StickyAction.reset clears its state, :107-116), ignores the action
        // -- action() is not called: no draw --, repeats nothing and returns reward 0
        lane_autoreset<E>(d, i, L, q, &own);
        st.reset_steps++;
        sl.word = 0u;
        E::obs(L.s, L.flags, o.obs, L.trig);
        o.reward = 0.0, o.terminated = false, o.truncated = false, o.ep_ret = 0.0, o.ep_len = 0;
        L.flags &= ~kNeedsReset;
        return;
    }
    if ((MODE == MI_AUTORESET_DISABLED && (L.flags & kNeedsReset)) || !E::valid(a)) {
        // lane_step's two refusals: the lane, its generator and its sticky state are left untouched.  The action is validated AS GIVEN -- stricter than
        // the reference, which never looks at an action that a sticky one replaces.
        *d.error = (MODE == MI_AUTORESET_DISABLED && (L.flags & kNeedsReset)) ? kErrDisabledStepped : kErrInvalidAction;
        E::obs(L.s, L.flags, o.obs, L.trig);
        o.reward = 0.0, o.terminated = false, o.truncated = false, o.ep_ret = 0.0, o.ep_len = 0;
        return;
    }
    Pcg64 &g = q ? q->rng : own;
    bool drew = false;
    if (w.sticky_duration) {  // StickyAction.action (:118-142) with an int duration: num_repeats = duration whenever a series runs
        uint32_t taken = sl.word & ~kStickyHasLast;
        bool stick = taken != 0u;  // already stuck: no draw
        if (!stick && (sl.word & kStickyHasLast)) stick = g.next_double() < w.sticky_p, drew = true;  // np_random.uniform() < p, float64
        a = stick ? sl.last : a;
        taken = stick ? taken + 1u : 0u;
        taken = taken == (uint32_t)w.sticky_duration ? 0u : taken;  // the series is over: is_sticky_actions, num_repeats, repeats_taken cleared
        sl.last = a, sl.word = kStickyHasLast | taken;
    }
    // RepeatAction.step (:197-220) over TimeLimit.step (wrappers/common.py:129-133): elapsed counts INNER steps
    const int trips = w.repeats > 0 ? w.repeats : 1;
    double total = 0.0, rew = 0.0;
    bool te = false, tr = false, active = true;
    for (int j = 0; j < trips; j++) {
        if (active) {
            if constexpr (HasStepDraws<E>::value) {
                if (E::step_draws(L.trig)) E::step_drawn(L.trig, g.next_double()), drew = true;
            }
            E::step(L.s, L.flags, a, d.P, rew, te, L.trig);
            L.elapsed += 1;
            tr = d.max_steps > 0 && (int)L.elapsed >= d.max_steps;
            total += rew;  // total_reward = 0.0; total_reward += float(reward), in inner order
            active = !(te || tr);
            if constexpr (MAXSKIP) {
                // before the `break`, as in the reference.  j is wave-uniform: a scalar branch around ONE inlined E::obs for the two trips that
                // write a slot (two call sites cost Pendulum's rollout ~25 VGPRs: past the 256 that keep its inline-asm FMAs clear of AGPR copies)
                if (j >= trips - 2) {
                    float frame[E::OBS];
                    E::obs(L.s, L.flags, frame, L.trig);
                    const bool last = j == trips - 1;
#pragma unroll
                    for (int k = 0; k < E::OBS; k++) sl.f[0][k] = last ? sl.f[0][k] : frame[k], sl.f[1][k] = last ? frame[k] : sl.f[1][k];
                    sl.written = 1u;
                }
            }
        }
    }
    if (w.repeats > 0) rew = total;  // (without RepeatAction the one reward as it is, the sign of a zero included)
    // what the vector level sees (RecordEpisodeStatistics, mi_stats): ONE step of this sub-environment with the summed reward
    L.ep_ret += rew, L.ep_len += 1;
    st.env_steps++;
    const bool done = te || tr;
    o.ep_ret = done ? L.ep_ret : 0.0;
    o.ep_len = done ? L.ep_len : 0;
    if (done) {
        st.episodes++;
        st.return_sum += L.ep_ret;
        st.length_sum += (uint64_t)L.ep_len;
    }
    if (MODE == MI_AUTORESET_SAME_STEP && done) {
        if constexpr (MAXSKIP)
            sl.max_frame(o.final_obs);
        else
            E::obs(L.s, L.flags, o.final_obs, L.trig);  // the last INNER observation
        o.has_final = true;
        lane_autoreset<E>(d, i, L, q, &own);  // (without a queue: continues from `own` and stores it)
        sl.word = 0u;
    } else if (!q && drew) {
        store_rng_state(d, i, own);
    }
    if constexpr (MAXSKIP) {
        if (MODE == MI_AUTORESET_SAME_STEP && done)
            E::obs(L.s, L.flags, o.obs, L.trig);  // the reset's observation
        else
            sl.max_frame(o.obs);
    } else {
        E::obs(L.s, L.flags, o.obs, L.trig);
    }
    o.reward = rew, o.terminated = te, o.truncated = tr;
    if (done && MODE != MI_AUTORESET_SAME_STEP)
        L.flags |= kNeedsReset;
    else
        L.flags &= ~kNeedsReset;
}

template <int W>
MI_DEV void store_row(float *dst, const float *src) {
    if (W == 4) {
        *reinterpret_cast<float4 *>(dst) = make_float4(src[0], src[1], src[2], src[3]);
    } else if (W == 2) {
        *reinterpret_cast<float2 *>(dst) = make_float2(src[0], src[1]);
    } else if (W == 6) {
        float2 *p = reinterpret_cast<float2 *>(dst);
        p[0] = make_float2(src[0], src[1]), p[1] = make_float2(src[2], src[3]), p[2] = make_float2(src[4], src[5]);
    } else {
#pragma unroll
        for (int k = 0; k < W; k++) dst[k] = src[k];
    }
}

template <int W>
MI_DEV void load_row(const float *src, float *dst) {
#pragma unroll
    for (int k = 0; k < W; k++) dst[k] = src[k];
}

// The lane's two frames: requested with the rest of the lane (arrive_skip_lane pins the loads where they were issued, like LaneRequest::arrive) and
// stored back by a launch that wrote a slot.  mi_reset, mi_set_state and the autoreset paths never come here.
template <class E>
MI_DEV void load_skip_lane(const WrapSkipDev &w, const DevEnv &d, int i, SkipWrapLane<E> &s) {
    load_row<E::OBS>(w.frames + (size_t)i * E::OBS, s.f[0]);
    load_row<E::OBS>(w.frames + ((size_t)d.N + i) * E::OBS, s.f[1]);
    s.written = 0u;
}
template <class E>
MI_DEV void arrive_skip_lane(SkipWrapLane<E> &s) {
#pragma unroll
    for (int k = 0; k < E::OBS; k++) hold_opaque(s.f[0][k]), hold_opaque(s.f[1][k]);
}
template <class E>
MI_DEV void store_skip_lane(const WrapSkipDev &w, const DevEnv &d, int i, const SkipWrapLane<E> &s) {
    if (!s.written) return;
    store_row<E::OBS>(w.frames + (size_t)i * E::OBS, s.f[0]);
    store_row<E::OBS>(w.frames + ((size_t)d.N + i) * E::OBS, s.f[1]);
}

}  // namespace
#endif  // MI355ENV_LANE_STEP_H
