// mj_wrapped_kernels.h -- RepeatAction / StickyAction of the scalar envs (wrappers/stateful_action.py:16-220) for the MuJoCo family: the wrapped form of
// mj_lane_step and the two kernels that run it.  lane_step_wrapped (lane_step.h) restates the same semantics for the classic kinds inside ONE launch; a
// MuJoCo step may be two launches already (cooperative physics, then glue), so here one outer step is a series of TRIPS on the env's stream:
//
//     mj_wrap_open_kernel                       the sticky decision of every row, its effective action row, a zero accumulator, its inner-step word
//     k x [ mj_physics_kernel -> ] mj_trip_kernel   one inner step of every row still in the series (k = num_repeats, 1 without RepeatAction)
//
// with no synchronisation in between.  A row leaves the series in the trip in which it terminates or truncates (TimeLimit counts inner steps), or in the
// last trip: that trip FINALISES it -- outputs, episode bookkeeping, LaneStats, a SAME_STEP autoreset, the kNeedsReset flag -- and sets the skip bit of
// its inner-step word, which the cooperative physics kernel takes as its `meta` (mjx_physics.h Args: a row whose masked bit is set retires its lanes)
// and the later trips' glue tests first.  The flag word of the state (DevEnv::meta) carries nothing new.
// mujoco.hip instantiates mj_trip_kernel over the stock models, mjx_model.hip and mjx_mass_model.hip over the per-lane-model env types; the plain kernels
// of mj_glue_kernels.h are not touched.
#ifndef MI355ENV_MJ_WRAPPED_KERNELS_H
#define MI355ENV_MJ_WRAPPED_KERNELS_H
#include "mj_glue_kernels.h"

namespace {

constexpr uint32_t kMjInnerSkip = 1u << 31;    // inner-step word: the row takes no (further) inner step in this outer step; bits 0..30: inner steps taken
constexpr uint32_t kMjStickyHasLast = 1u << 31;  // sticky word, as WrapDev::sticky_word: last_action is not None; bits 0..30: repeats_taken

// Opens an outer step.  StickyAction.action (:118-142) with an int duration, per row, BEFORE anything else the row's generator does in this step: a row
// that has a last action and is not inside a series draws np_random.uniform() from its own PCG64 (DevEnv::rng; the advanced state is stored) and starts a
// series if the draw is below p.  The effective action -- the last one while a series lasts -- becomes the last action: ONE array serves as both, and
// the trips read it where the plain step reads the caller's rows.  A row in its NEXT_STEP autoreset step draws nothing and loses its sticky state
// (StickyAction.reset, :107-116); a finished row under DISABLED is left as it is, its generator and sticky state included.  Under SAME_STEP every row steps.
// nu / act_f64 / mode are grid-uniform.
__global__ __launch_bounds__(kBlock) void mj_wrap_open_kernel(DevEnv d, MjWrapDev w, const void *actions, int nu, int act_f64, int mode) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.N) return;
    const bool resetting = mode != MI_AUTORESET_SAME_STEP && ((d.meta[i] >> kFlagShift) & kNeedsReset);
    w.acc[i] = 0.0;
    w.inner[i] = resetting ? kMjInnerSkip : 0u;
    if (!w.sticky_duration) return;
    if (resetting) {
        if (mode == MI_AUTORESET_NEXT_STEP) w.sticky_word[i] = 0u;
        return;
    }
    const uint32_t word = w.sticky_word[i];
    uint32_t taken = word & ~kMjStickyHasLast;
    bool stick = taken != 0u;  // already stuck: no draw
    if (!stick && (word & kMjStickyHasLast)) {
        Pcg64 g = load_rng(d, i);
        stick = g.next_double() < w.sticky_p;  // np_random.uniform() < p, float64
        store_rng_state(d, i, g);
    }
    taken = stick ? taken + 1u : 0u;
    taken = taken == (uint32_t)w.sticky_duration ? 0u : taken;  // the series is over: is_sticky_actions, num_repeats, repeats_taken cleared
    w.sticky_word[i] = kMjStickyHasLast | taken;
    if (stick) return;  // the row's last action stays the effective one
    const size_t row = (size_t)i * (size_t)nu;
    if (act_f64) {
        for (int u = 0; u < nu; u++) static_cast<double *>(w.last_action)[row + u] = static_cast<const double *>(actions)[row + u];
    } else {
        for (int u = 0; u < nu; u++) static_cast<float *>(w.last_action)[row + u] = static_cast<const float *>(actions)[row + u];
    }
}

// One trip of one row that is still in the series.  `extras` as in mj_lane_step.  `mode` and `trip` are grid-uniform (a kernel argument, not a template
// parameter: every instantiation holds a whole one-lane simulator).  Returns whether the row was finalised; reward / te / tr / out_ret / out_len are
// the outer step's then.
template <class E, bool COOP>
MI_DEV bool mj_lane_trip(const DevEnv &d, const MjWrapDev &w, int mode, int trip, int i, MjLane<E> &L, const mjx::ActRow action, double *obs, double *final_obs,
                         double *info, double &reward, bool &te, bool &tr, double &out_ret, int32_t &out_len, LaneStats &st, const double *extras, double *final_info,
                         const MjLaneFields<E> *lane) {
    te = tr = false, reward = 0.0, out_ret = 0.0, out_len = 0;
    if (mode == MI_AUTORESET_NEXT_STEP && (L.flags & kNeedsReset)) {
        // sync_vector_env.py:279-284: the step after a finished episode resets, ignores the action, repeats nothing and returns reward 0
        mj_autoreset<E>(d, i, L, obs, lane);
        if (info) E::reset_info(L.s, info);
        st.reset_steps++;
        L.flags &= ~kNeedsReset;
        return true;
    }
    if (mode == MI_AUTORESET_DISABLED && (L.flags & kNeedsReset)) {
        *d.error = kErrDisabledStepped;
        return true;
    }
    if (COOP) {
        typedef mjx::coop::Sim<typename E::Model, E::COOP_G> S;
        typename E::StepExtras x;
        E::after_from_extras(L.s, extras, x.after);
        x.cfrc = reinterpret_cast<const double (*)[6]>(extras + S::EX_CFRC);
        x.cinert = reinterpret_cast<const double (*)[10]>(extras + S::EX_CINERT);
        x.cvel = reinterpret_cast<const double (*)[6]>(extras + S::EX_CVEL);
        x.qfrc_actuator = extras + S::EX_QFA;
        x.qfrc_constraint = nullptr;
        x.ten = extras + S::EX_TEN;
        const double before[2] = {L.s[E::NQ + 2 * E::NV], L.s[E::NQ + 2 * E::NV + 1]};
        E::finish(L.s, before, x, action, d.P, obs, reward, te, info);
    } else {
        E::step(L.s, action, d.P, obs, reward, te, info, d.solver_newton != 0, lane);
    }
    // RepeatAction.step (:197-220) over TimeLimit.step (wrappers/common.py:129-133): elapsed counts INNER steps
    L.elapsed += 1;
    tr = d.max_steps > 0 && (int)L.elapsed >= d.max_steps;
    if (w.repeats > 0) {  // total_reward = 0.0; total_reward += float(reward), in inner order (without RepeatAction the one reward as it is)
        reward = w.acc[i] + reward;
        w.acc[i] = reward;
    }
    const bool done = te || tr;
    if (!done && trip + 1 < (w.repeats > 0 ? w.repeats : 1)) {
        te = tr = false;
        return false;
    }
    // what the vector level sees (RecordEpisodeStatistics, mi_stats): ONE step of this sub-environment with the summed reward
    L.ep_ret += reward, L.ep_len += 1;
    st.env_steps++;
    out_ret = done ? L.ep_ret : 0.0, out_len = done ? L.ep_len : 0;
    if (done) st.episodes++, st.return_sum += L.ep_ret, st.length_sum += (uint64_t)L.ep_len;
    if (mode == MI_AUTORESET_SAME_STEP && done) {  // final_obs / final_info: the last INNER step's; the top-level entries: the reset's
        if (final_obs)
            for (int k = 0; k < E::obs_dim(d.P); k++) final_obs[k] = obs[k];
        if (info && final_info)
            for (int k = 0; k < E::INFO; k++) final_info[k] = info[k];
        mj_autoreset<E>(d, i, L, obs, lane);
        if (info) E::reset_info(L.s, info);
        if (w.sticky_duration) w.sticky_word[i] = 0u;  // StickyAction.reset
    }
    if (done && mode != MI_AUTORESET_SAME_STEP)
        L.flags |= kNeedsReset;
    else
        L.flags &= ~kNeedsReset;
    return true;
}

// Trip `trip` of an outer step: rows whose inner-step word has the skip bit sit it out -- except in trip 0, where that bit marks the rows in their autoreset
// step (NEXT_STEP) or finished ones (DISABLED), which mj_lane_trip deals with as mj_lane_step does.  io.actions: the effective rows.
template <class E, bool COOP>
__global__ __launch_bounds__(kBlock) void mj_trip_kernel(DevEnv d, MjStepPtrs io, MjWrapDev w, int mode, int trip) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    if (i < d.N) {
        const uint32_t word = w.inner[i];
        if (trip == 0 || !(word & kMjInnerSkip)) {
            MjLane<E> L;
            mj_load<E>(d, i, L);
            double reward, out_ret;
            int32_t out_len;
            bool te, tr;
            const mjx::ActRow a = {static_cast<const char *>(io.actions) + (size_t)i * E::NU * (io.act_f64 ? 8 : 4), io.act_f64 != 0};
            MjLaneHolder<E> lane;
            lane.load(d, i);
            const bool stepped = !(word & kMjInnerSkip);
            const double *extras = nullptr;
            if constexpr (COOP) extras = io.extras + (size_t)i * mjx::coop::Sim<typename E::Model, E::COOP_G>::EX_TOTAL;
            const bool final = mj_lane_trip<E, COOP>(d, w, mode, trip, i, L, a, io.obs + (size_t)i * io.obs_dim,
                                                     io.final_obs ? io.final_obs + (size_t)i * io.obs_dim : nullptr, io.info ? io.info + (size_t)i * E::INFO : nullptr,
                                                     reward, te, tr, out_ret, out_len, st, extras, io.final_info ? io.final_info + (size_t)i * E::INFO : nullptr, lane.get());
            mj_store<E>(d, i, L);
            w.inner[i] = (final ? kMjInnerSkip : 0u) | ((word & ~kMjInnerSkip) + (stepped ? 1u : 0u));
            if (final) {
                if (io.reward) io.reward[i] = reward;
                if (io.terminated) io.terminated[i] = te;
                if (io.truncated) io.truncated[i] = tr;
                if (io.ep_ret) io.ep_ret[i] = out_ret;
                if (io.ep_len) io.ep_len[i] = out_len;
            }
        }
    }
    block_accumulate(d, st);
}

}  // namespace
#endif  // MI355ENV_MJ_WRAPPED_KERNELS_H
