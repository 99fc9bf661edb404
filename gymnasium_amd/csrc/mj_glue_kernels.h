// mj_glue_kernels.h -- the per-lane kernels of the MuJoCo family around the simulator of mjx_kernels.h: the vectoriser's state machine, reward,
// observation and statistics of one sub-environment per lane.  mujoco.hip instantiates them over the stock models, mjx_model.hip over the
// mjx::LaneModel env types, mjx_mass_model.hip over the mjx::MassLaneModel ones.
#ifndef MI355ENV_MJ_GLUE_KERNELS_H
#define MI355ENV_MJ_GLUE_KERNELS_H
#include <type_traits>

#include "lane_common.h"
#include "mjx_kernels.h"
#include "mjx_coop.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// MuJoCo-family kernels (mjx_kernels.h): same vectoriser state machine, float64 observations, float32 action rows
// ---------------------------------------------------------------------------------------------------------
template <class E>
struct MjLane {
    double s[E::S];
    uint32_t elapsed, flags;
    double ep_ret;
    int32_t ep_len;
};
// The sub-environment's own model fields of an env type over a mjx::LaneModel (void, and nothing to load, for the stock models): loaded once per launch
template <class E>
using MjLaneFields = typename mjx::ModelView<typename E::Model>::Fields;
template <class E>
struct MjLaneHolder {
    static constexpr bool HAS = !std::is_void<MjLaneFields<E>>::value;
    typename std::conditional<HAS, MjLaneFields<E>, char>::type fields;  // (a byte nobody touches for the stock models)
    MI_DEV void load(const DevEnv &d, int i) {
        if constexpr (HAS) fields.load(d.mj.rows, (size_t)d.N, (size_t)i);
    }
    MI_DEV const MjLaneFields<E> *get() const {
        if constexpr (HAS)
            return &fields;
        else
            return nullptr;
    }
};
template <class E>
MI_DEV void mj_load(const DevEnv &d, int i, MjLane<E> &L) {
    for (int k = 0; k < E::S; k++) L.s[k] = d.state[(size_t)k * d.N + i];
    const uint32_t m = d.meta[i];
    L.elapsed = m & kElapsedMask, L.flags = m >> kFlagShift;
    L.ep_ret = d.ep_ret[i], L.ep_len = d.ep_len[i];
}
template <class E>
MI_DEV void mj_store(const DevEnv &d, int i, const MjLane<E> &L) {
    for (int k = 0; k < E::S; k++) d.state[(size_t)k * d.N + i] = L.s[k];
    d.meta[i] = (L.elapsed & kElapsedMask) | (L.flags << kFlagShift);
    d.ep_ret[i] = L.ep_ret, d.ep_len[i] = L.ep_len;
}
template <class E>
MI_DEV void mj_autoreset(const DevEnv &d, int i, MjLane<E> &L, double *obs, const MjLaneFields<E> *lane = nullptr) {
    Pcg64 rng = load_rng(d, i);
    if constexpr (mjx::ModelView<typename E::Model>::MASS_PER_LANE)
        E::reset(rng, L.s, d.P, obs, lane);  // (the Humanoids' reset reads the lane's body masses)
    else
        E::reset(rng, L.s, d.P, obs);
    store_rng_state(d, i, rng);
    L.elapsed = 0, L.ep_ret = 0.0, L.ep_len = 0;
}

// one lockstep step of one MuJoCo sub-environment; obs / info rows are written straight to their destination
// `extras` != nullptr: the physics of this step was already advanced by mj_physics_kernel (L.s holds the new qpos / qvel
// and the old tracked point); nullptr: the one-lane simulator runs here.
template <class E, int MODE, bool COOP = false>
MI_DEV void mj_lane_step(const DevEnv &d, int i, MjLane<E> &L, const mjx::ActRow action, double *obs, double *final_obs, double *info,
                         double &reward, bool &te, bool &tr, double &out_ret, int32_t &out_len, LaneStats &st,
                         const double *extras = nullptr, double *final_info = nullptr, const MjLaneFields<E> *lane = nullptr) {
    te = tr = false, reward = 0.0;
    if (MODE == MI_AUTORESET_NEXT_STEP && (L.flags & kNeedsReset)) {
        mj_autoreset<E>(d, i, L, obs, lane);
        if (info) E::reset_info(L.s, info);
        st.reset_steps++;
    } else if (MODE == MI_AUTORESET_DISABLED && (L.flags & kNeedsReset)) {
        *d.error = kErrDisabledStepped;
        out_ret = 0.0, out_len = 0;
        return;
    } else {
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
        L.elapsed += 1;
        tr = d.max_steps > 0 && (int)L.elapsed >= d.max_steps;
        L.ep_ret += reward, L.ep_len += 1;
        st.env_steps++;
    }
    const bool done = te || tr;
    out_ret = done ? L.ep_ret : 0.0, out_len = done ? L.ep_len : 0;
    if (done) st.episodes++, st.return_sum += L.ep_ret, st.length_sum += (uint64_t)L.ep_len;
    if (MODE == MI_AUTORESET_SAME_STEP && done) {
        if (final_obs)
            for (int k = 0; k < E::obs_dim(d.P); k++) final_obs[k] = obs[k];
        if (info && final_info)  // sync_vector_env.py:309-317: the finishing step's info goes to "final_info" ...
            for (int k = 0; k < E::INFO; k++) final_info[k] = info[k];
        mj_autoreset<E>(d, i, L, obs, lane);
        if (info) E::reset_info(L.s, info);  // ... and the top-level entries of this sub-env are its reset info (:319)
    }
    if (done && MODE != MI_AUTORESET_SAME_STEP)
        L.flags |= kNeedsReset;
    else
        L.flags &= ~kNeedsReset;
}

template <class E, int MODE, bool COOP>
__global__ __launch_bounds__(kBlock) void mj_step_kernel(DevEnv d, MjStepPtrs io) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    if (i < d.N) {
        MjLane<E> L;
        mj_load<E>(d, i, L);
        double reward, out_ret;
        int32_t out_len;
        bool te, tr;
        const mjx::ActRow a = {static_cast<const char *>(io.actions) + (size_t)i * E::NU * (io.act_f64 ? 8 : 4), io.act_f64 != 0};
        // Two spellings of one call, on purpose: with a holder object in the stock instantiations -- even an empty one, as in mj_rollout_kernel -- the
        // DISABLED-mode kernels of the stock robots come out with two instructions in another order (scripts/kernel_stream_diff.py), and the stock
        // kernels are to stay what they were instruction for instruction.
        if constexpr (MjLaneHolder<E>::HAS) {
            MjLaneHolder<E> lane;
            lane.load(d, i);
            mj_lane_step<E, MODE, false>(d, i, L, a, io.obs + (size_t)i * io.obs_dim,
                                         io.final_obs ? io.final_obs + (size_t)i * io.obs_dim : nullptr,
                                         io.info ? io.info + (size_t)i * E::INFO : nullptr, reward, te, tr, out_ret, out_len, st, nullptr,
                                         io.final_info ? io.final_info + (size_t)i * E::INFO : nullptr, lane.get());
        } else {
            mj_lane_step<E, MODE, COOP>(d, i, L, a, io.obs + (size_t)i * io.obs_dim,
                                        io.final_obs ? io.final_obs + (size_t)i * io.obs_dim : nullptr,
                                        io.info ? io.info + (size_t)i * E::INFO : nullptr, reward, te, tr, out_ret, out_len, st,
                                        COOP ? io.extras + (size_t)i * mjx::coop::Sim<typename E::Model, E::COOP_G>::EX_TOTAL : nullptr,
                                        io.final_info ? io.final_info + (size_t)i * E::INFO : nullptr);
        }
        mj_store<E>(d, i, L);
        if (io.reward) io.reward[i] = reward;
        if (io.terminated) io.terminated[i] = te;
        if (io.truncated) io.truncated[i] = tr;
        if (io.ep_ret) io.ep_ret[i] = out_ret;
        if (io.ep_len) io.ep_len[i] = out_len;
    }
    block_accumulate(d, st);
}

template <class E>
__global__ __launch_bounds__(kBlock) void mj_reset_kernel(DevEnv d, const uint8_t *mask, double *obs, int obs_dim) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.N || (mask && !mask[i])) return;
    MjLane<E> L;
    mj_load<E>(d, i, L);
    L.flags &= ~kNeedsReset;
    if constexpr (MjLaneHolder<E>::HAS) {  // (two spellings, as in mj_step_kernel: the stock kernels stay what they were)
        MjLaneHolder<E> lane;
        lane.load(d, i);
        mj_autoreset<E>(d, i, L, obs ? obs + (size_t)i * obs_dim : nullptr, lane.get());
    } else {
        mj_autoreset<E>(d, i, L, obs ? obs + (size_t)i * obs_dim : nullptr);
    }
    mj_store<E>(d, i, L);
}

// fused rollout: T steps per launch, Box action space sampled on device from the batched space's single PCG64 stream
// (draw number (t*N + i)*NU + u belongs to lane i, component u, step t)
// ex (mi_rollout_infos; all members NULL for mi_rollout): per step the info row, the finished episodes' return / length and, under SAME_STEP, the final
// observation and info -- zeros in the rows that finished nothing.
template <class E, int MODE, bool SAMPLE>
__global__ __launch_bounds__(kBlock) void mj_rollout_kernel(DevEnv d, RolloutPtrs io, ActionStream as, int T, int obs_dim, int in_f64, RolloutExtra ex) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    LaneStats st = {0u, 0u, 0u, 0ull, 0.0};
    if (i < d.N) {
        MjLane<E> L;
        mj_load<E>(d, i, L);
        MjLaneHolder<E> lane;
        lane.load(d, i);
        u128 astate = 0;
        const u128 ainc = make_u128(as.inc_hi, as.inc_lo);
        if (SAMPLE) {
            astate = make_u128(as.state_hi, as.state_lo);
            uint64_t delta = (uint64_t)i * E::NU + 1u;
            for (int j = 0; delta; j++, delta >>= 1)
                if (delta & 1u) astate = as.pow2[j].mult * astate + as.pow2[j].plus;
        }
        const size_t N = (size_t)d.N;
        double scratch_obs[E::MAX_OBS], scratch_info[E::INFO > 0 ? E::INFO : 1];
        for (int t = 0; t < T; t++) {
            float a[E::NU];
            mjx::ActRow row = {a, false};
            if (SAMPLE) {
                for (int u = 0; u < E::NU; u++) {
                    const uint64_t hi = (uint64_t)(astate >> 64), lo = (uint64_t)astate, x = hi ^ lo;
                    const unsigned rot = (unsigned)(hi >> 58);
                    const uint64_t out = (x >> rot) | (x << ((0u - rot) & 63u));
                    const double lo_b = (double)(float)E::Model::actuator_ctrlrange[u][0], hi_b = (double)(float)E::Model::actuator_ctrlrange[u][1];
                    a[u] = (float)(lo_b + (hi_b - lo_b) * ((double)(out >> 11) * (1.0 / 9007199254740992.0)));
                    if (u + 1 < E::NU) astate = astate * pcg_mult() + ainc;
                }
                astate = as.jump_n.mult * astate + as.jump_n.plus;
                if (io.actions_out)
                    for (int u = 0; u < E::NU; u++) static_cast<float *>(io.actions_out)[(t * N + i) * E::NU + u] = a[u];
            } else {  // the caller's rows, read in place
                row.p = static_cast<const char *>(io.actions_in) + (t * N + i) * E::NU * (in_f64 ? 8 : 4), row.f64 = in_f64 != 0;
            }
            double reward, out_ret;
            int32_t out_len;
            bool te, tr;
            double *obs = io.obs ? static_cast<double *>(io.obs) + (t * N + i) * obs_dim : scratch_obs;
            double *fobs = ex.final_obs ? static_cast<double *>(ex.final_obs) + (t * N + i) * obs_dim : nullptr;
            double *finfo = ex.final_info ? ex.final_info + (t * N + i) * E::INFO : nullptr;
            // (the finishing step's info reaches final_info through the info row: without a caller's array a private row serves)
            double *info = ex.info ? ex.info + (t * N + i) * E::INFO : (finfo ? scratch_info : nullptr);
            mj_lane_step<E, MODE>(d, i, L, row, obs, fobs, info, reward, te, tr, out_ret, out_len, st, nullptr, finfo, lane.get());
            if (io.reward) io.reward[t * N + i] = reward;
            if (io.terminated) io.terminated[t * N + i] = te;
            if (io.truncated) io.truncated[t * N + i] = tr;
            if (ex.ep_ret) ex.ep_ret[t * N + i] = out_ret;
            if (ex.ep_len) ex.ep_len[t * N + i] = out_len;
            if (!(te || tr)) {
                if (fobs)
                    for (int k = 0; k < obs_dim; k++) fobs[k] = 0.0;
                if (finfo)
                    for (int k = 0; k < E::INFO; k++) finfo[k] = 0.0;
            }
        }
        mj_store<E>(d, i, L);
    }
    block_accumulate(d, st);
}

// Box.sample() of the batched action space for step t of a rollout: draw number (t N + i) NU + u of the stream
template <class E>
__global__ __launch_bounds__(kBlock) void mj_sample_kernel(DevEnv d, ActionStream as, int t, float *out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.N) return;
    const u128 ainc = make_u128(as.inc_hi, as.inc_lo);
    u128 astate = make_u128(as.state_hi, as.state_lo);
    uint64_t delta = ((uint64_t)t * (uint64_t)d.N + (uint64_t)i) * E::NU + 1u;
    for (int j = 0; delta; j++, delta >>= 1)
        if (delta & 1u) astate = as.pow2[j].mult * astate + as.pow2[j].plus;
    for (int u = 0; u < E::NU; u++) {
        const uint64_t hi = (uint64_t)(astate >> 64), lo = (uint64_t)astate, x = hi ^ lo;
        const unsigned rot = (unsigned)(hi >> 58);
        const uint64_t o = (x >> rot) | (x << ((0u - rot) & 63u));
        const double lo_b = (double)(float)E::Model::actuator_ctrlrange[u][0], hi_b = (double)(float)E::Model::actuator_ctrlrange[u][1];
        out[(size_t)i * E::NU + u] = (float)(lo_b + (hi_b - lo_b) * ((double)(o >> 11) * (1.0 / 9007199254740992.0)));
        astate = astate * pcg_mult() + ainc;
    }
}

}  // namespace
#endif  // MI355ENV_MJ_GLUE_KERNELS_H
