// engine_types.h -- what the engine's units (engine.hip, classic.hip, mujoco.hip, tabular.hip, lookahead.hip, lookahead_policy.hip, mjx_model.hip and mjx_mass_model.hip) agree on: the
// constants of the lane's flag word, the plain structs that ride in kernel arguments and in mi_vecenv, the handle itself, the launch functions one
// unit defines and another calls, and the error helpers of the host side.  No kernel and no device function lives here.
#ifndef MI355ENV_ENGINE_TYPES_H
#define MI355ENV_ENGINE_TYPES_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/mi355env.h"
#include "envs_classic.h"
#include "pcg64_dev.h"
#include "action_mask_internal.h"

using namespace mi;

namespace {

constexpr int kBlock = 256;  // 4 wavefronts: one per SIMD of a CU
constexpr int kErrInvalidAction = 1, kErrDisabledStepped = 2;
constexpr uint32_t kFlagShift = 30, kElapsedMask = (1u << kFlagShift) - 1u;

}  // namespace
// Plain types that cross the boundary between the translation units (launcher arguments, members of mi_vecenv): a named namespace, so that
// mi_classic's functions have external linkage.
namespace mi_internal {
// Transition table of a tabular (ToyText) environment, device pointers (mi_tabular_load).
struct TabTable {
    int nS, nA, K;
    const double *csprob, *prob, *reward, *isd;
    const int32_t *next, *count;
    const uint8_t *term;
    const int32_t *env_table;  // [N] table of each sub-environment when there are several (mi_tabular_table.num_tables > 1), else nullptr
};

// Per-sub-environment model fields of a MuJoCo env (mi_set_model_field), as they ride in DevEnv.
struct MjModelDev {
    int tab_ints[3];     // tab.nS, tab.nA, tab.K of the union below: always 0 here
    const double *rows;  // [mjx::MassLaneFields::WIDTH][N], read by the mjx::LaneModel / MassLaneModel instantiations only; NULL until the first mi_set_model_field
};
// Device view of one vector environment (passed by value as a kernel argument).
struct DevEnv {
    double *state;       // [S][N]   physics state, component-major
    uint32_t *meta;      // [N]      TimeLimit elapsed steps (bits 0..29) | flags (bits 30..31)
    uint64_t *rng;       // [4][N]   PCG64 {state_hi, state_lo, inc_hi, inc_lo}
    double *ep_ret;      // [N]      running episode return
    int32_t *ep_len;     // [N]      running episode length
    uint64_t *blk_count; // [grid][4] per-workgroup totals: env_steps, reset_steps, episodes, length_sum
    double *blk_ret;     // [grid]    per-workgroup sum of finished-episode returns
    int *error;          // sticky device error word
    int N;
    int max_steps;
    int solver_newton;   // MI_CFG_SOLVER_NEWTON (one-lane MuJoCo kernels; the cooperative kernel is chosen at launch)
    int tab_fickle_rows; // MI_ENV_TABULAR with params[2] != 0 (Taxi's fickle passenger): the state has a third row (TabLane::aux)
    EnvParams P;
    // By kind; the size and layout of DevEnv are the table's, as before the union.  Kernels of EVERY kind read tab.nS (seed_words_kernel /
    // seed_sequence_kernel: < 0 is the Blackjack marker), so the pointer of the MuJoCo kinds lies behind the table's three integers, which stay 0 for
    // them: it shares its bytes with tab.csprob, which only the tabular kernels read.
    union {
        TabTable tab;  // the tabular kinds
        MjModelDev mj; // the MuJoCo kinds
    };
};
static_assert(offsetof(MjModelDev, rows) == offsetof(TabTable, csprob) && sizeof(MjModelDev) <= sizeof(TabTable), "mj.rows must alias a pointer of the table, not nS / nA / K");
// Per-sub-environment attributes (mi_set_env_attr; the *AttrT types of envs_classic.h): attribute a of sub-environment i is rows[a * N + i] if bit
// a of `mask` is set, else its construction value.  An extra argument of step_kernel / rollout_kernel, which the other types do not read.
struct AttrDev {
    const double *rows;  // [A][N] component-major, like DevEnv::state
    uint32_t mask;       // wave-uniform
};
// The per-sub-environment action wrappers of the reference (wrappers/stateful_action.py) folded into the step (mi_set_step_wrappers): the last
// argument of step_wrapped_kernel / rollout_wrapped_kernel, which the env runs instead of step_kernel / rollout_kernel / rollout_infos_kernel then.
// Everything but the two arrays is wave-uniform.
struct WrapDev {
    int repeats;            // RepeatAction(env, repeats): inner steps per step(); 0: no such wrapper
    int sticky_duration;    // StickyAction(env, p, duration); 0: no such wrapper
    double sticky_p;
    uint64_t *last_action;  // [N] StickyAction.last_action: the bits of the lane's last effective action (E::Act)
    uint32_t *sticky_word;  // [N] bit 31: last_action is not None; bits 0..30: repeats_taken (is_sticky_actions <=> > 0; num_repeats is then the duration)
};
// ... and with MaxAndSkipObservation(env, skip) (wrappers/stateful_observation.py:564-649; mi_set_max_and_skip): what the env holds (mi_vecenv::wrap) and
// what the MAXSKIP instantiations of the two kernels take.  The others go on taking the WrapDev part alone: a longer argument would move the hidden
// kernel arguments behind it, and with them a literal in every existing instantiation.  In the env `repeats` is 0 while `skip` is on; the copy that
// a MAXSKIP kernel is launched with carries the skip as `repeats` too (classic.hip wrap_arg): RepeatAction's loop runs it.
struct WrapSkipDev : WrapDev {
    int skip;       // inner steps per step(); 0: no such wrapper
    float *frames;  // [2][N][OBS] the wrappers' _obs_buffer: slot-major, one OBS-wide row per lane (load_row / store_row: consecutive lanes, consecutive rows)
};
template <bool MAXSKIP>
using WrapArg = std::conditional_t<MAXSKIP, WrapSkipDev, WrapDev>;
// The same two wrappers for the MuJoCo kinds (mj_wrapped_kernels.h): an outer step is `repeats` trips of the plain step's launches, and what a row
// carries from trip to trip lives here.  Everything but the arrays is grid-uniform.
struct MjWrapDev {
    int repeats, sticky_duration;  // as WrapDev
    double sticky_p;
    void *last_action;      // [N][NU] StickyAction.last_action in the element type of the action rows (allocated at 8 bytes per component); after
                            // mj_wrap_open_kernel it IS the effective action row of the step, which the trips read.  NULL without StickyAction
    uint32_t *sticky_word;  // [N] as WrapDev::sticky_word
    double *acc;            // [N] RepeatAction's total_reward of the outer step in flight
    uint32_t *inner;        // [N] inner-step word: bit 31 the row sits the remaining trips out (the cooperative physics kernel's `meta`), bits 0..30 inner steps taken
};
}  // namespace mi_internal
using namespace mi_internal;
namespace {
// sizes of the step epilogue's rows (engine.hip): up to kEpiObsMax observation columns; beyond kEpiFoldMax step workgroups the fold is a launch of its own
constexpr int kEpiObsMax = 6, kEpiCols = 2 * kEpiObsMax + 3, kEpiFoldMax = 1024;
}  // namespace
namespace mi_internal {
struct EpiDev {
    int obs_on, obs_update, ret_on, ret_update, same_step, clip_pre, clip_post, fold_in_finish;  // clip_*: bit 0 = has min, bit 1 = has max
    int step_blocks;
    float gamma;
    double obs_eps, ret_eps, pre_lo, pre_hi, post_lo, post_hi;
    double *obs_mean, *obs_var, *obs_count, *ret_mean, *ret_var, *ret_count;              // the statistics before this step (read only)
    double *obs_mean2, *obs_var2, *obs_count2, *ret_mean2, *ret_var2, *ret_count2;        // where the updated ones go
    float *acc;
    uint8_t *prev_done;
    double *partial;   // [step_blocks][kEpiCols]
};
struct StepPtrs {
    const void *actions;
    float *obs;
    double *reward;
    uint8_t *terminated, *truncated;
    float *final_obs;
    double *ep_ret;
    int32_t *ep_len;
    // the on-device policy (mi_step with actions == NULL): per-lane states of the action stream [2][N] (lane i: the state whose output is draw
    // pos + i * act_dim), where the drawn actions go (or nullptr), and the jump to the lane's slot in the next batch (N * act_dim draws on)
    uint64_t *act_lane;
    void *actions_out;
    PcgJump act_jump;
};
// Action stream of the batched action space: ONE PCG64 generator drawn in sub-environment index order, so lane i
// consumes draw number t*N + i of the stream at step t.  jump[j] advances by 2^j draws; jump_n advances by N.
struct ActionStream {
    uint64_t state_hi, state_lo, inc_hi, inc_lo;
    const PcgJump *pow2;  // [64] device
    PcgJump jump_n;
    // the classic kinds' sampling rollouts (rollout_kernel, rollout_duo_kernel): the per-lane states (act_lane[2][N], act_init_kernel's meaning)
    // the launch leaves behind -- a lane writes its state after the last jump, i.e. its state for the position T * N draws on.  nullptr: none
    // (the other kernels; a launch inside a stream capture).  lane_valid: they hold the launch's start already, so no skip-ahead from state_hi / lo.
    uint64_t *lane;
    int lane_valid;
};

struct RolloutPtrs {
    const void *actions_in;
    void *actions_out;
    void *obs;
    double *reward;
    uint8_t *terminated, *truncated;
};
// What a rollout stores besides RolloutPtrs (mi_rollout_extra, same meaning; every member nullable): a kernel argument of its own, taken only by the
// kernels that store them -- RolloutPtrs, which the two-role and the branch-free kernels take by value, stays what it is.
struct RolloutExtra {
    void *final_obs;
    double *ep_ret;
    int32_t *ep_len;
    double *info, *final_info;
};
// MI_CFG_SHARED_RNG (include/mi355env.h): CartPoleVectorEnv's ONE generator on the device.  It is kept as a fixed BASE state (what mi_seed gave) plus
// the number of draws taken since: draw number n of the stream is the output after skipping n steps ahead of the base (Brown's O(log n) jump through
// the pow2 table), so every lane finds its own draws without a serial pass and nothing but two counters ever changes.
struct SharedRng {
    uint64_t *words;       // [8] device: base {state_hi, state_lo, inc_hi, inc_lo}, [4] consumed, [5] pos_base = first draw of the call in flight, [6] k = sub-envs it re-draws,
                           // [7] != 0: a batch with an action outside the space was refused (shared_validate_kernel) -- every later step is a no-op until the host has raised it
    const PcgJump *pow2;   // [64] device: jump by 2^j steps of the base generator's increment
    uint32_t *blk_done;    // [grid] sub-environments of each step workgroup that finished an episode in the previous step
    uint32_t *blk_prefix;  // [grid] exclusive scan of blk_done (shared_scan_kernel)
    double low, high;      // self.low / self.high (cartpole.py:489-491): the bounds of the last reset() serve the autoresets
};
// Per-sub-environment model fields of a MuJoCo kind (include/mi355env.h MI_MODEL_*; device side: mjx::LaneModel): where each field lies in the env's
// rows and the compiled-in values it starts from (mi_mujoco::model_field_info).
struct ModelFieldInfo {
    int width[MI_MODEL_FIELD_COUNT], offset[MI_MODEL_FIELD_COUNT], total;
    const double *defaults[MI_MODEL_FIELD_COUNT];
    // the rows derived from the body mass scale (MI_MODEL_DERIVED_*) and the compiled model's values of them
    int dwidth[MI_MODEL_DERIVED_COUNT], doffset[MI_MODEL_DERIVED_COUNT];
    const double *dcompiled[MI_MODEL_DERIVED_COUNT];
};
}  // namespace mi_internal
// The classic-control kernels behind plain launch functions (defined in classic.hip, called from engine.hip): what mi_step / mi_reset /
// mi_rollout do for the kinds CARTPOLE ... MOUNTAIN_CAR_CONTINUOUS once the arguments are validated and the buffers chosen.
namespace mi_classic {
int step(mi_vecenv *v, const mi_internal::StepPtrs &p, int act_kind);                                           // launch_step<E> of the env's kind
int reset(mi_vecenv *v, const uint8_t *device_mask, int has_bounds, double b0, double b1, float *device_obs);  // reset_kernel<E>
int rollout(mi_vecenv *v, const mi_internal::RolloutPtrs &p, const mi_internal::ActionStream &as, int T, bool sample, int actions_in_kind);
// ... and with the per-step extras (mi_rollout_infos): always the one-role kernel, the instantiations that store them
int rollout_infos(mi_vecenv *v, const mi_internal::RolloutPtrs &p, const mi_internal::RolloutExtra &ex, const mi_internal::ActionStream &as, int T, bool sample,
                  int actions_in_kind);
// MI_CFG_SHARED_RNG (CartPole only): reset = [bookkeeping, reset kernel]; step = [scan of the finished sub-environments, step kernel];
// rollout = T x [policy sample,] step; recount = blk_done from the flag words (after mi_set_state)
int shared_reset(mi_vecenv *v, float *device_obs);
int shared_step(mi_vecenv *v, const mi_internal::StepPtrs &p);
int shared_rollout(mi_vecenv *v, const mi_internal::RolloutPtrs &p, const mi_internal::ActionStream &as, int T, bool sample, const mi_internal::RolloutExtra *ex = nullptr);
int shared_recount(mi_vecenv *v);
}  // namespace mi_classic
// The MuJoCo family behind plain functions (defined in mujoco.hip, called from engine.hip): likewise for the eleven MuJoCo kinds -- over the stock models, the
// per-sub-environment model fields or the cooperative physics, as the env stands -- and what the host side needs to know about a robot (bool: false for another kind).
namespace mi_mujoco {
bool configure(mi_vecenv *v);  // mi_create: v->lay, v->extras_dim and the v->mj_coop default of v->cfg's robot
bool model_field_info(int kind, mi_internal::ModelFieldInfo &out);
bool action_bounds(int kind, double *lo, double *range);  // Box(low, high, (nu,), float32) from the float32 ctrlrange (mujoco_env.py:113-117): low, high - low
int reset(mi_vecenv *v, const uint8_t *device_mask, double *device_obs);
int step(mi_vecenv *v, const mi_internal::StepPtrs &p, double *info, double *final_info, int act_kind);  // (obs / final_obs are float64 rows here)
int rollout(mi_vecenv *v, const mi_internal::RolloutPtrs &p, const mi_internal::ActionStream &as, int T, bool sample, int in_f64, const mi_internal::RolloutExtra *ex);
}  // namespace mi_mujoco
// The ToyText kernels behind plain launch functions (defined in tabular.hip, called from engine.hip) for MI_ENV_TABULAR and MI_ENV_BLACKJACK; rollout
// chooses among the general, the branch-free and the Blackjack kernels.  The table is v->d.tab (mi_tabular_load).
namespace mi_tabular {
int reset(mi_vecenv *v, const uint8_t *device_mask, int64_t *device_obs);
int step(mi_vecenv *v, const mi_internal::StepPtrs &p, double *info, double *final_info, bool fused_sample);  // (obs / final_obs / actions are int64 rows here)
int rollout(mi_vecenv *v, const mi_internal::RolloutPtrs &p, const mi_internal::ActionStream &as, int T, bool sample, const mi_internal::RolloutExtra *ex);
}  // namespace mi_tabular
// mi_lookahead's kernels behind a plain launch function (defined in lookahead.hip, called from engine.hip once the arguments are validated):
// lookahead_kernel<E> of the env's kind, its per-lane type when the env is on those, and the element type of the action rows (candidate_lane.h's
// dispatch, as for the policy unit below; the candidate loop both units share is that header's).  Device pointers; every output nullable.
// (mi_lookahead_unit: `mi_lookahead` itself is the C entry point's name.)
namespace mi_lookahead_unit {
int launch(mi_vecenv *v, const void *actions, int act_kind, int horizon, int candidates, double gamma, double *returns, int32_t *steps, uint8_t *terminated,
           uint8_t *truncated, float *final_obs);
}  // namespace mi_lookahead_unit
// mi_lookahead_policy's kernels likewise (defined in lookahead_policy.hip): lookahead_policy_kernel<E, LDS> of the env's kind, its per-lane type when the
// env is on those, and the parameter path the launch function chooses.  params_per_candidate: P of a kind and a hidden width (0 for another kind).
namespace mi_lookahead_policy_unit {
int params_per_candidate(int kind, int hidden);
int launch(mi_vecenv *v, const float *params, int hidden, int horizon, int candidates, double gamma, double *returns, int32_t *steps, uint8_t *terminated,
           uint8_t *truncated, float *final_obs);
}  // namespace mi_lookahead_policy_unit
// The one-lane MuJoCo kernels of an env with per-sub-environment model fields (mi_set_model_field) -- mj_step_kernel and mj_rollout_kernel over
// mjx::LaneModel env types -- behind plain launch functions: they are instantiated in a translation unit of their own (mjx_model.hip),
// which compiles side by side with the others.  mujoco.hip launches through them (its lane_launchers; engine.hip calls preload and
// derive_constants only).  `mj_step_ptrs` is an MjStepPtrs -- a type of the unnamed namespace, whose name is
// part of the stock kernels' symbols and therefore stays there; every unit compiles the one definition below.  d.mj.rows are the env's rows.
// false: a kind the unit does not hold.
namespace mi_mjmodel {
bool step(int kind, int autoreset_mode, int grid, hipStream_t stream, const mi_internal::DevEnv &d, const void *mj_step_ptrs);
// mj_trip_kernel (mj_wrapped_kernels.h) over the same env types: trip `trip` of an outer step with RepeatAction / StickyAction on (mi_set_step_wrappers)
bool step_wrapped(int kind, int autoreset_mode, int trip, int grid, hipStream_t stream, const mi_internal::DevEnv &d, const void *mj_step_ptrs,
                  const mi_internal::MjWrapDev &w);
// load the unit's code object on the current device now (kernels load on first use, which a stream capture must not trigger)
bool preload(int kind);
bool rollout(int kind, int autoreset_mode, bool sample, int grid, hipStream_t stream, const mi_internal::DevEnv &d, const mi_internal::RolloutPtrs &p,
             const mi_internal::ActionStream &as, int T, int obs_dim, int in_f64, const mi_internal::RolloutExtra &ex);
}  // namespace mi_mjmodel
// The same over the mjx::MassLaneModel env types (mjx_mass_model.hip): what an env runs while it holds a body mass scale (mi_set_model_field
// MI_MODEL_BODY_MASS_SCALE with values; NULL takes it back to the kernels above).  A model type and a unit of their own, so that the kernels above stay
// without the mass rows.
namespace mi_mjmass {
bool step(int kind, int autoreset_mode, int grid, hipStream_t stream, const mi_internal::DevEnv &d, const void *mj_step_ptrs);
bool step_wrapped(int kind, int autoreset_mode, int trip, int grid, hipStream_t stream, const mi_internal::DevEnv &d, const void *mj_step_ptrs,
                  const mi_internal::MjWrapDev &w);
bool preload(int kind);  // (the constants kernel included)
bool rollout(int kind, int autoreset_mode, bool sample, int grid, hipStream_t stream, const mi_internal::DevEnv &d, const mi_internal::RolloutPtrs &p,
             const mi_internal::ActionStream &as, int T, int obs_dim, int in_f64, const mi_internal::RolloutExtra &ex);
// mj_reset_kernel over the same env types: the Humanoids' reset observation and tracked point read the sub-environment's body masses
bool reset(int kind, int grid, hipStream_t stream, const mi_internal::DevEnv &d, const uint8_t *mask, double *obs, int obs_dim);
// mj_model_constants_kernel: dof_invweight0, body_invweight0 and meaninertia of every sub-environment from the body mass scale rows of `rows`
// (the env's [mjx::MassLaneFields::WIDTH][N] block), written into the derived rows of the same block
bool derive_constants(int kind, int grid, hipStream_t stream, double *rows, int N);
}  // namespace mi_mjmass
namespace {
// argument of mj_step_kernel (mj_glue_kernels.h); crosses to mi_mjmodel::step as a const void *
struct MjStepPtrs {
    const void *actions;  // [N][NU] float32 rows, or float64 rows taken un-rounded (act_f64; mujoco_env.py:148 data.ctrl[:] = ctrl)
    double *obs, *reward;
    uint8_t *terminated, *truncated;
    double *final_obs, *ep_ret;
    int32_t *ep_len;
    double *info, *final_info;
    int obs_dim;
    const double *extras;  // [N][EX_TOTAL] rows written by mj_physics_kernel, or nullptr (one-lane simulator inside the step kernel)
    int act_f64;
};
}  // namespace
// shared with the other translation units of the library (hidden visibility): sets mi_last_error(), returns `code`
namespace mi_internal {
int set_error(int code, const char *msg);
}  // namespace mi_internal
namespace {

int fail(int code, const char *fmt, const char *detail = "") {
    char msg[512];
    snprintf(msg, sizeof msg, fmt, detail);
    return mi_internal::set_error(code, msg);
}

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) {                                                                           \
            char msg_[512];                                                                               \
            snprintf(msg_, sizeof msg_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return mi_internal::set_error((int)MI_ERR_HIP, msg_);                                          \
        }                                                                                                 \
    } while (0)

constexpr int kClassicKinds = 5;

}  // namespace

struct mi_vecenv {
    mi_config cfg;
    mi_layout lay;
    int device;
    hipStream_t stream, own_stream;
    DevEnv d;
    int grid;
    bool seeded, was_reset, act_seeded;
    bool has_epi;           // mi_set_step_epilogue: the wrappers run as the output stage of step_kernel
    EpiDev epi;
    mi_step_epilogue epi_host;  // what the caller attached: the statistics handles swap their two buffer sets every step, so epi is rebuilt
    double *d_epi_partial;      // [grid][kEpiCols] column sums of the step workgroups
    Pcg64 act_rng;          // host copy of the action-space generator
    PcgJump *d_pow2;        // [64] device jump table for act_rng.inc
    PcgJump jump_n;
    // the action stream as per-lane states on the device (act_sample_kernel): act_lane_valid = they correspond to the stream's position;
    // act_on_device = they ARE the position (the host copy act_rng is stale until act_sync_host reads lane 0 back)
    uint64_t *d_act_lane;   // [2][N]
    bool act_lane_valid, act_on_device;
    void *d_act_stage;      // mi_action_sample(MI_HOST): where the kernel writes before the copy to the caller's array
    size_t act_stage_bytes;
    // Staging for the MI_HOST entry points (SURVEY 8(b) "Ownership"): every step output lives in ONE device block and ONE pinned host
    // block of the same layout -- [error word | obs | reward | terminated | truncated | info | episode_return | episode_length | final_obs |
    // final_info], 256-byte aligned sections -- so a host step is one H2D (actions), one launch and one D2H of the prefix in use.
    // d_obs ... d_final_info / h_* are views into the two blocks.
    char *d_out, *h_out, *h_out_dev;  // h_out_dev: the device address of the pinned block (zero-copy step of the classic kinds)
    int *h_err;                       // sticky device error word, page-locked host memory
    size_t out_bytes, off_end[9];  // end offset of each section in the order above (after the header)
    void *d_actions, *h_actions;
    void *d_obs, *d_final;
    double *d_reward, *d_epret;
    uint8_t *d_term, *d_trunc, *d_mask;
    int32_t *d_eplen;
    uint64_t *d_words;
    size_t act_bytes, act_bytes_max, obs_bytes;
    double *d_info, *d_final_info;
    size_t info_bytes;
    mi_step_io h_io;        // the pinned host arrays (mi_host_buffers)
    mi_step_io pending;     // user pointers of a step that was enqueued by mi_step_async and not waited for yet
    size_t pending_bytes;
    bool has_pending;
    void *tab_bufs[8];
    bool tab_loaded;
    int tab_start_state;  // the one state every episode starts in (its cumulative initial probability is >= 1), -1 when the start is drawn among several
    // MuJoCo family: cooperative physics kernel (default) or the one-lane simulator (MI355ENV_MJ_SERIAL=1, cross-check)
    bool mj_coop;
    int extras_dim;
    double *d_extras;       // [N][EX_TOTAL]
    float *d_act_scratch;   // [N][NU] actions of the current rollout step when the caller does not keep them
    void *d_obs_scratch;    // [N][obs_dim] observations of the current rollout step when the caller does not keep them
    // MI_CFG_SHARED_RNG (CartPoleVectorEnv's semantics): the one generator and the bookkeeping of its draw positions, all device memory
    bool shared_rng;
    SharedRng shared;
    PcgJump *d_shared_pow2;
    Pcg64 shared_base;      // host copy of the base generator (mi_get_rng: base advanced by the device's `consumed` counter)
    // mi_set_env_attr: [A][N] float64 rows of the per-sub-environment attributes (allocated by the first call) and the set of attributes that
    // come from them.  attr_mask != 0 ("per-lane mode"): step and rollout run the *AttrT kernels (envs_classic.h); a bit, once set, stays set
    double *d_attr;
    uint32_t attr_mask;
    // mi_set_model_field (MuJoCo kinds): [MassLaneFields::WIDTH][N] float64 rows of gravity, actuator_gear, dof_damping, pair_friction, the body mass scale and the
    // constants derived from it (dof_invweight0, body_invweight0, meaninertia: the compiled-in values until a scale is set) -- allocated by the first
    // call, all fields at once, holding the compiled-in values -- and the set of fields a call has written (mi_get_model_field answers for the others without a copy).  d_model != NULL: step and rollout run the
    // one-lane kernels over the mjx::LaneModel env types (mjx_model.hip) for good; mj_coop is cleared with it.
    double *d_model;
    uint32_t model_mask;
    // mi_set_step_wrappers: RepeatAction / StickyAction of the sub-environments inside the step.  wrap_on: the *_wrapped_kernel entry points run, with
    // `wrap` as their last argument (its two arrays are allocated by the first call that switches StickyAction on).  per_lane: some call has switched
    // them on -- from then on the env stays on the per-lane types (envs_classic.h *AttrT) and their one-role kernels, as after mi_set_env_attr.
    // mi_set_max_and_skip: wrap.skip / wrap.frames (allocated by the first call that switches it on); wrap_on covers it too.
    WrapSkipDev wrap;
    bool wrap_on, per_lane;
    int wrap_act_kind;  // StickyAction: the element type of the action rows it has seen (last_action is kept in that type); -1: none yet
    // ... of a MuJoCo env (MjWrapDev; wrap.last_action is then [N][NU] at 8 bytes per component): the reward accumulator and the inner-step word of every row
    double *d_wrap_acc;
    uint32_t *d_wrap_inner;
    // sample(mask=...) / sample(probability=...) on the action stream (action_mask.hip): the pending 32-bit half and the words of the batch in flight,
    // the per-workgroup counts, the per-row slots; d_arg_stage: where a host caller's masks / probabilities are staged (MI_HOST only)
    mi_actmask::Ctl *d_act_ctl;
    uint32_t *d_act_partial, *d_act_slot;
    void *d_arg_stage;
    size_t arg_stage_bytes;
    bool masked_force_repair;  // MI355ENV_MASKED_FORCE_REPAIR=1 at mi_create
};

namespace {
bool is_mj(int kind) { return (kind >= kClassicKinds && kind <= MI_ENV_HUMANOID) || (kind >= MI_ENV_HOPPER && kind <= MI_ENV_INVERTED_DOUBLE_PENDULUM) || kind == MI_ENV_REACHER || kind == MI_ENV_HUMANOID_STANDUP || kind == MI_ENV_SWIMMER || kind == MI_ENV_PUSHER; }
bool is_tab(int kind) { return kind == MI_ENV_TABULAR || kind == MI_ENV_BLACKJACK; }  // Blackjack rides on the tabular kernels
}  // namespace
#endif  // MI355ENV_ENGINE_TYPES_H
