/*
 * mi355env.h -- C ABI of libmi355env.so, the MI355X (gfx950) lockstep vector-environment engine.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json: one call steps / resets all
 * `num_envs` sub-environments of a gymnasium.vector.VectorEnv on the GPU.  Plain pointers and sizes only;
 * no torch / numpy types.  Every entry point states the reference interface it replaces (paths relative
 * to the reference tree, gymnasium v1.4.0).
 *
 * Threading contract (same as the reference's SyncVectorEnv, which is single-threaded and not re-entrant):
 * one mi_vecenv may be used from one host thread at a time.  All work is enqueued on the env's HIP stream
 * (mi_set_stream); calls taking MI_HOST pointers synchronise that stream before returning, calls taking
 * MI_DEVICE pointers only enqueue.
 *
 * Errors: every function returns MI_OK (0) or a negative mi_status; mi_last_error() gives the message of
 * the last failure on the calling thread (the Python shim raises it as an exception, mirroring the
 * reference's AssertionError / ValueError / gymnasium.error.Error behaviour one level up).
 */
#ifndef MI355ENV_H
#define MI355ENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Entry points that were only ADDED since (mi_action_sample_masked and its three companions, mi_set_step_wrappers, mi_set_max_and_skip, mi_lookahead, mi_lookahead_policy) leave the number where it is: nothing an ABI 10
 * caller uses changed, and a caller that needs them finds out by looking the symbol up. */
#define MI355ENV_ABI_VERSION 10

typedef enum mi_status {
    MI_OK = 0,
    MI_ERR_INVALID_ARGUMENT = -1,
    MI_ERR_NO_DEVICE = -2,     /* no HIP device visible: the engine has NO CPU fallback */
    MI_ERR_HIP = -3,           /* a HIP runtime call failed; see mi_last_error() */
    MI_ERR_UNSUPPORTED = -4,
    MI_ERR_STATE = -5          /* e.g. step before reset/seed */
} mi_status;

/* Sub-environment dynamics.  Each value replaces the scalar env class named beside it. */
typedef enum mi_env_kind {
    MI_ENV_CARTPOLE = 0,               /* envs/classic_control/cartpole.py:119-247 (CartPole-v1)                */
    MI_ENV_PENDULUM = 1,               /* envs/classic_control/pendulum.py:102-171 (Pendulum-v1)                */
    MI_ENV_ACROBOT = 2,                /* envs/classic_control/acrobot.py:172-279,375-461 (Acrobot-v1)          */
    MI_ENV_MOUNTAIN_CAR = 3,           /* envs/classic_control/mountain_car.py:108-170 (MountainCar-v0)         */
    MI_ENV_MOUNTAIN_CAR_CONTINUOUS = 4, /* envs/classic_control/continuous_mountain_car.py:116-194              */
    /* MuJoCo family: the env class + MujocoEnv (envs/mujoco/mujoco_env.py:35-229) + the `mujoco` physics it calls  */
    MI_ENV_HALF_CHEETAH = 5,           /* envs/mujoco/half_cheetah_v5.py:153-281 + assets/half_cheetah.xml     */
    MI_ENV_ANT = 6,                    /* envs/mujoco/ant_v5.py:228-428 + assets/ant.xml                       */
    MI_ENV_HUMANOID = 7,               /* envs/mujoco/humanoid_v5.py:307-541 + assets/humanoid.xml             */
    /* ToyText: any finite MDP given as a transition table (mi_tabular_load); FrozenLake / CliffWalking / Taxi:
     * envs/toy_text/frozen_lake.py:324-348, cliffwalking.py:195-215, taxi.py:419-472, utils.py:4-8               */
    MI_ENV_TABULAR = 8,
    /* more of the MuJoCo family: same physics core, their own reward / observation glue */
    MI_ENV_HOPPER = 9,                     /* envs/mujoco/hopper_v5.py:146-343 + assets/hopper.xml                        */
    MI_ENV_WALKER2D = 10,                  /* envs/mujoco/walker2d_v5.py:151-345 + assets/walker2d_v5.xml                 */
    MI_ENV_INVERTED_PENDULUM = 11,         /* envs/mujoco/inverted_pendulum_v5.py:100-199 + assets/inverted_pendulum.xml  */
    MI_ENV_INVERTED_DOUBLE_PENDULUM = 12,  /* envs/mujoco/inverted_double_pendulum_v5.py:125-246 + its asset              */
    /* ToyText Blackjack-v1: envs/toy_text/blackjack.py:17-232 (Generator.choice card draws, dealer play-out, natural / sab rules);
     * observation row = int64[3] (player sum, dealer's showing card, usable ace); params[0] = natural, params[1] = sab */
    MI_ENV_BLACKJACK = 13,
    MI_ENV_REACHER = 14,                   /* envs/mujoco/reacher_v5.py:127-245 + assets/reacher.xml; params[0] = reward_dist_weight,
                                            * [1] = reward_control_weight, [4] = frame_skip                                  */
    MI_ENV_HUMANOID_STANDUP = 15,          /* envs/mujoco/humanoidstandup_v5.py:266-486 + assets/humanoidstandup.xml; params as HUMANOID with
                                            * [0] uph_cost_weight (unused by the reference) [5] impact_cost_weight [10],[11] impact_cost_range */
    MI_ENV_SWIMMER = 16,                   /* envs/mujoco/swimmer_v5.py:153-301 + assets/swimmer.xml (fluid forces of the medium: option density,
                                            * viscosity); params [0] forward_reward_weight [1] ctrl_cost_weight [2] reset_noise_scale
                                            * [3] exclude_current_positions [4] frame_skip                                     */
    MI_ENV_PUSHER = 17,                    /* envs/mujoco/pusher_v5.py:165-326 + assets/pusher_v5.xml; params [0] reward_near_weight [1] reward_control_weight
                                            * [4] frame_skip [5] reward_dist_weight                                            */
    MI_ENV_KIND_COUNT = 18
} mi_env_kind;

/* vector/vector_env.py:34-39 AutoresetMode; semantics of vector/sync_vector_env.py:277-319. */
typedef enum mi_autoreset_mode {
    MI_AUTORESET_NEXT_STEP = 0,
    MI_AUTORESET_SAME_STEP = 1,
    MI_AUTORESET_DISABLED = 2
} mi_autoreset_mode;

typedef enum mi_mem_location { MI_HOST = 0, MI_DEVICE = 1 } mi_mem_location;

/* Element types of the action / observation rows (mi_layout). */
typedef enum mi_dtype {
    MI_F32 = 0,
    MI_F64 = 1,
    MI_I64 = 2,
    /* action rows only (mi_step_io.actions_dtype): float64 values that were PYTHON floats on the caller's side -- the rows of a list-of-lists
     * batch, which sync_vector_env.py:274 iterate() hands to the scalar env as Python lists.  Python scalars are weak under NumPy 2's
     * promotion (NEP 50): np.float32 + float stays float32 where np.float32 + np.float64 becomes float64.  Only
     * MountainCarContinuous tells the two apart (continuous_mountain_car.py:153-155, its np.float32 state); every other kind treats the
     * value as MI_F64. */
    MI_F64_WEAK = 3,
    /* targets of mi_transform_observations(MI_OBS_CAST) only: no engine buffer holds them */
    MI_F16 = 4,
    MI_I32 = 5,
    MI_U8 = 6
} mi_dtype;

/*
 * Construction parameters = the kwargs the reference passes to the scalar env constructor through
 * make_vec(**kwargs) (envs/registration.py:957-963) plus the TimeLimit and vectoriser settings.
 *   params[] per kind:
 *     CARTPOLE                 params[0] = sutton_barto_reward (0/1)          cartpole.py:119-121
 *     PENDULUM                 params[0] = g (default 10.0)                   pendulum.py:102
 *     MOUNTAIN_CAR(_CONTINUOUS) params[0] = goal_velocity (default 0)         mountain_car.py:108
 *     HALF_CHEETAH / ANT / HUMANOID (constructor kwargs of half_cheetah_v5.py:153-164, ant_v5.py:228-245,
 *     humanoid_v5.py:307-326; all three share slots 0-4, the last two share 5-11):
 *       [0] forward_reward_weight  [1] ctrl_cost_weight  [2] reset_noise_scale
 *       [3] exclude_current_positions_from_observation (0/1)  [4] frame_skip
 *       [5] contact_cost_weight  [6] healthy_reward  [7] terminate_when_unhealthy (0/1)  [8],[9] healthy_z_range
 *       [10],[11] ANT: contact_force_range / HUMANOID: contact_cost_range
 *     HOPPER / WALKER2D (hopper_v5.py:146-160, walker2d_v5.py:172-185): slots 0-4 and 6-9 as above,
 *       [10],[11] healthy_angle_range  [12],[13] HOPPER: healthy_state_range
 *     INVERTED_PENDULUM / INVERTED_DOUBLE_PENDULUM: [2] reset_noise_scale [4] frame_skip [6] healthy_reward (double pendulum)
 *       [12] ANT: include_cfrc_ext_in_observation / HUMANOID: include_cinert_in_observation
 *       [13],[14],[15] HUMANOID: include_cvel / include_qfrc_actuator / include_cfrc_ext _in_observation
 *     TABULAR                  params[0] = number of states, params[1] = number of actions (table: mi_tabular_load);
 *                              params[2] != 0: Taxi's fickle passenger (envs/toy_text/taxi.py:436-451,462-464) with probability params[3] -- reset
 *                              draws fickle_step, the first move with the passenger aboard re-draws the destination (Generator.choice);
 *                              layout.state_dim is then 3 (state, prob, fickle_step | buffered 32-bit half << 1)
 */
typedef struct mi_config {
    int32_t struct_size;         /* = sizeof(mi_config) */
    int32_t kind;                /* mi_env_kind */
    int32_t num_envs;            /* N >= 1 (sub-environments owned by THIS device / rank) */
    int32_t max_episode_steps;   /* TimeLimit (wrappers/common.py:116-150); <= 0 disables truncation */
    int32_t autoreset_mode;      /* mi_autoreset_mode */
    int32_t reserved[3];         /* reserved[0]: option bits (MI_CFG_*), the others 0 */
    double params[16];
} mi_config;
/* mi_config.reserved[0] bits.  MI_CFG_SOLVER_NEWTON: the MuJoCo kinds whose MJCF asks for `solver="PGS" iterations="50"` (HUMANOID,
 * HUMANOID_STANDUP: assets/humanoid.xml:8) run that solver by default; this bit selects the converged primal Newton solver instead (the
 * same convex problem solved to 1e-10 -- a deliberate, faster deviation from the reference, opt-in only). */
#define MI_CFG_SOLVER_NEWTON 1
/* MI_CFG_FAST_MATH: the classic-control kinds (CARTPOLE .. MOUNTAIN_CAR_CONTINUOUS) reproduce the reference's libm by default -- sin / cos /
 * pow(x, 2) / powf(x, 2) bit for bit, so whole trajectories are array_equal to SyncVectorEnv's (classic_control/cartpole.py:180-181,
 * pendulum.py:131, acrobot.py:263-283).  This bit selects the device's own sin / cos (<= 1 ulp away) and x * x instead: ~1.2-2x the
 * env-steps/s, results within the tolerances of tests/test_gpu_parity.py's fast-math cases.  Opt-in only. */
#define MI_CFG_FAST_MATH 2
/* MI_CFG_SHARED_RNG (MI_ENV_CARTPOLE only): the semantics of the reference's own NumPy vector environment `CartPoleVectorEnv`
 * (envs/classic_control/cartpole.py:353-505; what `make_vec("CartPole-v1")` returns by default: it is the id's vector_entry_point) instead of
 * SyncVectorEnv's.  The dynamics are the same expressions; what differs:
 *   - ONE generator for all sub-environments.  reset() draws `uniform(low, high, size=(4, N))` -- component-major: draw c * N + i is component c
 *     of sub-environment i (cartpole.py:493-500); a step re-draws the k sub-environments that finished in the previous step with
 *     `uniform(low, high, size=(4, k))` in index order (draw c * k + j for the j-th of them, :475-478).  mi_seed reads ONE generator (pcg[0..3]),
 *     mi_seed_sequence seeds it with SeedSequence(base_seed) (first_index must be 0), mi_get_rng reports it in every row.
 *   - reset bounds given to mi_reset PERSIST for the autoresets that follow (self.low / self.high, :489-491); mi_reset takes no mask.
 *   - NEXT_STEP autoreset only; with sutton_barto_reward a sub-environment that did not terminate is rewarded -0.0 (`-np.array(terminated)`, :466).
 *   The reference returns float32 rewards there (:466-468): the values (+-1, +-0) are exact in either type; mi_step_io.reward stays float64 and the host
 *   class casts.  Sub-environments do not shard across devices in this mode (draw positions depend on every other sub-environment's episode ends). */
#define MI_CFG_SHARED_RNG 4

typedef struct mi_layout {
    int32_t obs_dim;      /* observation row length (elements) */
    int32_t obs_dtype;    /* mi_dtype */
    int32_t act_dim;      /* action row length; discrete envs: 1 element of MI_I64 per env */
    int32_t act_dtype;    /* mi_dtype */
    int32_t state_dim;    /* physics state row length for mi_get_state/mi_set_state (float64) */
    int32_t info_dim;     /* per-env info row length (float64), 0 for classic control; MuJoCo columns:
                             HALF_CHEETAH: x_position, x_velocity, reward_forward, reward_ctrl   (half_cheetah_v5.py:230,241-246)
                             ANT / HUMANOID: x_position, y_position, distance_from_origin, x_velocity, y_velocity,
                                             reward_forward, reward_ctrl, reward_contact, reward_survive (ant_v5.py:359-366,384-389)
                             HUMANOID / HUMANOID_STANDUP append tendon_length[2], tendon_velocity[2] (humanoid_v5.py:486-487) */
    int32_t reserved[2];
} mi_layout;

/*
 * Buffers of one step() call, all row-major [num_envs][dim].  Pointers are all host or all device
 * (mi_mem_location).  Nullable members are skipped.
 *   actions          in   [N][act_dim] act_dtype     (i64 for Discrete -- what iterate(MultiDiscrete) yields); Box kinds: float32
 *                                               rows (layout.act_dtype, the dtype of the space and of its sampler) or, with
 *                                               actions_dtype = MI_F64, float64 rows taken UN-ROUNDED.
 *                                               NULL (ABI 7, loc == MI_DEVICE): the ON-DEVICE POLICY -- the step kernel itself draws
 *                                               `action_space.sample()` from the action stream (mi_action_seed), i.e. the call is
 *                                               `step(action_space.sample())` (utils/performance.py:82-97, the metric's own loop) in one
 *                                               launch with no host-to-device traffic; the stream advances by N * act_dim draws
 *   actions_out      out  [N][act_dim] act_dtype     with actions == NULL: the actions that were drawn (NULL to skip)
 *   obs              out  [N][obs_dim] obs_dtype
 *   reward           out  [N] f64                     (sync_vector_env.py:171)
 *   terminated       out  [N] u8 0/1                  (np.bool_ compatible)
 *   truncated        out  [N] u8 0/1
 *   final_obs        out  [N][obs_dim]  SAME_STEP only: rows of envs that finished this step (others untouched)
 *   episode_return   out  [N] f64      vector RecordEpisodeStatistics "r" (wrappers/vector/common.py:156-235):
 *   episode_length   out  [N] i32      "l"; both 0 where the env did not finish an episode this step
 *   info             out  [N][info_dim] f64   the numeric entries of the scalar env's info dict (layout.info_dim columns);
 *                                               rows of sub-envs that RESET in this call (NEXT_STEP autoreset step, SAME_STEP after a
 *                                               finished episode) hold the scalar env's reset info instead (_get_reset_info)
 *   final_info       out  [N][info_dim] f64   SAME_STEP only: the info of the step that finished the episode, for the rows of
 *                                               envs that finished this step (sync_vector_env.py:309-317 "final_info"; others untouched)
 */
typedef struct mi_step_io {
    const void *actions;
    void *obs;
    double *reward;
    uint8_t *terminated;
    uint8_t *truncated;
    void *final_obs;
    double *episode_return;
    int32_t *episode_length;
    double *info;
    double *final_info;
    /* Element type of `actions` for the Box kinds: MI_F32 (0, the default: layout.act_dtype), MI_F64 or MI_F64_WEAK.  The reference hands the caller's rows
     * to the scalar env as they are (vector/sync_vector_env.py:274 iterate(); envs/classic_control/pendulum.py:127-134 np.clip(u)[0],
     * continuous_mountain_car.py:153 action[0], envs/mujoco/mujoco_env.py:148 data.ctrl[:] = ctrl), so a float64 action array is NOT
     * rounded to float32 on the way in, and NumPy's promotion rules then make parts of the step float64 arithmetic that are float32 for a
     * float32 row (the control cost of the MuJoCo kinds, Pendulum's torque terms, MountainCarContinuous' velocity update).  MI_F64
     * reproduces that; the pinned action array of mi_host_buffers is sized for either type.  Ignored by the Discrete kinds (MI_I64). */
    int32_t actions_dtype;
    int32_t reserved;
    void *actions_out; /* ABI 7: see above (only read when actions == NULL) */
} mi_step_io;

/* Buffers of one fused rollout() call: T consecutive step()s in one launch, time-major [T][N][dim].
 * Any output pointer may be NULL (not materialised).  Device pointers only. */
typedef struct mi_rollout_io {
    const void *actions_in;   /* [T][N][act_dim] or NULL => sample on device from the action stream; element type: actions_in_dtype */
    void *actions_out;        /* [T][N][act_dim] the sampled actions (NULL to skip)                    */
    void *obs;                /* [T][N][obs_dim] */
    double *reward;           /* [T][N] */
    uint8_t *terminated;      /* [T][N] */
    uint8_t *truncated;       /* [T][N] */
    int32_t actions_in_dtype; /* Box kinds: MI_F32 (0, default) or MI_F64 rows in actions_in (see mi_step_io.actions_dtype); actions_out is always layout.act_dtype */
    int32_t reserved;
} mi_rollout_io;

/* What step() returns besides obs / reward / flags, for every step of a fused rollout (ABI 10, mi_rollout_infos): device pointers, time-major,
 * each nullable.  Row [t] of an array holds what mi_step_io's member of the same name holds after the t-th of T consecutive mi_step calls:
 *   episode_return / episode_length   0 where the sub-environment did not finish an episode at step t
 *   info                              the scalar env's info; its RESET info in rows that reset at step t (the NEXT_STEP autoreset step, a
 *                                     finished row under SAME_STEP)
 *   final_obs / final_info            SAME_STEP only: the last observation / info of the episode, in rows that finished at step t
 * ONE deliberate difference from mi_step, which leaves the final_obs / final_info rows of sub-environments that finished nothing untouched:
 * here those rows are written as ZEROS, so every element of every requested array is defined after the call and the caller needs no memset
 * pass.  The mask of the rows that carry a value is terminated | truncated of the same step (mi_rollout_io). */
typedef struct mi_rollout_extra {
    void *final_obs;          /* [T][N][obs_dim] obs_dtype */
    double *episode_return;   /* [T][N] */
    int32_t *episode_length;  /* [T][N] */
    double *info;             /* [T][N][info_dim]; NULL when layout.info_dim == 0 */
    double *final_info;       /* [T][N][info_dim]; NULL when layout.info_dim == 0 */
} mi_rollout_extra;

/* Running totals kept on device (the multi-GPU metric all-reduce operates on these three numbers). */
typedef struct mi_stats {
    uint64_t env_steps;       /* sub-env steps that advanced dynamics (utils/performance.py:88-90 counting) */
    uint64_t reset_steps;     /* NEXT_STEP autoreset steps (not counted as env steps)                       */
    uint64_t episodes;        /* finished episodes                                                          */
    double return_sum;        /* sum of finished-episode returns                                            */
    uint64_t length_sum;      /* sum of finished-episode lengths                                            */
} mi_stats;

typedef struct mi_vecenv mi_vecenv;

/* Library / device ----------------------------------------------------------------------------------- */
int mi_abi_version(void);
const char *mi_last_error(void);
/* Number of visible HIP devices (0 on a CPU-only host; never an error). */
int mi_device_count(void);

/* Lifetime.  Replaces SyncVectorEnv.__init__ (vector/sync_vector_env.py:76-185) / the vector_entry_point
 * creator call (envs/registration.py:963).  Fails with MI_ERR_NO_DEVICE when no GPU is present. */
int mi_create(const mi_config *cfg, int device, mi_vecenv **out);
/* Replaces VectorEnv.close_extras (vector/vector_env.py:238-240). */
void mi_destroy(mi_vecenv *env);
int mi_get_layout(const mi_vecenv *env, mi_layout *out);
/* Use an existing hipStream_t (e.g. torch's current stream) for all subsequent work.  NULL means the legacy
 * default stream (what torch.cuda.current_stream().cuda_stream is by default).  Until this is called the env
 * uses the engine's non-blocking stream of its device (one per device and process, shared by all envs).
 * Stream capture: mi_step with loc == MI_DEVICE (without a step epilogue) only launches kernels on this stream -- no synchronising HIP call,
 * no host-side state that changes from step to step -- so a caller may put the stream into capture (hipStreamBeginCapture) and record any
 * number of steps into a hipGraph (gymnasium_amd.HipVectorEnv.capture_steps does; tests/test_gpu_graph_capture.py).  The host-side checks of
 * mi_step (the sticky device error word) are made at capture time only: after replays, mi_synchronize / the next eager call raises it. */
int mi_set_stream(mi_vecenv *env, void *hip_stream);
int mi_synchronize(mi_vecenv *env);

/* Seeding.  Replaces Env.reset(seed=...) -> seeding.np_random (core.py:157-159, utils/seeding.py:10-42)
 * with the SyncVectorEnv fan-out seed+i (vector/sync_vector_env.py:207-208).
 *   mi_seed:          pcg[N][4] = {state_hi, state_lo, inc_hi, inc_lo} of each env's PCG64 (host pointer);
 *                     mask (host, nullable) selects which envs are re-seeded.
 *   mi_seed_sequence: env i <- PCG64(SeedSequence(base_seed + first_index + i)) computed on device. */
int mi_seed(mi_vecenv *env, const uint64_t *pcg, const uint8_t *mask);
int mi_seed_sequence(mi_vecenv *env, uint64_t base_seed, uint64_t first_index, const uint8_t *mask);

/* Replaces SyncVectorEnv.reset (vector/sync_vector_env.py:187-264) incl. options["reset_mask"] (:214-246)
 * and the classic-control reset options (envs/classic_control/utils.py:17-46; pendulum.py:151-162):
 *   bounds (host, nullable) = {low, high}  (Pendulum: {x_init, y_init}).
 * mask/obs are host or device pointers per `loc`; rows with mask==0 are not written. */
int mi_reset(mi_vecenv *env, const uint8_t *mask, const double *bounds, void *obs, int loc);

/* Replaces SyncVectorEnv.step (vector/sync_vector_env.py:266-337) with TimeLimit (wrappers/common.py:129-133)
 * and the scalar env's step() folded into one kernel launch. */
int mi_step(mi_vecenv *env, const mi_step_io *io, int loc);

/*
 * Asynchronous host stepping (SURVEY.md 8(b) "Threading"): replaces AsyncVectorEnv.step_async / step_wait
 * (vector/async_vector_env.py:440-521).  mi_step_async enqueues actions H2D -> step kernel -> ONE D2H of the output block and returns
 * without synchronising; mi_step_wait synchronises, reports errors and fills the arrays given to mi_step_async (host pointers).  One step
 * may be pending per env.  mi_step(io, MI_HOST) is exactly mi_step_async + mi_step_wait.
 *
 * mi_host_buffers: the env's own PINNED host arrays, laid out like the device output block (actions, obs, reward, terminated,
 * truncated, info, episode_return, episode_length, final_obs, final_info; valid until mi_destroy).  Passing these pointers to
 * mi_step / mi_step_async makes the host path zero-copy: the D2H lands where the caller reads, the actions are uploaded from where the
 * caller wrote them (SURVEY.md 8(b) "Ownership").
 */
int mi_step_async(mi_vecenv *env, const mi_step_io *io);
int mi_step_wait(mi_vecenv *env);
int mi_host_buffers(mi_vecenv *env, mi_step_io *out);

/* Transition table of a MI_ENV_TABULAR environment (host pointers, copied to the device).  Replaces the `P` dict and
 * `initial_state_distrib` the toy-text constructors build (frozen_lake.py:255-303, cliffwalking.py:118-135, taxi.py:281-334):
 *   csprob[nS][nA][K]   np.cumsum of the outcome probabilities (what categorical_sample compares against, utils.py:4-8)
 *   prob / next_state / reward / terminated [nS][nA][K]   the outcome tuples; count[nS][nA] outcomes are valid
 *   isd_csprob[nS]      np.cumsum(initial_state_distrib)
 * step: i = argmax(csprob[s][a] > rng.random()); reset: s = argmax(isd_csprob > rng.random()).  Observations are int64
 * states; layout.info_dim = 1 (the "prob" entry of the info dict).
 * num_tables > 1 (ABI 6): every array above gains a leading [num_tables] axis and env_table[N] names each sub-environment's table -- SyncVectorEnv over
 * scalar envs that were constructed differently, e.g. FrozenLake with map_name=None, where every sub-environment draws its own random map
 * (frozen_lake.py:241-242).  All tables share num_states / num_actions / max_outcomes.  num_tables 0 or 1 with env_table NULL: one table for all. */
typedef struct mi_tabular_table {
    int32_t num_states, num_actions, max_outcomes, num_tables;
    const double *csprob, *prob;
    const int32_t *next_state;
    const double *reward;
    const uint8_t *terminated;
    const int32_t *count;
    const double *isd_csprob;
    const int32_t *env_table; /* [N] host pointer: table index of each sub-environment, or NULL */
} mi_tabular_table;
int mi_tabular_load(mi_vecenv *env, const mi_tabular_table *table);

/* Random policy on device: the action space's generator (spaces/space.py:112-122 Space.seed), given as the
 * PCG64 {state_hi,state_lo,inc_hi,inc_lo}.  rollout then reproduces
 *   for t in range(T): step(action_space.sample())   (spaces/multi_discrete.py:176-178, spaces/box.py:463-465)
 * bit-for-bit in a single launch. */
int mi_action_seed(mi_vecenv *env, const uint64_t pcg[4]);
int mi_rollout(mi_vecenv *env, int T, const mi_rollout_io *io);
/* mi_rollout that also stores the arrays of `extra` (ABI 10).  extra == NULL, or all its members NULL, IS mi_rollout(env, T, io): the same
 * dispatch and the same kernels.  With a member set, the classic-control kinds run the one-role rollout kernel's variant that stores them
 * (never the two-role kernel), ToyText the general tabular kernel (never the branch-free ones), the MuJoCo kinds their rollout path.
 * final_obs / final_info under NEXT_STEP, and info / final_info for a kind without info columns: MI_ERR_INVALID_ARGUMENT; DISABLED autoreset:
 * MI_ERR_UNSUPPORTED, like mi_rollout.  The action stream advances as in mi_rollout (one position, shared with mi_step(actions == NULL) and
 * mi_action_sample); nothing allocates and nothing synchronises. */
int mi_rollout_infos(mi_vecenv *env, int T, const mi_rollout_io *io, const mi_rollout_extra *extra);
/* The action stream as a sampler of its own (ABI 7).  All three keep ONE position: whatever draws mi_rollout / mi_step(actions == NULL) /
 * mi_action_sample consume, the next consumer continues where the last one stopped, exactly like successive `action_space.sample()` calls on
 * the reference's seeded space (spaces/space.py:112-122 seed(), spaces/multi_discrete.py:176-178, spaces/box.py:463-465 sample()).
 *   mi_action_sample: out[T][N][act_dim] (layout.act_dtype) <- the next T batches of `action_space.sample()`; loc == MI_DEVICE only enqueues
 *                     (a host class hands them out one batch per sample() call: T launches' worth of policy in one), MI_HOST synchronises.
 *                     T == 0 just prepares the per-lane stream states (before a stream capture: mi_step(actions == NULL) is capturable).
 *   mi_action_get:    the generator that would produce the NEXT draw, as {state_hi, state_lo, inc_hi, inc_lo} (synchronises when the position
 *                     lives on the device, i.e. after mi_step(actions == NULL) / mi_action_sample): hand it to np.random.PCG64 to continue on the host.
 *   mi_action_skip:   move the position by `draws` (negative: backwards -- a host class that sampled ahead returns what it did not hand out). */
int mi_action_sample(mi_vecenv *env, int T, void *out, int loc);
int mi_action_get(mi_vecenv *env, uint64_t pcg[4]);
int mi_action_skip(mi_vecenv *env, int64_t draws);
/* `action_space.sample(mask=...)` / `sample(probability=...)` of the batched Discrete space (added to ABI 10; spaces/multi_discrete.py:180-249 _apply_mask
 * over MultiDiscrete([A] * N): ONE generator, rows visited in index order).  Discrete kinds only (act_dim == 1, MI_I64: CARTPOLE, ACROBOT,
 * MOUNTAIN_CAR, TABULAR, BLACKJACK; others: MI_ERR_UNSUPPORTED); A = the number of actions.  Both continue the ONE action stream of
 * mi_action_sample / mi_step(actions == NULL) / mi_rollout and leave its position on the device with the per-lane states valid for it.
 *   mi_action_sample_masked:   mask[N][A] int8 of 0 / 1, A <= 64.  valid = the indices holding 1, k = their number: k == 0 -> action 0, k == 1 ->
 *                     valid[0], nothing drawn either way; k >= 2 -> valid[j], j = Generator.choice's bounded integer: Lemire's method on 32-BIT
 *                     values taken from PCG64's buffered half (the low half of a 64-bit output first, its high half kept for the next 32-bit
 *                     draw; 64-bit draws neither use nor clear a pending half).  A rejected draw (probability (2^32 mod k) / 2^32) takes one
 *                     value more.  The batch therefore consumes a data-dependent number of outputs and may leave a half pending.
 *   mi_action_sample_weighted: prob[N][A] float64, A <= 7 (np.sum is the plain left-to-right sum up to there).  valid = (p > 0) & (p <= 1);
 *                     cdf = cumsum(p[valid] / sum(p)); cdf /= cdf[-1]; action = valid[searchsorted(cdf, random(), side="right")]: one 64-bit
 *                     output per row, like the plain sampler.
 *   out[N] int64.  loc == MI_DEVICE only enqueues on the env's stream: no allocation, no synchronising call, no host-side state that changes
 *   from call to call; MI_HOST stages the rows and synchronises.
 *   Invalid rows -- a mask value other than 0 / 1; a probability outside [0, 1] or NaN; !np.isclose(sum(p), 1) (rtol 1e-5, atol 1e-8): the WHOLE
 *   batch is refused: `out` is not written, position and pending half stay where they were, and the sticky device error word is set --
 *   MI_HOST returns MI_ERR_INVALID_ARGUMENT at once, MI_DEVICE raises it at the next synchronising call (mi_synchronize, mi_get_stats, the next
 *   mi_step), the same way as an action outside the space.  A deliberate deviation from the reference, whose assertion fires at the first
 *   invalid row and leaves its generator mid-batch -- like the whole-batch refusal of MI_CFG_SHARED_RNG.
 *   MI355ENV_MASKED_FORCE_REPAIR=1 (read at mi_create; tests): every masked batch goes through the stage that otherwise only recomputes the rows
 *   behind a rejected draw.  Results are identical.
 *   mi_action_get_buffered / mi_action_set_buffered: the pending half as NumPy names it (bit_generator.state "has_uint32" / "uinteger").  get
 *   goes with mi_action_get and synchronises like it; set follows mi_action_seed, which clears the half. */
int mi_action_sample_masked(mi_vecenv *env, const int8_t *mask, void *out, int loc);
int mi_action_sample_weighted(mi_vecenv *env, const double *prob, void *out, int loc);
int mi_action_get_buffered(mi_vecenv *env, uint32_t *has_uint32, uint32_t *uinteger);
int mi_action_set_buffered(mi_vecenv *env, uint32_t has_uint32, uint32_t uinteger);

/* Bookkeeping ------------------------------------------------------------------------------------------ */
int mi_get_stats(mi_vecenv *env, mi_stats *out);     /* synchronises */
int mi_reset_stats(mi_vecenv *env);
/* Per-env flag bits of mi_get_state/mi_set_state. */
#define MI_FLAG_NEEDS_RESET 1u /* the env finished last step (SyncVectorEnv._autoreset_envs, sync_vector_env.py:329) */
#define MI_FLAG_STATE_F32 2u   /* MountainCarContinuous: state currently held as float32 (continuous_mountain_car.py:178) */
/* MuJoCo kinds: a state row is [qpos(nq), qvel(nv), qacc_warmstart(nv), tracked_x, tracked_y] -- the Cartesian position
 * the next step's velocity reward is differenced against comes from the last forward pass and lags qpos. */
/* Physics state rows [N][state_dim] float64 (host pointers); checkpoint/resume + teacher-forced tests.
 * Replaces poking env.unwrapped.state (tests/envs/test_env_implementation.py:255-321 compares it).
 * Domain of mi_set_state for the classic-control kinds: angles that go into sin / cos within |x| < 105414336 (the range in which the engine's
 * routines ARE glibc's; CartPole and Pendulum defer to the device library beyond it, Acrobot and MountainCar -- which wrap / clip their angle --
 * assume it).  The host classes refuse rows outside it (gymnasium_amd/envs/classic_control.py _STATE_LIMITS); a binding of its own should too. */
int mi_get_state(mi_vecenv *env, double *state, int32_t *elapsed_steps, uint8_t *flags);
int mi_set_state(mi_vecenv *env, const double *state, const int32_t *elapsed_steps, const uint8_t *flags);
/* Per-env PCG64 words, same layout as mi_seed (host pointer). */
int mi_get_rng(mi_vecenv *env, uint64_t *pcg);

/*
 * Per-sub-environment physics (ABI 8): SyncVectorEnv.set_attr / get_attr (vector/sync_vector_env.py:365-398) on the attributes the scalar env's
 * step() reads, for the five classic-control kinds (not with MI_CFG_SHARED_RNG or MI_CFG_FAST_MATH).
 * mi_set_env_attr: `values` = num_envs float64, one per sub-environment, host (on_device = 0, staged before the call returns) or device memory
 * (on_device = 1: a device-to-device copy enqueued on the env's stream); NULL restores the construction value.  Takes effect from the next
 * mi_step / mi_rollout; resets do not undo it and mi_get_state does not include it.  The first call switches the env to the per-lane kernels,
 * whose values live in device memory updated in place (a HIP graph captured after the switch sees later calls).
 * mi_get_env_attr: the current values into `host_out` (num_envs float64); synchronises.
 * The string kinematics_integrator is stored as 0 ("euler") / 1 (anything else: semi-implicit Euler, cartpole.py:185).
 * ACROBOT (acrobot.py:147-167): book_or_nips is stored as 0 ("book", and any other string) / 1 ("nips").  A sub-environment whose
 * torque_noise_max is > 0 takes one draw from its own generator (the one its resets consume) in every step, before the dynamics; a step that also
 * resets (SAME_STEP) draws for the step first.  LINK_LENGTH_2 and AVAIL_TORQUE are not attributes here.  Domain: the RK4 stage angles must stay
 * within the exact sin / cos range above, which holds for masses in [0, 2], LINK_LENGTH_1 and the COM positions in [0, 1.5], LINK_MOI in [0.5, 100],
 * MAX_VEL_1 in [0, 16], MAX_VEL_2 in [0, 32], dt in [0, 0.25], torque_noise_max <= 4 and state velocities within (16, 32): the host class refuses
 * anything else (gymnasium_amd/envs/classic_control.py ACROBOT_ATTR_RANGES, where the bound is worked out); a binding of its own should too.  An
 * angle that leaves that range before wrap() becomes NaN instead of being wrapped one turn at a time.
 */
enum {
    MI_ATTR_CARTPOLE_GRAVITY = 0, MI_ATTR_CARTPOLE_MASSCART = 1, MI_ATTR_CARTPOLE_MASSPOLE = 2, MI_ATTR_CARTPOLE_TOTAL_MASS = 3,
    MI_ATTR_CARTPOLE_LENGTH = 4, MI_ATTR_CARTPOLE_POLEMASS_LENGTH = 5, MI_ATTR_CARTPOLE_FORCE_MAG = 6, MI_ATTR_CARTPOLE_TAU = 7,
    MI_ATTR_CARTPOLE_KINEMATICS_INTEGRATOR = 8, MI_ATTR_CARTPOLE_THETA_THRESHOLD_RADIANS = 9, MI_ATTR_CARTPOLE_X_THRESHOLD = 10,
    MI_ATTR_CARTPOLE_COUNT = 11,
    MI_ATTR_PENDULUM_G = 0, MI_ATTR_PENDULUM_M = 1, MI_ATTR_PENDULUM_L = 2, MI_ATTR_PENDULUM_DT = 3, MI_ATTR_PENDULUM_MAX_SPEED = 4,
    MI_ATTR_PENDULUM_MAX_TORQUE = 5, MI_ATTR_PENDULUM_COUNT = 6,
    MI_ATTR_MOUNTAIN_CAR_FORCE = 0, MI_ATTR_MOUNTAIN_CAR_GRAVITY = 1, MI_ATTR_MOUNTAIN_CAR_MAX_SPEED = 2, MI_ATTR_MOUNTAIN_CAR_MIN_POSITION = 3,
    MI_ATTR_MOUNTAIN_CAR_MAX_POSITION = 4, MI_ATTR_MOUNTAIN_CAR_GOAL_POSITION = 5, MI_ATTR_MOUNTAIN_CAR_GOAL_VELOCITY = 6, MI_ATTR_MOUNTAIN_CAR_COUNT = 7,
    MI_ATTR_MOUNTAIN_CAR_CONTINUOUS_MIN_ACTION = 0, MI_ATTR_MOUNTAIN_CAR_CONTINUOUS_MAX_ACTION = 1, MI_ATTR_MOUNTAIN_CAR_CONTINUOUS_POWER = 2,
    MI_ATTR_MOUNTAIN_CAR_CONTINUOUS_MAX_SPEED = 3, MI_ATTR_MOUNTAIN_CAR_CONTINUOUS_MIN_POSITION = 4, MI_ATTR_MOUNTAIN_CAR_CONTINUOUS_MAX_POSITION = 5,
    MI_ATTR_MOUNTAIN_CAR_CONTINUOUS_GOAL_POSITION = 6, MI_ATTR_MOUNTAIN_CAR_CONTINUOUS_GOAL_VELOCITY = 7, MI_ATTR_MOUNTAIN_CAR_CONTINUOUS_COUNT = 8,
    MI_ATTR_ACROBOT_LINK_LENGTH_1 = 0, MI_ATTR_ACROBOT_LINK_MASS_1 = 1, MI_ATTR_ACROBOT_LINK_MASS_2 = 2, MI_ATTR_ACROBOT_LINK_COM_POS_1 = 3,
    MI_ATTR_ACROBOT_LINK_COM_POS_2 = 4, MI_ATTR_ACROBOT_LINK_MOI = 5, MI_ATTR_ACROBOT_MAX_VEL_1 = 6, MI_ATTR_ACROBOT_MAX_VEL_2 = 7,
    MI_ATTR_ACROBOT_DT = 8, MI_ATTR_ACROBOT_TORQUE_NOISE_MAX = 9, MI_ATTR_ACROBOT_BOOK_OR_NIPS = 10, MI_ATTR_ACROBOT_COUNT = 11
};
int mi_set_env_attr(mi_vecenv *env, int attr, const double *values, int on_device);
int mi_get_env_attr(mi_vecenv *env, int attr, double *host_out);

/*
 * Per-sub-environment model fields of the MuJoCo kinds (added to ABI 10, which it leaves as it is): this engine's spelling of writing
 * env.unwrapped.model.opt.gravity, .actuator_gear[:, 0], .dof_damping and the sliding friction of the compiled contact pairs (the element-wise
 * maximum of the two geoms' geom_friction[:, 0]) in every sub-environment of a SyncVectorEnv.  An extension: the reference's scalar envs have no
 * such attributes.  Like all MuJoCo physics here the parity with `mujoco` is UNPINNED (no `mujoco` build to take fixtures from); the CPU oracle,
 * which takes the same fields as data, is the reference for these fields.  No compiled-model quantity is derived from any of them.
 * mi_model_field_width: 3 / nu / nv / number of contact pairs (0 for a robot without any) / nbody; < 0: not a MuJoCo kind, or no such field.
 * mi_set_model_field: `values` = [num_envs][width] row-major float64, host (on_device = 0: checked and staged before the call returns) or device
 * memory (on_device = 1: transposed into the env's rows by a small kernel on the env's stream; the caller has checked the values); NULL restores
 * the compiled-in values.  Takes effect from the next mi_step / mi_rollout; resets do not undo it and mi_get_state does not include it.  The
 * first call allocates the rows of all fields at the compiled-in values and moves the env to the one-lane simulator for good (a robot whose
 * default is the cooperative kernel gets slower: docs/results_log.md; MI355ENV_MJ_COOP=1 does not bring it back); the values live in device
 * memory updated in place, so mi_step stays capturable and a HIP graph captured after the switch sees later calls.  That first call also loads
 * the per-lane kernels' code object (kernels otherwise load on first use, which a stream capture must not trigger): a capture may follow it at once.
 * Refused: a kind that is not a MuJoCo one (MI_ERR_UNSUPPORTED); a non-finite value, a negative damping, a friction below 1e-5 -- MuJoCo's
 * documented minimum (MI_ERR_INVALID_ARGUMENT).
 * mi_get_model_field: the current values into `host_out` ([num_envs][width] float64); synchronises.
 *
 * MI_MODEL_BODY_MASS_SCALE (added to ABI 10 as well; width nbody, the world body's column is accepted and has no effect): body b of a
 * sub-environment has `scale` times the compiled mass AND inertia tensor -- the same link at another density, so its centre of mass, principal
 * axes and fluid box stay.  Values must be finite and >= 1e-3 (a stated floor: the lightest compiled bodies stay above the simulator's 1e-15 mass
 * test and M stays positive definite).  Unlike the other four fields this one drags compiled constants with it: dof_invweight0, body_invweight0
 * and meaninertia (from M(qpos0) and its inverse).  The call derives them for every sub-environment on the device, one lane each, with the
 * mass-matrix code of the step kernels (mj_model_constants_kernel, on the env's stream, no host work per sub-environment); every use site of the
 * one-lane simulator reads the lane's values.  While a scale is held the env runs kernels of their own (mjx::MassLaneModel: the mass rows stay out of
 * the kernels of the other four fields, which they would slow down).  NULL restores the scale 1 and the compiled-in constants, copied, not derived, and
 * takes the env back to the kernels without the mass rows: an env that never sets this field runs on exactly what it ran before the field existed.
 * Because the first call with values and the call with NULL change which kernels mi_step launches, a HIP graph captured before either of them must be
 * captured again (it would go on launching the other kernels, which ignore, or keep, the scale); between the two, later calls with values are seen by a
 * captured graph like those of the other fields.
 * mi_get_model_derived: the derived constants of every sub-environment into `host_out` -- [num_envs][nv], [num_envs][nbody][2] or [num_envs][1]
 * float64; the compiled model's values until a scale is set; synchronises.
 */
enum { MI_MODEL_GRAVITY = 0, MI_MODEL_ACTUATOR_GEAR = 1, MI_MODEL_DOF_DAMPING = 2, MI_MODEL_PAIR_FRICTION = 3, MI_MODEL_BODY_MASS_SCALE = 4, MI_MODEL_FIELD_COUNT = 5 };
enum { MI_MODEL_DERIVED_DOF_INVWEIGHT0 = 0, MI_MODEL_DERIVED_BODY_INVWEIGHT0 = 1, MI_MODEL_DERIVED_MEANINERTIA = 2, MI_MODEL_DERIVED_COUNT = 3 };
int mi_model_field_width(mi_vecenv *env, int field);
int mi_set_model_field(mi_vecenv *env, int field, const double *values, int on_device);
int mi_get_model_field(mi_vecenv *env, int field, double *host_out);
int mi_get_model_derived(mi_vecenv *env, int which, double *host_out);

/*
 * The per-sub-environment action wrappers (added to ABI 10, which it leaves as it is): gymnasium.wrappers.RepeatAction and StickyAction
 * (wrappers/stateful_action.py:16-220) around every scalar env, outside its TimeLimit -- what
 * make_vec(id, n, "sync", wrappers=(lambda e: StickyAction(RepeatAction(e, k), p, d),)) builds -- for the five classic-control kinds (not with
 * MI_CFG_SHARED_RNG or MI_CFG_FAST_MATH, not with a step epilogue attached) and the eleven MuJoCo kinds (below).  They live below the vector level, so
 * the engine steps each lane differently; mi_step, mi_rollout and mi_rollout_infos all follow, for the classic kinds in one launch as before.
 *   num_repeats >= 1: RepeatAction(env, num_repeats).  A step runs up to num_repeats inner steps with the same action and stops after the first that
 *     terminates or truncates; reward = 0.0 + r_1 + r_2 ... in that order; obs (and final_obs under SAME_STEP) is the last inner step's; TimeLimit
 *     counts INNER steps.  The NEXT_STEP autoreset step repeats nothing.  episode_return / episode_length and mi_stats count what the vector level
 *     sees: one step per call (utils/performance.py:88-90) and the sum of the summed rewards.  0: no such wrapper.
 *   sticky_duration >= 1: StickyAction(env, sticky_probability, sticky_duration) OUTSIDE the RepeatAction: one decision per call.  A lane that has a
 *     last action and is not inside a series takes ONE float64 draw u from its own generator (the one its resets consume; mi_get_rng shows it
 *     moved) BEFORE the step and any draw of the step itself (ACROBOT's torque noise), and starts a series if u < sticky_probability; inside a
 *     series nothing is drawn.  The effective action -- the last one while a series lasts -- becomes the last action.  Every reset of a row (mi_reset
 *     with or without mask, the NEXT_STEP autoreset step, the SAME_STEP reset) clears its state, so the first step after a reset draws nothing.  A
 *     (low, high) duration range is not offered: Generator.integers takes PCG64's buffered 32-bit half, which these lanes do not carry.  0: no such
 *     wrapper (sticky_probability is then ignored; 0.0 with a duration still draws).
 *   (0, any, 0) switches both off; num_repeats 1 without StickyAction differs from that only in `0.0 + reward` (a reward of -0.0 becomes 0.0).
 * Every call (re)constructs the wrappers: the sticky state of all rows is cleared.  The first call that switches one on moves the env to the
 * per-lane kernels for good (as mi_set_env_attr does); the state lives in device memory, allocated by that call: mi_step stays capturable.
 * mi_get_state / mi_set_state do not carry it.  Actions are validated as given (stricter than the reference, which never sees an action that a
 * sticky one replaces); mi_rollout's actions_out are the policy's actions, not the effective ones.  With StickyAction on, the element type of the
 * action rows (mi_step_io.actions_dtype) must not change from call to call: MI_ERR_UNSUPPORTED.
 * The MuJoCo kinds (both kernel paths, MI_CFG_SOLVER_NEWTON, float32 and float64 action rows, with or without mi_set_model_field, set before or after
 * this call): the same semantics, float64 observations, the info row (and final_info under SAME_STEP) of the last executed inner step.  One call of
 * mi_step is a series of launches on the env's stream with no synchronisation between them: a small kernel that takes every row's sticky decision (the
 * draw from the row's generator, before anything else that generator does in the step) and leaves the effective action row, then num_repeats trips
 * of what the plain step launches ([cooperative physics ->] glue).  A row that terminated or was truncated inside the repeat, or that is in its
 * NEXT_STEP autoreset step, sits the remaining trips out, the cooperative physics included; its outputs, episode bookkeeping and mi_stats are
 * written by the trip in which it finishes.  mi_rollout / mi_rollout_infos are then a host loop over the T steps on the stream (the form the
 * cooperative kinds' rollout always had): sampled actions are drawn first, a sticky action replaces the drawn one, the draw is consumed either way.
 * The state -- the sticky word, the last action row ([num_envs][act_dim] at 8 bytes per component, which after the opening kernel IS the effective
 * row), a reward accumulator and an inner-step word per row -- is device memory allocated by this call; nothing of it appears in mi_get_state, whose
 * flag bits are the two they were.  The env stays on its plain kernels: with (0, any, 0) mi_step launches exactly what it launched before.  Actions are
 * not validated (these kinds never validate a Box action).  The engine keeps a COPY of the last action row; the reference keeps a view of the
 * caller's batch, so a caller that overwrites that batch in place changes the reference's sticky action and not this one's.  mi_set_max_and_skip stays
 * with the classic kinds.
 */
int mi_set_step_wrappers(mi_vecenv *env, int num_repeats, double sticky_probability, int sticky_duration);

/*
 * gymnasium.wrappers.MaxAndSkipObservation(env, skip) (wrappers/stateful_observation.py:564-649) around every scalar env, outside its TimeLimit --
 * what make_vec(id, n, "sync", wrappers=(lambda e: MaxAndSkipObservation(e, skip),)) builds; the reference has no vector form.  Added to ABI 10, which
 * it leaves as it is.  The five classic-control kinds, under the conditions of mi_set_step_wrappers; mi_step, mi_rollout and mi_rollout_infos follow.
 *   A step runs up to `skip` inner steps with the same action and stops after the first that terminates or truncates (TimeLimit counts INNER steps);
 *   reward = 0.0 + r_0 + r_1 ... in that order.  Each sub-environment owns two observation frames (float32, the observation's dtype): the observation
 *   after inner step skip - 2 is written to frame 0, the one after inner step skip - 1 to frame 1, and the step returns the element-wise maximum of the
 *   two frames AS THEY THEN STAND (obs; under SAME_STEP final_obs, with obs the reset observation).  The frames are zeros when the wrapper is
 *   constructed and NOTHING clears them afterwards: not mi_reset (with or without mask), not mi_set_state, not an autoreset.  A step that ended before
 *   it wrote a frame returns the maximum over what an earlier step -- of an earlier episode, or the constructor -- left there.  The NEXT_STEP
 *   autoreset step returns the plain reset observation, reward 0, and repeats nothing; DISABLED refuses a finished row as mi_step always does.
 *   A NaN in either frame comes out (np.max); which zero comes out of +0 and -0 is not pinned, by NumPy's reduction or here.
 *   episode_return / episode_length and mi_stats count one step per call with the summed reward, as under RepeatAction.
 * skip >= 2 switches the wrapper on and zeroes the frames (every call constructs it anew); 0 switches it off; 1 or a negative value:
 * MI_ERR_INVALID_ARGUMENT.  MI_ERR_UNSUPPORTED: another kind, MI_CFG_SHARED_RNG, MI_CFG_FAST_MATH, a step epilogue attached, or RepeatAction on
 * (mi_set_step_wrappers with num_repeats > 0 is refused likewise while this is on: fold the repeat into skip).  StickyAction (num_repeats == 0)
 * composes with it as with RepeatAction: one decision per call, taken first.  The first call that switches it on moves the env to the per-lane
 * kernels for good; the frames live in device memory, allocated by that call: mi_step stays capturable.  mi_get_state / mi_set_state do not carry them;
 * mi_get_max_and_skip_frames copies them out as float32 [2][num_envs][obs_dim] (on_device = 0: host memory, synchronises; 1: device memory,
 * enqueued on the env's stream); MI_ERR_STATE while the wrapper is off.
 */
int mi_set_max_and_skip(mi_vecenv *env, int skip);
int mi_get_max_and_skip_frames(mi_vecenv *env, float *dst, int on_device);

/*
 * Lookahead: the discounted return of `candidates` action sequences of length `horizon` for every sub-environment, each started from the
 * sub-environment's present state, with the env itself left untouched -- what a sampling planner (random shooting, CEM, MPPI) asks of a model.  Added
 * to ABI 10, which it leaves as it is; the reference has no counterpart: it is K * N copies of the env, set_state, `horizon` steps and a reduction.
 * The five classic-control kinds on the exact kernels, in every autoreset mode, with or without mi_set_env_attr (each candidate uses the attributes of
 * its own sub-environment).  Device pointers only; the call enqueues one launch on the env's stream and does not synchronise.
 *   Candidate k of sub-environment i works on a private copy of the lane -- state, elapsed steps, flags, attributes, generator.  For
 *   t = 0 .. horizon - 1 it applies actions[t][k][i] with the sequence of mi_step: the validity check, the env's step, elapsed += 1,
 *   truncated = max_episode_steps > 0 && elapsed >= max_episode_steps.  It stops after the first step that terminates or truncates; later actions
 *   are ignored.
 *   actions     in   [horizon][candidates][N][act_dim]  i64 for the Discrete kinds; Box kinds: actions_dtype = MI_F32 rows, or MI_F64 / MI_F64_WEAK
 *                                                        rows taken un-rounded (mi_step_io.actions_dtype)
 *   returns     out  [candidates][N] f64     G = 0, disc = 1; per step taken: G = G + disc * reward, disc = disc * gamma -- the product rounded
 *                                            before the sum, every operation in float64 in that order
 *   steps       out  [candidates][N] i32     steps taken
 *   terminated  out  [candidates][N] u8 0/1  of the last step taken
 *   truncated   out  [candidates][N] u8 0/1  of the last step taken
 *   final_obs   out  [candidates][N][obs_dim] obs_dtype   the observation after the last step taken
 *   Every output is nullable (NULL = not wanted).
 * A sub-environment that waits for its reset (NEXT_STEP after a finished episode, DISABLED likewise) gives returns 0, steps 0, both flags 0 and its
 * present observation.  ACROBOT with torque_noise_max != 0 draws inside its step: every candidate of sub-environment i draws from a private copy of that
 * sub-environment's generator, so all of them see the noise the env itself would see next, and the generator does not move.
 * Nothing of the env changes: state, elapsed steps, flags, generators, the action stream, mi_stats and the episode statistics are what they were.  An
 * action outside a Discrete space is reported through the sticky error word like mi_step's (the candidate does not move in that step).
 * MI_ERR_UNSUPPORTED: another kind, MI_CFG_SHARED_RNG, MI_CFG_FAST_MATH, mi_set_step_wrappers / mi_set_max_and_skip on, a step epilogue attached.
 * MI_ERR_INVALID_ARGUMENT: horizon or candidates < 1, candidates * N >= 2^31, gamma outside [0, 1], actions NULL, a wrong struct_size or actions_dtype.
 * MI_ERR_STATE: before the first reset, or with an asynchronous step pending.
 */
typedef struct mi_lookahead_io {
    int32_t struct_size;      /* = sizeof(mi_lookahead_io) */
    int32_t actions_dtype;    /* Box kinds: MI_F32 (0, default), MI_F64 or MI_F64_WEAK; ignored by the Discrete kinds */
    const void *actions;
    double *returns;
    int32_t *steps;
    uint8_t *terminated;
    uint8_t *truncated;
    void *final_obs;
    int32_t horizon;
    int32_t candidates;
    double gamma;
} mi_lookahead_io;
int mi_lookahead(mi_vecenv *env, const mi_lookahead_io *io);

/*
 * Lookahead over POLICIES: mi_lookahead with the action of every step computed in the lane from the observation, by a small network whose parameters
 * are the candidate -- what evolution strategies, ARS, CEM over parameters and population-based search ask of a model.  Added to ABI 10, which it
 * leaves as it is.  Everything is mi_lookahead's -- the private copy of the lane (state, elapsed steps, flags, attributes, generator), mi_step's
 * sequence per step, the stop after the first step that terminates or truncates, the outputs and their nullability, the return recurrence, the
 * sub-environment that waits for its reset, the untouched env, the kinds, one launch on the env's stream and no synchronisation -- except where the
 * actions come from:
 *   params      in   [candidates][P] f32, row-major.  Candidate k uses row k for all N sub-environments.
 *   The action of step t is computed from the float32 observation of the candidate's current state (the values mi_step would have returned; first: of
 *   the present state).  OBS = obs_dim, A = the number of actions (Discrete kinds) or act_dim (Box kinds: 1), h = hidden:
 *     h == 0        row = W[A][OBS], b[A]; P = A (OBS + 1).  y[o] = b[o]; then for j = 0 .. OBS - 1 in that order: y[o] = y[o] + W[o][j] * obs[j].
 *     1 <= h <= 256 row = W1[h][OBS], b1[h], W2[A][h], b2[A]; P = h (OBS + 1) + A (h + 1).  y[o] = b2[o]; then for u = 0 .. h - 1 in that order:
 *                   z = b1[u]; for j ascending: z = z + W1[u][j] * obs[j];  a = z > 0 ? z : 0 (a NaN gives 0);  for every o: y[o] = y[o] + W2[o][u] * a.
 *   Every product and every sum is a float32 operation rounded on its own: no FMA, no re-association, subnormals kept.  That order IS the contract;
 *   NumPy reproduces it bit for bit.
 *     Discrete kinds: best = 0; for o = 1 .. A - 1: if y[o] > y[best], best = o.  Strict: the first maximum wins, and no comparison with a NaN holds -- a
 *                     NaN y[o], o >= 1, is never chosen and a NaN y[0] is never displaced (NOT np.argmax's rule, which returns the first NaN).  The
 *                     action is `best`: always inside the space.
 *     Box kinds:      y[0] is the float32 action row, taken as mi_lookahead takes an MI_F32 row: the env's own clip applies, nothing squashes it.
 *   No tanh, no sigmoid: they would need an exact float32 restatement of libm's.
 * MI_ERR_UNSUPPORTED and MI_ERR_STATE: as mi_lookahead.
 * MI_ERR_INVALID_ARGUMENT: hidden outside [0, 256], horizon or candidates < 1, candidates * N >= 2^31, gamma outside [0, 1], params NULL, a wrong struct_size.
 */
typedef struct mi_lookahead_policy_io {
    int32_t struct_size;      /* = sizeof(mi_lookahead_policy_io) */
    const float *params;
    double *returns;
    int32_t *steps;
    uint8_t *terminated;
    uint8_t *truncated;
    void *final_obs;
    int32_t horizon;
    int32_t candidates;
    int32_t hidden;
    double gamma;
} mi_lookahead_policy_io;
int mi_lookahead_policy(mi_vecenv *env, const mi_lookahead_policy_io *io);

/*
 * Stateful vector wrappers as device epilogues of the step path.  All array arguments are DEVICE
 * pointers; work is enqueued on `hip_stream` (NULL = the legacy default stream); nothing synchronises except mi_rms_get/set.
 *
 * mi_running_stats replaces gymnasium/wrappers/utils.py:33-71 RunningMeanStd (mean[dim], var[dim], count; __init__: mean 0,
 * var 1, count = epsilon).  `dtype` is the dtype NumPy holds mean / var in there: MI_F32 for float32 observations
 * (NormalizeObservation builds RunningMeanStd(dtype=float32)), MI_F64 for float64 observations and for the scalar return
 * statistics of NormalizeReward.  mi_rms_get / mi_rms_set move the statistics to / from the host as float64 (checkpointing,
 * `wrapper.obs_rms.mean` ...).
 */
typedef struct mi_running_stats mi_running_stats;
int mi_rms_create(int device, int dim, int dtype, double epsilon, mi_running_stats **out);
void mi_rms_destroy(mi_running_stats *stats);
int mi_rms_get(mi_running_stats *stats, void *hip_stream, double *mean, double *var, double *count);       /* host pointers, synchronises */
int mi_rms_set(mi_running_stats *stats, void *hip_stream, const double *mean, const double *var, const double *count);
/*
 * NormalizeObservation.observations (gymnasium/wrappers/vector/stateful_observation.py:144-160):
 *   if update: obs_rms.update(obs)  [np.mean / np.var over axis 0, then update_mean_var_count_from_moments]
 *   out = ((obs - mean) / sqrt(var + epsilon)).astype(float32)
 * obs: [num_rows][dim] of obs_dtype (MI_F32 / MI_F64), out: [num_rows][dim] float32.
 */
int mi_normalize_observation(mi_running_stats *stats, void *hip_stream, const void *obs, int obs_dtype, int num_rows, double epsilon,
                             int update, void *out);
/*
 * NormalizeReward.step after the wrapped step (gymnasium/wrappers/vector/stateful_reward.py:150-176):
 *   active = all (same_step) | ~prev_done;  accumulated[active] = accumulated[active] * gamma * (1 - terminated) + reward
 *   if update and any(active): return_rms.update(accumulated[active]);  prev_done = terminated | truncated
 *   same_step: accumulated[prev_done] = 0;   out = reward / sqrt(return_rms.var + epsilon)
 * accumulated: [num_envs] float32 (zeroed by the caller on reset()), prev_done: [num_envs] uint8, return_rms: dim 1, MI_F64.
 */
int mi_normalize_reward(mi_running_stats *return_rms, void *hip_stream, float *accumulated, uint8_t *prev_done, const double *reward,
                        const uint8_t *terminated, const uint8_t *truncated, int num_envs, double gamma, double epsilon, int same_step,
                        int update, double *out);
/* ClipReward (gymnasium/wrappers/vector/vectorize_reward.py:115-151 -> np.clip(reward, min, max)); NULL bound = None. */
int mi_clip_reward(int device, void *hip_stream, const double *reward, int num_envs, const double *min_reward, const double *max_reward,
                   double *out);

/*
 * The two normalisations over a whole trajectory (ABI 9): the post-processing of mi_rollout's output, which the wrappers' step path
 * cannot reach.  Each call equals T consecutive calls of the per-step function above on rows t = 0..T-1 -- the statistics are updated
 * from step t's batch, then step t is normalised with the updated statistics (stateful_observation.py:144-160,
 * stateful_reward.py:150-176), and a step without an active row leaves them alone -- in a fixed number of launches: nothing in step t
 * depends on the normalised values of earlier steps.  Scratch memory is the caller's: `workspace` is a device pointer, 8-byte aligned,
 * of at least mi_wrapper_steps_workspace(T, rows, dim) bytes (dim = 1 for the reward pass; -1 = bad argument: T in [1, 65535],
 * rows * dim below 2^31), its contents are not kept between calls.  Nothing is allocated and nothing synchronises.
 *   obs: [T][num_rows][dim] of obs_dtype, out: [T][num_rows][dim] float32; out may alias obs when obs_dtype is MI_F32.
 *   reward / terminated / truncated / out: [T][num_envs]; out may alias reward.  accumulated and prev_done are read at entry and hold
 *   the values after step T at exit.
 * ClipReward over a trajectory is mi_clip_reward over T * num_envs elements.
 */
int64_t mi_wrapper_steps_workspace(int T, int rows, int dim);
int mi_normalize_observation_steps(mi_running_stats *stats, void *hip_stream, const void *obs, int obs_dtype, int T, int num_rows,
                                   double epsilon, int update, void *out, void *workspace, int64_t workspace_bytes);
int mi_normalize_reward_steps(mi_running_stats *return_rms, void *hip_stream, float *accumulated, uint8_t *prev_done, const double *reward,
                              const uint8_t *terminated, const uint8_t *truncated, int T, int num_envs, double gamma, double epsilon,
                              int same_step, int update, double *out, void *workspace, int64_t workspace_bytes);

/*
 * The vector action wrappers (gymnasium/wrappers/vector/vectorize_action.py:183-300) over an action block in device memory, element by element:
 *   MI_TRANSFORM_CLIP            ClipAction:    np.clip(action, p0, p1)   p0 = low, p1 = high of the wrapped Box (transform_action.py:118-120)
 *   MI_TRANSFORM_AFFINE_INVERSE  RescaleAction: (action - p0) / p1        p0 = intercept, p1 = gradient of rescale_box (wrappers/utils.py:263-264)
 * in / out: [elements] device pointers of in_dtype / out_dtype (MI_F32 -> MI_F32, MI_F64 -> MI_F32, MI_F64 -> MI_F64), rows of act_dim entries
 * (elements = T * num_envs * act_dim); element i uses entry i % act_dim of p0 / p1.  The arithmetic runs in in_dtype -- the reference's rows
 * promote against float32 bounds to their own dtype -- and is rounded once to out_dtype, so p0 / p1 must hold float32 values.  NaN propagates
 * as in np.clip.  p0 / p1: HOST pointers of act_dim <= MI_TRANSFORM_MAX_ACT_DIM entries, copied into the kernel's arguments: the call only
 * enqueues on hip_stream -- no allocation, no synchronisation, no state -- and may be captured into a graph.  out must not overlap in.
 * (Added to ABI 10, which it leaves as it is.)
 */
#define MI_TRANSFORM_CLIP 0
#define MI_TRANSFORM_AFFINE_INVERSE 1
#define MI_TRANSFORM_MAX_ACT_DIM 32
int mi_transform_actions(int device, void *hip_stream, const void *in, int in_dtype, void *out, int out_dtype, int64_t elements, int act_dim,
                         int kind, const double *p0, const double *p1);

/*
 * The stateless observation transforms of gymnasium/wrappers/vector/vectorize_observation.py over an observation block in device memory
 * (csrc/observation_wrappers.hip; added to ABI 10, which they leave as it is).  Both calls only enqueue on hip_stream: no allocation, no
 * synchronisation, no state.  out must not overlap in.
 *
 * mi_transform_observations, element by element over in / out: [elements] device pointers of in_dtype / out_dtype:
 *   MI_OBS_AFFINE  RescaleObservation: gradient * obs + intercept (wrappers/utils.py:260-261), MI_F32 -> MI_F32 or MI_F64 -> MI_F64: the product
 *                  rounded once, then the sum rounded once, never an FMA.  Rows of obs_dim <= MI_OBS_MAX_DIM entries (elements = T * num_envs *
 *                  obs_dim); element i uses entry i % obs_dim of gradient / intercept: DEVICE arrays of obs_dim values of in_dtype.
 *   MI_OBS_CAST    DtypeObservation: NumPy's C cast (transform_observation.py:633) from MI_F32 / MI_F64 / MI_I64 to MI_F16 / MI_F32 / MI_F64 / MI_I32 /
 *                  MI_I64 / MI_U8.  Float -> float is rounded once to nearest-even (MI_F64 -> MI_F16 does NOT pass through float32), float -> integer
 *                  truncates (NaN and values outside the target's range: undefined, as in NumPy), integer -> integer keeps the low bits.  obs_dim is
 *                  not used; gradient and intercept are NULL.
 *
 * mi_one_hot, FlattenObservation of a Discrete space or a Tuple of them (spaces/utils.py:167-195): parts = num_parts <= MI_ONE_HOT_MAX_PARTS
 * device columns of `rows` int64 states (HOST array of device pointers; start / width: HOST arrays, the spaces' start and n), out: device
 * [rows][W] int64, W = width[0] + ... : column (width[0] + ... + width[k - 1]) + j of a row is 1 iff parts[k][row] - start[k] == j, everything else 0.
 * A state outside [start, start + n) leaves its segment zero (the reference raises IndexError or wraps a negative index).
 */
#define MI_OBS_AFFINE 0
#define MI_OBS_CAST 1
#define MI_OBS_MAX_DIM 1024
#define MI_ONE_HOT_MAX_PARTS 4
int mi_transform_observations(int device, void *hip_stream, const void *in, int in_dtype, void *out, int out_dtype, int64_t elements, int obs_dim,
                              int kind, const void *gradient, const void *intercept);
int mi_one_hot(int device, void *hip_stream, const int64_t *const *parts, int num_parts, const int64_t *start, const int32_t *width, int64_t rows,
               int64_t *out);

/*
 * gymnasium.wrappers.DiscretizeObservation / DiscretizeAction around EVERY SCALAR env (wrappers/transform_observation.py:755-907,
 * transform_action.py:201-345; the reference has no vector form) over a block in device memory (csrc/discretize.hip; added to ABI 10, which they
 * leave as it is).  Both calls only enqueue on hip_stream -- no allocation, no synchronisation, no state -- and may be captured into a graph.  The
 * device compares, selects and divides integers; every floating-point value it uses was computed on the host by the reference's own NumPy
 * expressions in the Box's dtype.  bins: HOST array of the dimension count's positive entries, copied into the kernel's arguments; lo, hi_clip, edges,
 * centres: DEVICE arrays of the Box's dtype.  The concatenated table is staged in LDS: at most MI_DISCRETIZE_MAX_TABLE entries, a longer one is
 * refused with MI_ERR_INVALID_ARGUMENT (the Python wrappers refuse it in their constructors).
 *
 * mi_discretize_observations: in [rows][obs_dim] MI_F32 / MI_F64 (rows = num_envs for step() and reset(), T * num_envs for a rollout),
 * obs_dim <= MI_DISCRETIZE_MAX_DIM.  Per dimension d: x is clipped to [lo[d], hi_clip[d]] (hi_clip = high - 1e-8 rounded to the Box's dtype; NaN stays
 * NaN), then i_d = the number of edges e of dimension d with !(x < e) -- np.digitize(x, edges) on non-decreasing edges, duplicates included, and NaN in
 * the last bin.  edges: the bins[d] - 1 interior edges of every dimension, concatenated (sum(bins - 1) <= MI_DISCRETIZE_MAX_TABLE; NULL when that is 0).
 * multidiscrete != 0: out [rows][obs_dim] int64 of the i_d; otherwise out [rows] int64 of the mixed-radix sum idx = idx * bins[d] + i_d over d
 * (prod(bins) <= 2^62).
 *
 * mi_discretize_actions: in MI_I64 / MI_I32 indices, out [rows][act_dim] of out_dtype (MI_F32 / MI_F64), act_dim <= MI_TRANSFORM_MAX_ACT_DIM.  centres:
 * the bins[d] bin centres of every dimension, concatenated (sum(bins) <= MI_DISCRETIZE_MAX_TABLE).  multidiscrete != 0: in [rows][act_dim], every index
 * clamped to [0, bins[d] - 1].  Otherwise in [rows] flat indices, unravelled with floor division and floor modulo, last dimension first, in 64 bits
 * (Python's % and //: -1 over 7 bins is bin 6, a flat index never clamps); indices in [0, 2^31) under a prod(bins) < 2^31 take a 32-bit path with the
 * same results.
 */
#define MI_DISCRETIZE_MAX_DIM 32
#define MI_DISCRETIZE_MAX_TABLE 2048
int mi_discretize_observations(int device, void *hip_stream, const void *in, int in_dtype, int64_t rows, int obs_dim, const int32_t *bins,
                               const void *lo, const void *hi_clip, const void *edges, int multidiscrete, int64_t *out);
int mi_discretize_actions(int device, void *hip_stream, const void *in, int in_dtype, int64_t rows, int act_dim, const int32_t *bins,
                          const void *centres, int multidiscrete, void *out, int out_dtype);

/*
 * gymnasium.wrappers.NormalizeObservation / NormalizeReward around EVERY SCALAR env (wrappers/stateful_observation.py:464-561,
 * stateful_reward.py:20-142, wrappers/utils.py:33-71) -- what SyncVectorEnv over wrapped scalar envs computes: one set of running statistics per
 * sub-environment, each updated from a batch of one (csrc/per_env_normalize.hip, arithmetic in csrc/per_env_normalize_internal.h; added to ABI 10,
 * which they leave as it is).  Bit for bit the reference's NumPy arithmetic; no reduction over the batch.  Both calls only enqueue ONE kernel on
 * hip_stream: no allocation, no synchronisation.  All state lives in device arrays the caller owns, described by mi_per_env_state (N = num_envs,
 * D = obs_dim); either half may be absent (obs_mean == NULL / ret_mean == NULL).
 *
 * Observation half.  obs_mean / obs_var: [N][D] of obs_dtype -- MI_F32 for float32 observations, MI_F64 for float64 ones --, initially 0 and 1.
 * obs_count: float64, initially 1e-4; obs_first: 1 while a row has not been updated since construction (MI_F64 only: the reference's arrays are
 * float32 until the first update, which makes that update's var * count a float32 product).  A row's count and flag are read by the D threads of
 * the row, so they are DOUBLE-BUFFERED: [2][N], a call reads half `obs_phase` and writes the other half for every row; the caller flips
 * obs_phase after every call that had an observation block.
 * Reward half, all float64 [N]: acc (the discounted return, initially 0; only `terminated` of a step clears it, never a reset or a truncation),
 * ret_mean / ret_var / ret_count (0, 1, 1e-4), and was_done [N] uint8: the rows that finished in the previous step.  Under
 * MI_AUTORESET_NEXT_STEP such a row is in its autoreset step: reward_out is 0.0 and nothing of the row changes; under SAME_STEP and DISABLED every
 * row takes the step.  was_done is rewritten as terminated | truncated by every call; the caller clears the rows it resets.
 *
 * mi_per_env_normalize_step, what one reset() or step() returns:
 *   obs / obs_out: [N][D] obs_dtype / float32 (NULL: no observation block).  row_mask ([N] uint8, or NULL = every row): rows outside it are left
 *     alone -- statistics untouched, obs_out[row] = prev_out[row] (the batch returned last; prev_out NULL: obs_out[row] is not written).
 *   final_obs / final_out / final_mask (SAME_STEP, or all NULL): for the rows in final_mask the final observation updates the statistics and is
 *     normalised FIRST, then the row's `obs`: two updates in one call.  Rows outside final_mask: final_out is 0.
 *   reward / terminated / truncated / reward_out: [N] (NULL reward: no reward block).
 * mi_per_env_normalize_steps, the T consecutive step() calls of a rollout: obs [T][N][D], obs_out [T][N][D] float32 (may alias obs for MI_F32),
 *   reward / terminated / truncated / reward_out [T][N] (reward_out may alias reward).  Every thread keeps its statistics in registers over the T
 *   steps and stores them once; the result and the state left behind equal T calls of mi_per_env_normalize_step.  NEXT_STEP and DISABLED only
 *   (SAME_STEP needs the final observations: MI_ERR_UNSUPPORTED).
 * N * D must stay below 2^31; T * N * D is indexed in 64 bits.
 */
typedef struct mi_per_env_state {
    void *obs_mean, *obs_var;   /* [N][D] of obs_dtype, or NULL: no NormalizeObservation */
    double *obs_count;          /* [2][N] */
    uint8_t *obs_first;         /* [2][N] */
    int32_t obs_phase;          /* 0 / 1: the half of obs_count / obs_first that is current */
    int32_t obs_dtype;          /* MI_F32 / MI_F64 */
    int32_t obs_dim;
    int32_t obs_update;         /* update_running_mean of NormalizeObservation */
    double obs_epsilon;
    double *acc, *ret_mean, *ret_var, *ret_count; /* [N], or ret_mean == NULL: no NormalizeReward */
    uint8_t *was_done;          /* [N] */
    double gamma, reward_epsilon;
    int32_t reward_update;      /* update_running_mean of NormalizeReward */
    int32_t autoreset_mode;     /* mi_autoreset_mode */
} mi_per_env_state;
int mi_per_env_normalize_step(int device, void *hip_stream, const mi_per_env_state *state, int num_envs, const void *obs, void *obs_out,
                              const uint8_t *row_mask, const void *prev_out, const void *final_obs, void *final_out, const uint8_t *final_mask,
                              const double *reward, const uint8_t *terminated, const uint8_t *truncated, double *reward_out);
int mi_per_env_normalize_steps(int device, void *hip_stream, const mi_per_env_state *state, int T, int num_envs, const void *obs, void *obs_out,
                               const double *reward, const uint8_t *terminated, const uint8_t *truncated, double *reward_out);

/*
 * gymnasium.wrappers.FrameStackObservation / DelayObservation / TimeAwareObservation around EVERY SCALAR env
 * (wrappers/stateful_observation.py:304-461, 35-103, 106-301 under vector/sync_vector_env.py:207-337) -- what SyncVectorEnv over wrapped scalar
 * envs returns (csrc/stateful_observation.hip, index arithmetic in csrc/stateful_observation_internal.h; added to ABI 10, which they leave as it
 * is).  The wrappers move data; the only arithmetic is the normalised time, float32(t / max_timesteps) with the quotient taken in float64, and
 * the exact widenings to float64.  Both calls only enqueue ONE kernel on hip_stream: no allocation, no synchronisation.  One state struct per
 * wrapper; all state lives in device arrays the caller owns (N = num_envs, D = dim, the flat size of one input observation).  A call READS the
 * `_in` arrays and WRITES every entry of the `_out` arrays (never the same memory); the caller swaps them after the call.
 *
 *   MI_SO_FRAME_STACK  depth = stack_size k >= 1.  out [N][k][D] of in_dtype.  carried_in: the stack returned last, [N][k][D] (the caller
 *                      keeps the output; carried_out is not used).  padding: 0 the reset observation, 1 zeros, 2 padding_value ([D] in_dtype).
 *   MI_SO_DELAY        depth = delay >= 0.  out [N][D] of in_dtype.  carried_in / carried_out: the last `delay` raw observations [N][delay][D],
 *                      oldest first; count_in / count_out [N] int32: how many of them (the last ones) the row's queue holds.
 *   MI_SO_TIME_AWARE   out [N][D + 1] of out_dtype: the observation widened, then the time -- int32 counter (normalize_time = 0) or
 *                      float32(t / max_timesteps) -- converted to out_dtype: MI_F64 (float64 observations; float32 ones with the integer
 *                      time), MI_F32 (float32 observations with the normalised time).  dim = 0 gives the time column alone, [N][1] MI_I32 or
 *                      MI_F32 (flatten=False).  count_in / count_out [N] int32: the counters.
 *   pending_in / pending_out [N] uint8, all kinds: the rows that finished in the previous step (under NEXT_STEP their next step is the reset).
 *
 * mi_stateful_observation_step, what one reset() (is_reset = 1) or step() returns.  A reset: rows in row_mask ([N] uint8, NULL = all) reset,
 *   the others keep their state and get prev_out[row] (the batch returned last; NULL: zeros).  A step: under NEXT_STEP the rows of pending_in
 *   reset, the others step; under SAME_STEP (final_obs / final_out / final_mask, or all NULL when no row finished) a row of final_mask first
 *   takes final_obs as a step -- final_out, laid out like out; zeros outside the mask -- and then resets with obs.  terminated / truncated [N]:
 *   the step's flags (pending_out; not read by a reset or under SAME_STEP).
 * mi_stateful_observation_steps, the T consecutive step() calls of a rollout: obs [T][N][D], out [T][N][...], terminated / truncated [T][N].
 *   FrameStack and Delay are one write stream over all T * N outputs (each looks back at most k - 1 / delay steps through the flags), TimeAware
 *   walks the T steps per row.  Values and the state left behind equal T calls of mi_stateful_observation_step, except that FrameStack's new
 *   carried state is out[T - 1], which the caller keeps.  NEXT_STEP and DISABLED only (MI_ERR_UNSUPPORTED under SAME_STEP).
 * The elements of one step (N * k * D) must stay below 2^31; the trajectory is indexed in 64 bits.
 */
enum { MI_SO_FRAME_STACK = 0, MI_SO_DELAY = 1, MI_SO_TIME_AWARE = 2 };
typedef struct mi_stateful_observation_state {
    int32_t kind;             /* MI_SO_* */
    int32_t in_dtype;         /* MI_F32 / MI_F64 */
    int32_t out_dtype;        /* FrameStack / Delay: in_dtype; TimeAware: see above */
    int32_t dim;              /* D */
    int32_t depth;            /* stack_size / delay */
    int32_t padding;          /* FrameStack: 0 reset / 1 zero / 2 custom */
    int32_t normalize_time;   /* TimeAware */
    int32_t max_timesteps;    /* TimeAware with normalize_time */
    int32_t autoreset_mode;   /* mi_autoreset_mode */
    int32_t reserved;
    const void *padding_value;
    const void *carried_in;
    void *carried_out;
    const int32_t *count_in;
    int32_t *count_out;
    const uint8_t *pending_in;
    uint8_t *pending_out;
} mi_stateful_observation_state;
int mi_stateful_observation_step(int device, void *hip_stream, const mi_stateful_observation_state *state, int num_envs, int is_reset, const void *obs,
                                 void *out, const uint8_t *row_mask, const void *prev_out, const void *final_obs, void *final_out,
                                 const uint8_t *final_mask, const uint8_t *terminated, const uint8_t *truncated);
int mi_stateful_observation_steps(int device, void *hip_stream, const mi_stateful_observation_state *state, int T, int num_envs, const void *obs,
                                  void *out, const uint8_t *terminated, const uint8_t *truncated);

/* The same three wrappers as the OUTPUT STAGE of the step kernel (classic-control kinds): mi_step / mi_step_async then return the wrapped
 * observations and rewards in place of the raw ones -- one extra launch per step (the normalisations need the statistics of the WHOLE batch,
 * stateful_observation.py:146-152) instead of the ten of the stand-alone passes, and no staging for host callers: the values are rewritten
 * before the step's single device-to-host copy.  Reward order: ClipReward (clip_pre) -> NormalizeReward -> ClipReward (clip_post); each part
 * optional.  The handles and arrays stay owned by the caller and must outlive the attachment; NULL detaches.  Fused rollouts (mi_rollout)
 * and resets are not affected: normalise a reset observation with mi_normalize_observation, a rollout's trajectory with
 * mi_normalize_observation_steps / mi_normalize_reward_steps / mi_clip_reward on the same handles and arrays. */
typedef struct mi_step_epilogue {
    mi_running_stats *obs_rms;     /* NormalizeObservation: float32 statistics of obs_dim columns, or NULL */
    double obs_epsilon;
    int32_t obs_update;            /* update_running_mean */
    int32_t reward_update;
    mi_running_stats *return_rms;  /* NormalizeReward: scalar float64 statistics, or NULL */
    float *accumulated;            /* [N] device: discounted return per sub-environment */
    uint8_t *prev_done;            /* [N] device */
    double gamma, reward_epsilon;
    int32_t clip_pre, clip_post;   /* bit 0: has min, bit 1: has max */
    double clip_pre_min, clip_pre_max, clip_post_min, clip_post_max;
} mi_step_epilogue;
int mi_set_step_epilogue(mi_vecenv *env, const mi_step_epilogue *epilogue);

#ifdef __cplusplus
}
#endif
#endif /* MI355ENV_H */
