// engine.hip -- libmi355env.so: the host side and the C ABI of include/mi355env.h for the lockstep vector-environment kernels for MI355X (gfx950):
// argument checking, the buffers, the action stream's bookkeeping, and the six family-independent kernels (seed_words_kernel, seed_sequence_kernel,
// sticky_clear_kernel, act_init_kernel, act_sample_kernel, model_transpose_kernel).  No environment family's kernels are instantiated or chosen here:
// the classic-control kinds are classic.hip's (namespace mi_classic), the MuJoCo kinds mujoco.hip's (mi_mujoco, with mjx_model.hip and
// mjx_mass_model.hip behind it), the ToyText kinds tabular.hip's (mi_tabular) -- plain functions that take the env once its arguments are validated and
// its buffers chosen.  So this unit includes none of their kernel headers and compiles in seconds.  What the units of the library share is in
// engine_types.h (structs, mi_vecenv, cross-unit launch functions) and lane_common.h (device helpers).
//
// Execution model: one sub-environment per lane, 256-thread workgroups (4 wavefronts of 64, one per SIMD of a CU);
// at num_envs = 65536 the grid is 256 workgroups = one per CU.  Sub-environment state is struct-of-arrays in HBM
// (component-major float64, so a wavefront's 64 loads of one component are one contiguous 512-byte segment), the
// API-typed outputs (obs rows, reward, flags) are written straight from registers as contiguous per-wavefront
// segments.  TimeLimit, the autoreset state machine, the per-env PCG64 streams and the episode-return bookkeeping
// all live on device; a step() is ONE kernel launch, a rollout(T) is ONE launch for T steps with the state held
// in registers in between (the MuJoCo kinds: physics + glue per step for the cooperative robots, and a series of such trips per step while
// RepeatAction / StickyAction are on, mujoco.hip launch_mj_step_wrapped).  There is no CPU fallback anywhere in this library.
//
// Reference semantics reproduced (paths relative to the reference tree):
//   vector/sync_vector_env.py:187-337  SyncVectorEnv.reset/step incl. NEXT_STEP / SAME_STEP / DISABLED autoreset
//   wrappers/common.py:116-150         TimeLimit
//   wrappers/vector/common.py:156-235  RecordEpisodeStatistics (r, l)
//   envs/classic_control/*.py          dynamics (envs_classic.h)
//   utils/seeding.py:10-42             per-env Generator(PCG64(SeedSequence(seed + i))) (pcg64_dev.h)
//   spaces/multi_discrete.py:176-178, spaces/box.py:463-465   action_space.sample() (rollout with on-device policy)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "engine_types.h"
#include "lane_common.h"
#include "wrappers_internal.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------

__global__ void seed_words_kernel(DevEnv d, const uint64_t *words, const uint8_t *mask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.N || (mask && !mask[i])) return;
#pragma unroll
    for (int k = 0; k < 4; k++) d.rng[(size_t)k * d.N + i] = words[(size_t)4 * i + k];
    if (d.tab.nS < 0) d.state[(size_t)d.N + i] = 0.0;  // Blackjack: a fresh Generator has no buffered 32-bit half
    if (d.tab_fickle_rows) d.state[(size_t)2 * d.N + i] = 0.0;  // fickle Taxi: likewise
}

__global__ void seed_sequence_kernel(DevEnv d, uint64_t first_seed, const uint8_t *mask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.N || (mask && !mask[i])) return;
    uint64_t w[4];
    seed_sequence_words(first_seed + (uint64_t)i, w);
    Pcg64 r;
    r.srandom(w);
    d.rng[i] = (uint64_t)(r.state >> 64), d.rng[(size_t)d.N + i] = (uint64_t)r.state;
    d.rng[(size_t)2 * d.N + i] = (uint64_t)(r.inc >> 64), d.rng[(size_t)3 * d.N + i] = (uint64_t)r.inc;
    if (d.tab.nS < 0) d.state[(size_t)d.N + i] = 0.0;  // Blackjack: a fresh Generator has no buffered 32-bit half
    if (d.tab_fickle_rows) d.state[(size_t)2 * d.N + i] = 0.0;  // fickle Taxi: likewise
}

// ---------------------------------------------------------------------------------------------------------
// The action stream as per-lane states (mi_step with actions == NULL, mi_action_sample): `action_space.sample()` of the BATCHED space is one
// generator drawn in sub-environment order (spaces/multi_discrete.py:176-178 `random(nvec.shape) * nvec`, spaces/box.py:463-465 `uniform(low, high,
// size)` over (N, act_dim) row-major), so lane i owns draws pos + i * D + u of every batch.  act_lane[2][N] holds, per lane, the state whose output IS
// its next draw; a batch later the lane is N * D draws further on (jump).  Kept on the device, the stream needs nothing from the host between
// steps: a captured HIP graph replays sampled steps, and a loop of step(sample()) enqueues no host-to-device traffic.
// ---------------------------------------------------------------------------------------------------------
// mi_reset with StickyAction on: the rows that reset forget their last action and leave a running series (mi_set_step_wrappers)
__global__ __launch_bounds__(kBlock) void sticky_clear_kernel(uint32_t *sticky_word, const uint8_t *mask, int N) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < N && (!mask || mask[i])) sticky_word[i] = 0u;
}

__global__ __launch_bounds__(kBlock) void act_init_kernel(ActionStream as, uint64_t *act_lane, int N, int D) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    u128 s = make_u128(as.state_hi, as.state_lo);
    uint64_t delta = (uint64_t)i * (uint64_t)D + 1ull;  // skip ahead: one affine map per set bit
    for (int j = 0; delta; j++, delta >>= 1)
        if (delta & 1ull) s = as.pow2[j].mult * s + as.pow2[j].plus;
    act_lane[i] = (uint64_t)(s >> 64), act_lane[(size_t)N + i] = (uint64_t)s;
}
// what a draw becomes: Discrete (n > 0): (u * n).astype(int64); Box: uniform(low[u], high[u]).astype(float32) with the space's float32 bounds
struct ActSpec {
    int D;           // act_dim
    double n;        // number of actions of a Discrete sub-space, 0 for Box
    double lo[24], range[24];
};
// T batches: out[t][i][u]; one launch (a host class hands them out one batch per sample() call)
__global__ __launch_bounds__(kBlock) void act_sample_kernel(ActSpec sp, ActionStream as, uint64_t *act_lane, void *out, int T, int N) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const u128 inc = make_u128(as.inc_hi, as.inc_lo);
    u128 s = make_u128(act_lane[i], act_lane[(size_t)N + i]);
    for (int t = 0; t < T; t++) {
        const size_t row = ((size_t)t * N + i) * sp.D;
        for (int u = 0; u < sp.D; u++) {
            const double x = (double)(pcg_output(s) >> 11) * (1.0 / 9007199254740992.0);
            if (sp.n > 0)
                static_cast<int64_t *>(out)[row + u] = (int64_t)(x * sp.n);
            else
                static_cast<float *>(out)[row + u] = (float)(sp.lo[u] + sp.range[u] * x);
            if (u + 1 < sp.D) s = s * pcg_mult() + inc;
        }
        s = as.jump_n.mult * s + as.jump_n.plus;
    }
    act_lane[i] = (uint64_t)(s >> 64), act_lane[(size_t)N + i] = (uint64_t)s;
}

// mi_set_model_field with device values: the caller's [N][width] rows into `width` component-major rows of the env's block
__global__ __launch_bounds__(kBlock) void model_transpose_kernel(const double *src, double *dst, int N, int width) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    for (int c = 0; c < width; c++) dst[(size_t)c * N + i] = src[(size_t)i * width + c];
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------

}  // namespace
// shared with the other translation units of the library (hidden visibility): sets mi_last_error(), returns `code`
namespace mi_internal {
thread_local char g_err[512] = "";
int set_error(int code, const char *msg) {
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}
}  // namespace mi_internal
namespace {

const mi_layout kLayouts[kClassicKinds] = {
    {CartPole::OBS, MI_F32, 1, MI_I64, CartPole::S, 0, {0, 0}},
    {Pendulum::OBS, MI_F32, 1, MI_F32, Pendulum::S, 0, {0, 0}},
    {Acrobot::OBS, MI_F32, 1, MI_I64, Acrobot::S, 0, {0, 0}},
    {MountainCar::OBS, MI_F32, 1, MI_I64, MountainCar::S, 0, {0, 0}},
    {MountainCarContinuous::OBS, MI_F32, 1, MI_F32, MountainCarContinuous::S, 0, {0, 0}},
};
const int kNumActions[MI_ENV_KIND_COUNT] = {2, 0, 3, 3, 0, 0, 0, 0, 0};

// The sticky device error word lives in page-locked host memory (the kernels write it through its device address on the rare error): after
// a stream synchronisation it is simply read, no copy.
int raise_device_error(mi_vecenv *v) {  // precondition: the stream is idle (a kernel in flight could set the word again right after the clear)
    const int err = *v->h_err;
    if (!err) return MI_OK;
    *v->h_err = 0;
    if (v->shared_rng && v->shared.words) {  // the shared-generator mode refuses every step after a bad batch until it has been raised: lift that
        (void)hipMemsetAsync(v->shared.words + 7, 0, sizeof(uint64_t), v->stream);
        (void)hipStreamSynchronize(v->stream);
    }
    if (err == kErrInvalidAction) return fail(MI_ERR_INVALID_ARGUMENT, "action outside the action space");
    if (err == mi_actmask::kErrInvalidSampleArg)
        return fail(MI_ERR_INVALID_ARGUMENT, "action sampling: a mask value other than 0 / 1, or probabilities outside [0, 1] or not summing to 1; the batch was refused");
    return fail(MI_ERR_STATE, "DISABLED autoreset: a finished sub-environment was stepped without reset");
}
int check_device_error(mi_vecenv *v) {
    HIP_TRY(hipStreamSynchronize(v->stream));
    return raise_device_error(v);
}

int set_device(const mi_vecenv *v) {
    HIP_TRY(hipSetDevice(v->device));
    return MI_OK;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int mi_abi_version(void) { return MI355ENV_ABI_VERSION; }
const char *mi_last_error(void) { return mi_internal::g_err; }

int mi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

static int create_buffers(mi_vecenv *v, const mi_config *cfg, int device);

int mi_create(const mi_config *cfg, int device, mi_vecenv **out) {
    if (!cfg || !out || cfg->struct_size != (int32_t)sizeof(mi_config)) return fail(MI_ERR_INVALID_ARGUMENT, "bad mi_config");
    if (cfg->kind < 0 || cfg->kind >= MI_ENV_KIND_COUNT) return fail(MI_ERR_INVALID_ARGUMENT, "unknown env kind");
    if (cfg->num_envs < 1) return fail(MI_ERR_INVALID_ARGUMENT, "num_envs must be >= 1");
    if (cfg->autoreset_mode < 0 || cfg->autoreset_mode > 2) return fail(MI_ERR_INVALID_ARGUMENT, "bad autoreset mode");
    if (cfg->max_episode_steps > (int)kElapsedMask) return fail(MI_ERR_INVALID_ARGUMENT, "max_episode_steps too large");
    if ((cfg->reserved[0] & MI_CFG_SHARED_RNG) && (cfg->kind != MI_ENV_CARTPOLE || cfg->autoreset_mode != MI_AUTORESET_NEXT_STEP))
        return fail(MI_ERR_UNSUPPORTED, "MI_CFG_SHARED_RNG is CartPoleVectorEnv's semantics: MI_ENV_CARTPOLE with NEXT_STEP autoreset only");
    const int ndev = mi_device_count();
    if (ndev == 0)
        return fail(MI_ERR_NO_DEVICE, "no HIP device visible: libmi355env runs on MI355X (gfx950) only and has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(MI_ERR_INVALID_ARGUMENT, "device index out of range");
    mi_vecenv *v = new (std::nothrow) mi_vecenv();
    if (!v) return fail(MI_ERR_HIP, "out of host memory");
    memset(v, 0, sizeof *v);
    v->cfg = *cfg, v->device = device;
    const int rc = create_buffers(v, cfg, device);
    if (rc != MI_OK) {  // a failing allocation half way: release what the earlier ones got (mi_destroy skips the null ones) and keep the message
        const std::string msg = mi_last_error();
        mi_destroy(v);
        return fail(rc, "%s", msg.c_str());
    }
    *out = v;
    return MI_OK;
}

static int create_buffers(mi_vecenv *v, const mi_config *cfg, int device) {
    if (is_mj(cfg->kind)) {
        mi_mujoco::configure(v);  // the robot's layout, and which physics kernel it runs
    } else if (cfg->kind == MI_ENV_BLACKJACK) {
        const mi_layout l = {3, MI_I64, 1, MI_I64, 2, 0, {0, 0}};
        v->lay = l;
        v->d.tab.nS = -1, v->d.tab.nA = 2, v->d.tab.K = 0;  // the marker the kernels branch on (is_blackjack)
        v->tab_loaded = true;
    } else if (is_tab(cfg->kind)) {
        const mi_layout l = {1, MI_I64, 1, MI_I64, cfg->params[2] != 0.0 ? 3 : 2, 1, {0, 0}};  // (the fickle Taxi keeps one more word per sub-env)
        v->lay = l;
    } else {
        v->lay = kLayouts[cfg->kind];
    }
    HIP_TRY(hipSetDevice(device));
    // One engine stream per DEVICE, shared by every env of the process and never destroyed.  A stream is a hardware queue with its own
    // scratch-memory reservation, sized for the hungriest kernel launched on it (the one-lane MuJoCo kernels keep ~20 KB per lane there):
    // a stream per env made a long-lived process that creates and closes many envs (the GPU test-suite: > 100) abort inside the runtime
    // at the first large-scratch launch of some later env.  Sub-environments of different envs are independent, so sharing only serialises
    // launches that a caller wanting overlap can still separate with mi_set_stream.
    {
        static std::mutex mu;
        static hipStream_t shared[64] = {};
        std::lock_guard<std::mutex> lock(mu);
        if (device < 64) {
            if (!shared[device]) HIP_TRY(hipStreamCreateWithFlags(&shared[device], hipStreamNonBlocking));
            v->stream = shared[device];
        } else {
            HIP_TRY(hipStreamCreateWithFlags(&v->own_stream, hipStreamNonBlocking));
            v->stream = v->own_stream;
        }
    }
    const size_t N = (size_t)cfg->num_envs;
    v->grid = (int)((N + kBlock - 1) / kBlock);
    DevEnv &d = v->d;
    d.N = cfg->num_envs, d.max_steps = cfg->max_episode_steps;
    d.solver_newton = (cfg->reserved[0] & MI_CFG_SOLVER_NEWTON) ? 1 : 0;
    d.tab_fickle_rows = (cfg->kind == MI_ENV_TABULAR && cfg->params[2] != 0.0) ? 1 : 0;
    for (int k = 0; k < 16; k++) d.P.p[k] = cfg->params[k];
    HIP_TRY(hipMalloc(&d.state, sizeof(double) * v->lay.state_dim * N));
    HIP_TRY(hipMalloc(&d.meta, sizeof(uint32_t) * N));
    HIP_TRY(hipMalloc(&d.rng, sizeof(uint64_t) * 4 * N));
    HIP_TRY(hipMalloc(&d.ep_ret, sizeof(double) * N));
    HIP_TRY(hipMalloc(&d.ep_len, sizeof(int32_t) * N));
    HIP_TRY(hipMalloc(&d.blk_count, sizeof(uint64_t) * 4 * v->grid));
    HIP_TRY(hipMalloc(&d.blk_ret, sizeof(double) * v->grid));
    HIP_TRY(hipMalloc(&v->d_pow2, sizeof(PcgJump) * 64));
    HIP_TRY(hipMalloc(&v->d_act_lane, sizeof(uint64_t) * 2 * N));
    HIP_TRY(hipMalloc((void **)&v->d_act_ctl, sizeof(mi_actmask::Ctl)));
    HIP_TRY(hipMemsetAsync(v->d_act_ctl, 0, sizeof(mi_actmask::Ctl), v->stream));
    if (v->lay.act_dim == 1 && v->lay.act_dtype == MI_I64) {  // the Discrete kinds: mi_action_sample_masked / _weighted never allocate
        HIP_TRY(hipMalloc((void **)&v->d_act_partial, sizeof(uint32_t) * v->grid));
        HIP_TRY(hipMalloc((void **)&v->d_act_slot, sizeof(uint32_t) * N));
    }
    {
        const char *fr = getenv("MI355ENV_MASKED_FORCE_REPAIR");  // tests: every masked batch through the repair stage
        v->masked_force_repair = fr && fr[0] == '1';
    }
    v->shared_rng = (cfg->reserved[0] & MI_CFG_SHARED_RNG) != 0;
    if (v->shared_rng) {
        HIP_TRY(hipMalloc(&v->shared.words, sizeof(uint64_t) * 8));
        HIP_TRY(hipMalloc(&v->d_shared_pow2, sizeof(PcgJump) * 64));
        HIP_TRY(hipMalloc(&v->shared.blk_done, sizeof(uint32_t) * v->grid));
        HIP_TRY(hipMalloc(&v->shared.blk_prefix, sizeof(uint32_t) * v->grid));
        HIP_TRY(hipMemsetAsync(v->shared.words, 0, sizeof(uint64_t) * 8, v->stream));
        HIP_TRY(hipMemsetAsync(v->shared.blk_done, 0, sizeof(uint32_t) * v->grid, v->stream));
        HIP_TRY(hipMemsetAsync(v->shared.blk_prefix, 0, sizeof(uint32_t) * v->grid, v->stream));
        v->shared.pow2 = v->d_shared_pow2, v->shared.low = -0.05, v->shared.high = 0.05;
    }
    HIP_TRY(hipMemsetAsync(d.state, 0, sizeof(double) * v->lay.state_dim * N, v->stream));
    HIP_TRY(hipMemsetAsync(d.meta, 0, sizeof(uint32_t) * N, v->stream));
    HIP_TRY(hipMemsetAsync(d.rng, 0, sizeof(uint64_t) * 4 * N, v->stream));
    HIP_TRY(hipMemsetAsync(d.ep_ret, 0, sizeof(double) * N, v->stream));
    HIP_TRY(hipMemsetAsync(d.ep_len, 0, sizeof(int32_t) * N, v->stream));
    HIP_TRY(hipMemsetAsync(d.blk_count, 0, sizeof(uint64_t) * 4 * v->grid, v->stream));
    HIP_TRY(hipMemsetAsync(d.blk_ret, 0, sizeof(double) * v->grid, v->stream));
    v->act_bytes = N * (v->lay.act_dtype == MI_I64 ? 8 : 4) * v->lay.act_dim;
    v->act_bytes_max = N * 8 * v->lay.act_dim;  // a Box kind may be handed float64 rows (mi_step_io.actions_dtype)
    v->obs_bytes = N * (v->lay.obs_dtype == MI_F32 ? sizeof(float) : sizeof(double)) * v->lay.obs_dim;
    v->info_bytes = N * sizeof(double) * (v->lay.info_dim > 0 ? v->lay.info_dim : 1);
    {
        const size_t sizes[9] = {v->obs_bytes, sizeof(double) * N, N, N, v->info_bytes, sizeof(double) * N, sizeof(int32_t) * N, v->obs_bytes, v->info_bytes};
        size_t off = 256, start[9];  // (the first 256 bytes are unused: the error word moved to its own page-locked word)
        for (int k = 0; k < 9; k++) start[k] = off, off = (off + sizes[k] + 255) & ~(size_t)255, v->off_end[k] = start[k] + sizes[k];
        v->out_bytes = off;
        HIP_TRY(hipMalloc(&v->d_out, v->out_bytes));
        HIP_TRY(hipHostMalloc((void **)&v->h_out, v->out_bytes, hipHostMallocDefault));
        HIP_TRY(hipMemsetAsync(v->d_out, 0, v->out_bytes, v->stream));
        memset(v->h_out, 0, v->out_bytes);
        HIP_TRY(hipHostMalloc((void **)&v->h_err, 256, hipHostMallocDefault));
        *v->h_err = 0;
        void *derr = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&derr, v->h_err, 0));
        d.error = reinterpret_cast<int *>(derr);
        HIP_TRY(hipHostGetDevicePointer((void **)&v->h_out_dev, v->h_out, 0));
        char *D = v->d_out, *H = v->h_out;
        v->d_obs = D + start[0], v->d_reward = (double *)(D + start[1]), v->d_term = (uint8_t *)(D + start[2]), v->d_trunc = (uint8_t *)(D + start[3]);
        v->d_info = (double *)(D + start[4]), v->d_epret = (double *)(D + start[5]), v->d_eplen = (int32_t *)(D + start[6]);
        v->d_final = D + start[7], v->d_final_info = (double *)(D + start[8]);
        HIP_TRY(hipMalloc(&v->d_actions, v->act_bytes_max));
        HIP_TRY(hipHostMalloc(&v->h_actions, v->act_bytes_max, hipHostMallocDefault));
        memset(v->h_actions, 0, v->act_bytes_max);
        v->h_io.actions = v->h_actions, v->h_io.obs = H + start[0], v->h_io.reward = (double *)(H + start[1]);
        v->h_io.terminated = (uint8_t *)(H + start[2]), v->h_io.truncated = (uint8_t *)(H + start[3]), v->h_io.info = (double *)(H + start[4]);
        v->h_io.episode_return = (double *)(H + start[5]), v->h_io.episode_length = (int32_t *)(H + start[6]);
        v->h_io.final_obs = H + start[7], v->h_io.final_info = (double *)(H + start[8]);
    }
    HIP_TRY(hipMalloc(&v->d_mask, N));
    HIP_TRY(hipMalloc(&v->d_words, sizeof(uint64_t) * 4 * N));
    if (is_mj(cfg->kind)) {
        HIP_TRY(hipMalloc(&v->d_extras, sizeof(double) * v->extras_dim * N));
        HIP_TRY(hipMalloc(&v->d_act_scratch, v->act_bytes));
        HIP_TRY(hipMalloc(&v->d_obs_scratch, v->obs_bytes));
        HIP_TRY(hipMemsetAsync(v->d_extras, 0, sizeof(double) * v->extras_dim * N, v->stream));
    }
    HIP_TRY(hipStreamSynchronize(v->stream));
    return MI_OK;
}

void mi_destroy(mi_vecenv *v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    (void)hipStreamSynchronize(v->stream);
    void *ptrs[] = {v->d.state, v->d.meta, v->d.rng, v->d.ep_ret, v->d.ep_len, v->d.blk_count, v->d.blk_ret, v->d_out,
                    v->d_pow2, v->d_act_lane, v->d_act_stage, v->d_actions, v->d_mask, v->d_words, v->d_extras, v->d_act_scratch, v->d_obs_scratch,
                    v->shared.words, v->d_shared_pow2, v->shared.blk_done, v->shared.blk_prefix, v->d_attr, v->d_model, v->wrap.last_action, v->wrap.sticky_word, v->wrap.frames,
                    v->d_act_ctl, v->d_act_partial, v->d_act_slot, v->d_arg_stage, v->d_wrap_acc, v->d_wrap_inner};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (v->h_out) (void)hipHostFree(v->h_out);
    if (v->h_err) (void)hipHostFree(v->h_err);
    if (v->h_actions) (void)hipHostFree(v->h_actions);
    for (void *p : v->tab_bufs)
        if (p) (void)hipFree(p);
    if (v->d_epi_partial) (void)hipFree(v->d_epi_partial);
    if (v->own_stream) (void)hipStreamDestroy(v->own_stream);
    delete v;
}

// Per-sub-environment attributes (include/mi355env.h MI_ATTR_*): the construction values of a kind's attributes and their number, 0 for a kind
// without.  The order is the one of envs_classic.h *AttrT::attr_default; the constructor's values (mi_config.params) replace the defaults.
static int attr_defaults(const mi_vecenv *v, double *out) {
    switch (v->cfg.kind) {
    case MI_ENV_CARTPOLE: {
        const double d[] = {9.8, 1.0, 0.1, 0.1 + 1.0, 0.5, 0.1 * 0.5, 10.0, 0.02, 0.0, 12 * 2 * kPi / 360, 2.4};
        memcpy(out, d, sizeof d);
        return MI_ATTR_CARTPOLE_COUNT;
    }
    case MI_ENV_PENDULUM: {
        const double d[] = {v->cfg.params[0], 1.0, 1.0, 0.05, 8.0, 2.0};
        memcpy(out, d, sizeof d);
        return MI_ATTR_PENDULUM_COUNT;
    }
    case MI_ENV_ACROBOT: {
        const double d[] = {1.0, 1.0, 1.0, 0.5, 0.5, 1.0, 4 * kPi, 9 * kPi, 0.2, 0.0, 0.0};
        memcpy(out, d, sizeof d);
        return MI_ATTR_ACROBOT_COUNT;
    }
    case MI_ENV_MOUNTAIN_CAR: {
        const double d[] = {0.001, 0.0025, 0.07, -1.2, 0.6, 0.5, v->cfg.params[0]};
        memcpy(out, d, sizeof d);
        return MI_ATTR_MOUNTAIN_CAR_COUNT;
    }
    case MI_ENV_MOUNTAIN_CAR_CONTINUOUS: {
        const double d[] = {-1.0, 1.0, 0.0015, 0.07, -1.2, 0.6, 0.45, v->cfg.params[0]};
        memcpy(out, d, sizeof d);
        return MI_ATTR_MOUNTAIN_CAR_CONTINUOUS_COUNT;
    }
    }
    return 0;
}
static int attr_check(mi_vecenv *v, int attr, double *defaults) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    const int n = attr_defaults(v, defaults);
    if (!n) return fail(MI_ERR_UNSUPPORTED, "per-sub-environment attributes: the five classic-control kinds only");
    if (v->shared_rng) return fail(MI_ERR_UNSUPPORTED, "per-sub-environment attributes: not with MI_CFG_SHARED_RNG (CartPoleVectorEnv has no set_attr)");
    if (v->cfg.reserved[0] & MI_CFG_FAST_MATH) return fail(MI_ERR_UNSUPPORTED, "per-sub-environment attributes: not with MI_CFG_FAST_MATH");
    if (attr < 0 || attr >= n) return fail(MI_ERR_INVALID_ARGUMENT, "attribute id out of range for this kind");
    if (v->has_pending) return fail(MI_ERR_STATE, "an asynchronous step is pending (mi_step_wait)");
    return MI_OK;
}

int mi_set_env_attr(mi_vecenv *v, int attr, const double *values, int on_device) {
    double defaults[16];
    if (const int rc = attr_check(v, attr, defaults)) return rc;
    if (set_device(v)) return MI_ERR_HIP;
    const size_t N = (size_t)v->cfg.num_envs;
    if (!v->d_attr)  // every row at once: a later attribute needs no allocation
        HIP_TRY(hipMalloc(&v->d_attr, sizeof(double) * (size_t)attr_defaults(v, defaults) * N));
    double *row = v->d_attr + (size_t)attr * N;
    if (values && on_device) {
        HIP_TRY(hipMemcpyAsync(row, values, sizeof(double) * N, hipMemcpyDeviceToDevice, v->stream));
    } else {  // staged: the caller may reuse its array as soon as this returns
        std::vector<double> host(N, defaults[attr]);
        if (values) memcpy(host.data(), values, sizeof(double) * N);
        HIP_TRY(hipMemcpyAsync(row, host.data(), sizeof(double) * N, hipMemcpyHostToDevice, v->stream));
        HIP_TRY(hipStreamSynchronize(v->stream));
    }
    v->attr_mask |= 1u << attr;
    return MI_OK;
}

int mi_get_env_attr(mi_vecenv *v, int attr, double *host_out) {
    double defaults[16];
    if (const int rc = attr_check(v, attr, defaults)) return rc;
    if (!host_out) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (set_device(v)) return MI_ERR_HIP;
    const size_t N = (size_t)v->cfg.num_envs;
    if (!(v->attr_mask & (1u << attr))) {
        for (size_t i = 0; i < N; i++) host_out[i] = defaults[attr];
        return MI_OK;
    }
    HIP_TRY(hipMemcpyAsync(host_out, v->d_attr + (size_t)attr * N, sizeof(double) * N, hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    return MI_OK;
}

// Per-sub-environment model fields of the MuJoCo kinds (include/mi355env.h MI_MODEL_*; device side: mjx::LaneModel).  As everywhere on this path the
// parity with `mujoco` is UNPINNED; the CPU oracle, which takes the same fields as data, is the reference.
static bool model_field_info(const mi_vecenv *v, ModelFieldInfo &out) { return v && mi_mujoco::model_field_info(v->cfg.kind, out); }
static int model_field_check(mi_vecenv *v, int field, ModelFieldInfo &f) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (!model_field_info(v, f)) return fail(MI_ERR_UNSUPPORTED, "per-sub-environment model fields: the MuJoCo kinds only");
    if (field < 0 || field >= MI_MODEL_FIELD_COUNT) return fail(MI_ERR_INVALID_ARGUMENT, "model field id out of range");
    if (v->has_pending) return fail(MI_ERR_STATE, "an asynchronous step is pending (mi_step_wait)");
    return MI_OK;
}

int mi_model_field_width(mi_vecenv *v, int field) {
    ModelFieldInfo f;
    if (!model_field_info(v, f) || field < 0 || field >= MI_MODEL_FIELD_COUNT) return -1;
    return f.width[field];
}

int mi_set_model_field(mi_vecenv *v, int field, const double *values, int on_device) {
    ModelFieldInfo f;
    if (const int rc = model_field_check(v, field, f)) return rc;
    const size_t N = (size_t)v->cfg.num_envs;
    const int w = f.width[field];
    if (values && !on_device)
        for (size_t k = 0; k < N * (size_t)w; k++) {
            const double x = values[k];
            if (!(x - x == 0.0)) return fail(MI_ERR_INVALID_ARGUMENT, "mi_set_model_field: non-finite value");
            if (field == MI_MODEL_DOF_DAMPING && x < 0.0) return fail(MI_ERR_INVALID_ARGUMENT, "mi_set_model_field: dof_damping must be >= 0");
            if (field == MI_MODEL_PAIR_FRICTION && x < 1e-5) return fail(MI_ERR_INVALID_ARGUMENT, "mi_set_model_field: pair_friction must be >= 1e-5 (MuJoCo's minimum)");
            if (field == MI_MODEL_BODY_MASS_SCALE && x < 1e-3) return fail(MI_ERR_INVALID_ARGUMENT, "mi_set_model_field: body_mass_scale must be >= 1e-3");
        }
    if (set_device(v)) return MI_ERR_HIP;
    if (!v->d_model) {  // every field at once, at the compiled-in values: a later field needs no allocation (mi_step stays capturable)
        if (!mi_mjmodel::preload(v->cfg.kind)) {  // ... and the per-lane kernels loaded now: a capture may follow this call at once
            (void)hipGetLastError();
            return fail(MI_ERR_HIP, "mi_set_model_field: could not load the per-lane-model kernels");
        }
        double *rows = nullptr;
        HIP_TRY(hipMalloc(&rows, sizeof(double) * (size_t)f.total * N));
        std::vector<double> host((size_t)f.total * N);
        for (int a = 0; a < MI_MODEL_FIELD_COUNT; a++)
            for (int c = 0; c < f.width[a]; c++)
                for (size_t i = 0; i < N; i++) host[(size_t)(f.offset[a] + c) * N + i] = f.defaults[a][c];
        for (int a = 0; a < MI_MODEL_DERIVED_COUNT; a++)  // the compiled model's constants, copied: nothing is derived until a scale is set
            for (int c = 0; c < f.dwidth[a]; c++)
                for (size_t i = 0; i < N; i++) host[(size_t)(f.doffset[a] + c) * N + i] = f.dcompiled[a][c];
        if (hipMemcpyAsync(rows, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, v->stream) != hipSuccess ||
            hipStreamSynchronize(v->stream) != hipSuccess) {
            (void)hipFree(rows);
            return fail(MI_ERR_HIP, "mi_set_model_field: could not initialise the model rows");
        }
        v->d_model = rows, v->d.mj.rows = rows;
        v->mj_coop = false;  // for good: the cooperative kernels read the compiled-in model
    }
    if (field == MI_MODEL_BODY_MASS_SCALE && values && !mi_mjmass::preload(v->cfg.kind)) {  // the kernels with the mass rows, loaded now like the others
        (void)hipGetLastError();
        return fail(MI_ERR_HIP, "mi_set_model_field: could not load the per-lane-model kernels");
    }
    v->model_mask |= 1u << field;
    if (w == 0) return MI_OK;  // (a robot without contact pairs)
    double *dst = v->d_model + (size_t)f.offset[field] * N;
    if (values && on_device) {
        hipLaunchKernelGGL(model_transpose_kernel, dim3(v->grid), dim3(kBlock), 0, v->stream, values, dst, (int)N, w);
        HIP_TRY(hipGetLastError());
    } else {  // staged: the caller may reuse its array as soon as this returns
        std::vector<double> host((size_t)w * N);
        for (int c = 0; c < w; c++)
            for (size_t i = 0; i < N; i++) host[(size_t)c * N + i] = values ? values[i * (size_t)w + c] : f.defaults[field][c];
        HIP_TRY(hipMemcpyAsync(dst, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, v->stream));
        HIP_TRY(hipStreamSynchronize(v->stream));
    }
    if (field != MI_MODEL_BODY_MASS_SCALE) return MI_OK;
    if (values) {  // the constants the model compiler derives from the masses, per sub-environment, on the device and on the env's stream
        if (!mi_mjmass::derive_constants(v->cfg.kind, v->grid, v->stream, v->d_model, (int)N)) return fail(MI_ERR_UNSUPPORTED, "no per-lane-model kernel for this env kind");
        HIP_TRY(hipGetLastError());
    } else {  // the stock model: its compiled-in constants, copied
        const int first = f.doffset[0], rows = f.total - first;  // (the derived rows are the tail of the block)
        std::vector<double> host((size_t)rows * N);
        for (int a = 0; a < MI_MODEL_DERIVED_COUNT; a++)
            for (int c = 0; c < f.dwidth[a]; c++)
                for (size_t i = 0; i < N; i++) host[(size_t)(f.doffset[a] - first + c) * N + i] = f.dcompiled[a][c];
        HIP_TRY(hipMemcpyAsync(v->d_model + (size_t)first * N, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, v->stream));
        HIP_TRY(hipStreamSynchronize(v->stream));
        v->model_mask &= ~(1u << MI_MODEL_BODY_MASS_SCALE);  // no scale is held: back to the kernels without the mass rows (mjx_model.hip)
    }
    return MI_OK;
}

int mi_get_model_field(mi_vecenv *v, int field, double *host_out) {
    ModelFieldInfo f;
    if (const int rc = model_field_check(v, field, f)) return rc;
    if (!host_out) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    const size_t N = (size_t)v->cfg.num_envs;
    const int w = f.width[field];
    if (!(v->model_mask & (1u << field))) {  // never written: the compiled-in values, no synchronisation
        for (size_t i = 0; i < N; i++)
            for (int c = 0; c < w; c++) host_out[i * (size_t)w + c] = f.defaults[field][c];
        return MI_OK;
    }
    if (w == 0) return MI_OK;
    if (set_device(v)) return MI_ERR_HIP;
    std::vector<double> host((size_t)w * N);
    HIP_TRY(hipMemcpyAsync(host.data(), v->d_model + (size_t)f.offset[field] * N, sizeof(double) * host.size(), hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    for (size_t i = 0; i < N; i++)
        for (int c = 0; c < w; c++) host_out[i * (size_t)w + c] = host[(size_t)c * N + i];
    return MI_OK;
}

int mi_get_model_derived(mi_vecenv *v, int which, double *host_out) {
    ModelFieldInfo f;
    if (const int rc = model_field_check(v, MI_MODEL_BODY_MASS_SCALE, f)) return rc;
    if (which < 0 || which >= MI_MODEL_DERIVED_COUNT) return fail(MI_ERR_INVALID_ARGUMENT, "derived model constant id out of range");
    if (!host_out) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    const size_t N = (size_t)v->cfg.num_envs;
    const int w = f.dwidth[which];
    if (!(v->model_mask & (1u << MI_MODEL_BODY_MASS_SCALE))) {  // no scale was ever set: the compiled model's values, no synchronisation
        for (size_t i = 0; i < N; i++)
            for (int c = 0; c < w; c++) host_out[i * (size_t)w + c] = f.dcompiled[which][c];
        return MI_OK;
    }
    if (set_device(v)) return MI_ERR_HIP;
    std::vector<double> host((size_t)w * N);
    HIP_TRY(hipMemcpyAsync(host.data(), v->d_model + (size_t)f.doffset[which] * N, sizeof(double) * host.size(), hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    for (size_t i = 0; i < N; i++)
        for (int c = 0; c < w; c++) host_out[i * (size_t)w + c] = host[(size_t)c * N + i];
    return MI_OK;
}

// RepeatAction / StickyAction of the sub-environments (include/mi355env.h mi_set_step_wrappers; device side: lane_step_wrapped).
int mi_set_step_wrappers(mi_vecenv *v, int num_repeats, double sticky_probability, int sticky_duration) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    const bool mj = is_mj(v->cfg.kind);  // the MuJoCo kinds: trips of the plain step's launches (mujoco.hip launch_mj_step_wrapped)
    if (!mj && (v->cfg.kind < 0 || v->cfg.kind >= kClassicKinds))
        return fail(MI_ERR_UNSUPPORTED, "mi_set_step_wrappers: the five classic-control kinds and the eleven MuJoCo kinds only");
    if (v->shared_rng) return fail(MI_ERR_UNSUPPORTED, "mi_set_step_wrappers: not with MI_CFG_SHARED_RNG (CartPoleVectorEnv has no sub-environments to wrap)");
    if (v->cfg.reserved[0] & MI_CFG_FAST_MATH) return fail(MI_ERR_UNSUPPORTED, "mi_set_step_wrappers: not with MI_CFG_FAST_MATH");
    if (v->has_epi) return fail(MI_ERR_UNSUPPORTED, "mi_set_step_wrappers: not with a step epilogue attached (mi_set_step_epilogue)");
    if (v->has_pending) return fail(MI_ERR_STATE, "an asynchronous step is pending (mi_step_wait)");
    if (v->wrap.skip && num_repeats > 0)
        return fail(MI_ERR_UNSUPPORTED, "mi_set_step_wrappers: not RepeatAction with mi_set_max_and_skip on (fold the repeat into skip)");
    if (num_repeats < 0 || sticky_duration < 0 || sticky_duration >= (1 << 30))
        return fail(MI_ERR_INVALID_ARGUMENT, "mi_set_step_wrappers: num_repeats and sticky_duration must be >= 0 (0: no such wrapper)");
    if (sticky_duration && !(sticky_probability >= 0.0 && sticky_probability < 1.0))
        return fail(MI_ERR_INVALID_ARGUMENT, "mi_set_step_wrappers: sticky_probability must be in [0, 1)");
    if (set_device(v)) return MI_ERR_HIP;
    const size_t N = (size_t)v->cfg.num_envs;
    if (sticky_duration) {
        const size_t last_bytes = sizeof(uint64_t) * N * (mj ? (size_t)v->lay.act_dim : 1);  // (a MuJoCo row: act_dim components at 8 bytes)
        if (!v->wrap.last_action) HIP_TRY(hipMalloc(&v->wrap.last_action, last_bytes));
        if (!v->wrap.sticky_word) HIP_TRY(hipMalloc(&v->wrap.sticky_word, sizeof(uint32_t) * N));
        // a newly constructed StickyAction: last_action None, not stuck
        HIP_TRY(hipMemsetAsync(v->wrap.last_action, 0, last_bytes, v->stream));
        HIP_TRY(hipMemsetAsync(v->wrap.sticky_word, 0, sizeof(uint32_t) * N, v->stream));
    }
    if (mj && (num_repeats > 0 || sticky_duration > 0)) {  // what a row carries from trip to trip; mj_wrap_open_kernel initialises both every step
        if (!v->d_wrap_acc) HIP_TRY(hipMalloc(&v->d_wrap_acc, sizeof(double) * N));
        if (!v->d_wrap_inner) HIP_TRY(hipMalloc(&v->d_wrap_inner, sizeof(uint32_t) * N));
    }
    v->wrap.repeats = num_repeats, v->wrap.sticky_duration = sticky_duration, v->wrap.sticky_p = sticky_duration ? sticky_probability : 0.0;
    v->wrap_on = num_repeats > 0 || sticky_duration > 0 || v->wrap.skip > 0;
    v->wrap_act_kind = -1;
    if (v->wrap_on && !mj) v->per_lane = true;
    return MI_OK;
}

// MaxAndSkipObservation of the sub-environments (include/mi355env.h mi_set_max_and_skip; device side: lane_step_wrapped<..., MAXSKIP>).
int mi_set_max_and_skip(mi_vecenv *v, int skip) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (v->cfg.kind < 0 || v->cfg.kind >= kClassicKinds) return fail(MI_ERR_UNSUPPORTED, "mi_set_max_and_skip: the five classic-control kinds only");
    if (v->shared_rng) return fail(MI_ERR_UNSUPPORTED, "mi_set_max_and_skip: not with MI_CFG_SHARED_RNG (CartPoleVectorEnv has no sub-environments to wrap)");
    if (v->cfg.reserved[0] & MI_CFG_FAST_MATH) return fail(MI_ERR_UNSUPPORTED, "mi_set_max_and_skip: not with MI_CFG_FAST_MATH");
    if (v->has_epi) return fail(MI_ERR_UNSUPPORTED, "mi_set_max_and_skip: not with a step epilogue attached (mi_set_step_epilogue)");
    if (v->wrap.repeats > 0) return fail(MI_ERR_UNSUPPORTED, "mi_set_max_and_skip: not with RepeatAction on (mi_set_step_wrappers; fold the repeat into skip)");
    if (v->has_pending) return fail(MI_ERR_STATE, "an asynchronous step is pending (mi_step_wait)");
    if (skip < 0 || skip == 1) return fail(MI_ERR_INVALID_ARGUMENT, "mi_set_max_and_skip: skip must be >= 2 (0: no such wrapper)");
    if (set_device(v)) return MI_ERR_HIP;
    if (skip) {  // a newly constructed MaxAndSkipObservation: np.zeros((2, *shape))
        const size_t bytes = sizeof(float) * 2 * (size_t)v->cfg.num_envs * (size_t)v->lay.obs_dim;
        if (!v->wrap.frames) HIP_TRY(hipMalloc(&v->wrap.frames, bytes));
        HIP_TRY(hipMemsetAsync(v->wrap.frames, 0, bytes, v->stream));
    }
    v->wrap.skip = skip;
    v->wrap_on = v->wrap.repeats > 0 || v->wrap.sticky_duration > 0 || skip > 0;
    if (v->wrap_on) v->per_lane = true;
    return MI_OK;
}
int mi_get_max_and_skip_frames(mi_vecenv *v, float *dst, int on_device) {
    if (!v || !dst) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (!v->wrap.skip) return fail(MI_ERR_STATE, "mi_get_max_and_skip_frames: MaxAndSkipObservation is not on (mi_set_max_and_skip)");
    if (v->has_pending) return fail(MI_ERR_STATE, "an asynchronous step is pending (mi_step_wait)");
    if (set_device(v)) return MI_ERR_HIP;
    const size_t bytes = sizeof(float) * 2 * (size_t)v->cfg.num_envs * (size_t)v->lay.obs_dim;
    HIP_TRY(hipMemcpyAsync(dst, v->wrap.frames, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, v->stream));
    if (!on_device) HIP_TRY(hipStreamSynchronize(v->stream));
    return MI_OK;
}

// The reference's stateful vector wrappers as the output stage of the classic-control step kernel (include/mi355env.h mi_step_epilogue).
int mi_set_step_epilogue(mi_vecenv *v, const mi_step_epilogue *e) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (v->wrap_on && e) return fail(MI_ERR_UNSUPPORTED, "mi_set_step_epilogue: not with mi_set_step_wrappers on (use the mi_normalize_* passes)");
    if (v->shared_rng && e) return fail(MI_ERR_UNSUPPORTED, "MI_CFG_SHARED_RNG: the step epilogue belongs to the per-sub-environment step kernel");
    if (set_device(v)) return MI_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(v->stream));
    if (!e) {
        v->has_epi = false;
        return MI_OK;
    }
    if (is_mj(v->cfg.kind) || is_tab(v->cfg.kind))
        return fail(MI_ERR_INVALID_ARGUMENT, "mi_set_step_epilogue: only the classic-control kinds fuse the wrappers into their step kernel (use the mi_normalize_* passes)");
    const mi_running_stats *o = e->obs_rms, *r = e->return_rms;
    if (o && (o->dim != v->lay.obs_dim || o->dtype != MI_F32 || o->device != v->device))
        return fail(MI_ERR_INVALID_ARGUMENT, "mi_set_step_epilogue: obs_rms must be float32 statistics of obs_dim columns on the env's device");
    if (r && (r->dim != 1 || r->dtype != MI_F64 || r->device != v->device || !e->accumulated || !e->prev_done))
        return fail(MI_ERR_INVALID_ARGUMENT, "mi_set_step_epilogue: return_rms must be scalar float64 statistics on the env's device, with accumulated and prev_done");
    if ((o && !(e->obs_epsilon > 0)) || (r && (!(e->reward_epsilon > 0) || !(e->gamma >= 0 && e->gamma <= 1))))
        return fail(MI_ERR_INVALID_ARGUMENT, "mi_set_step_epilogue: epsilon must be positive, gamma in [0, 1]");
    if (!v->d_epi_partial) HIP_TRY(hipMalloc(&v->d_epi_partial, sizeof(double) * kEpiCols * (size_t)v->grid));
    EpiDev d = {};
    d.obs_on = o != nullptr, d.obs_update = e->obs_update != 0, d.ret_on = r != nullptr, d.ret_update = e->reward_update != 0;
    d.same_step = v->cfg.autoreset_mode == MI_AUTORESET_SAME_STEP;
    d.clip_pre = e->clip_pre & 3, d.clip_post = e->clip_post & 3;
    d.gamma = (float)e->gamma, d.obs_eps = e->obs_epsilon, d.ret_eps = e->reward_epsilon;
    d.pre_lo = e->clip_pre_min, d.pre_hi = e->clip_pre_max, d.post_lo = e->clip_post_min, d.post_hi = e->clip_post_max;
    d.acc = e->accumulated, d.prev_done = e->prev_done;
    d.partial = v->d_epi_partial, d.step_blocks = v->grid, d.fold_in_finish = v->grid <= kEpiFoldMax;
    v->epi_host = *e;
    v->epi = d, v->has_epi = d.obs_on || d.ret_on || d.clip_pre || d.clip_post;
    return MI_OK;
}

int mi_get_layout(const mi_vecenv *v, mi_layout *out) {
    if (!v || !out) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    *out = v->lay;
    return MI_OK;
}

int mi_set_stream(mi_vecenv *v, void *hip_stream) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    hipStream_t s = (hipStream_t)hip_stream;  // NULL is the legacy default stream (torch's default current stream)
    if (s != v->stream) {
        if (set_device(v)) return MI_ERR_HIP;
        // Order the hand-over between streams with a host synchronise -- unless the NEW stream is being captured into a graph: a synchronising call
        // during a (global-mode) capture is not allowed by the stream-capture rules, even on another stream.  HipVectorEnv.capture_steps synchronises
        // the engine BEFORE it opens the capture, so nothing is pending on the old stream then.
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (s && hipStreamIsCapturing(s, &cap) != hipSuccess) {
            (void)hipGetLastError();
            cap = hipStreamCaptureStatusNone;
        }
        if (cap == hipStreamCaptureStatusNone) HIP_TRY(hipStreamSynchronize(v->stream));
        v->stream = s;
    }
    return MI_OK;
}

int mi_synchronize(mi_vecenv *v) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (set_device(v)) return MI_ERR_HIP;
    return check_device_error(v);
}

static int upload_mask(mi_vecenv *v, const uint8_t *mask, const uint8_t **d_mask) {
    *d_mask = nullptr;
    if (!mask) return MI_OK;
    HIP_TRY(hipMemcpyAsync(v->d_mask, mask, (size_t)v->cfg.num_envs, hipMemcpyHostToDevice, v->stream));
    *d_mask = v->d_mask;
    return MI_OK;
}

// MI_CFG_SHARED_RNG: (re)base the one generator -- its words, a zero draw counter and the jump table of its increment
static int shared_rebase(mi_vecenv *v, const Pcg64 &g) {
    v->shared_base = g;
    const uint64_t words[8] = {(uint64_t)(g.state >> 64), (uint64_t)g.state, (uint64_t)(g.inc >> 64), (uint64_t)g.inc, 0, 0, 0, 0};
    PcgJump tab[64];
    for (int j = 0; j < 64; j++) tab[j] = pcg_jump(g.inc, (u128)1 << j);
    HIP_TRY(hipMemcpyAsync(v->shared.words, words, sizeof words, hipMemcpyHostToDevice, v->stream));
    HIP_TRY(hipMemcpyAsync(v->d_shared_pow2, tab, sizeof tab, hipMemcpyHostToDevice, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));  // both sources are on this stack frame
    v->seeded = true;
    return MI_OK;
}

int mi_seed(mi_vecenv *v, const uint64_t *pcg, const uint8_t *mask) {
    if (!v || !pcg) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (set_device(v)) return MI_ERR_HIP;
    if (v->shared_rng) {
        Pcg64 g;
        g.state = make_u128(pcg[0], pcg[1]), g.inc = make_u128(pcg[2], pcg[3]);
        return shared_rebase(v, g);
    }
    const uint8_t *dm;
    if (int rc = upload_mask(v, mask, &dm)) return rc;
    HIP_TRY(hipMemcpyAsync(v->d_words, pcg, sizeof(uint64_t) * 4 * (size_t)v->cfg.num_envs, hipMemcpyHostToDevice, v->stream));
    hipLaunchKernelGGL(seed_words_kernel, dim3(v->grid), dim3(kBlock), 0, v->stream, v->d, (const uint64_t *)v->d_words, dm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(v->stream));  // the host buffers may be reused by the caller
    v->seeded = true;
    return MI_OK;
}

int mi_seed_sequence(mi_vecenv *v, uint64_t base_seed, uint64_t first_index, const uint8_t *mask) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (set_device(v)) return MI_ERR_HIP;
    if (v->shared_rng) {  // Generator(PCG64(SeedSequence(seed))) -- the same host arithmetic seed_sequence_kernel runs per lane
        if (first_index != 0) return fail(MI_ERR_UNSUPPORTED, "MI_CFG_SHARED_RNG: one generator for all sub-environments, they do not shard (first_index must be 0)");
        uint64_t w[4];
        seed_sequence_words(base_seed, w);
        Pcg64 g;
        g.srandom(w);
        return shared_rebase(v, g);
    }
    const uint8_t *dm;
    if (int rc = upload_mask(v, mask, &dm)) return rc;
    hipLaunchKernelGGL(seed_sequence_kernel, dim3(v->grid), dim3(kBlock), 0, v->stream, v->d, base_seed + first_index, dm);
    HIP_TRY(hipGetLastError());
    if (mask) HIP_TRY(hipStreamSynchronize(v->stream));
    v->seeded = true;
    return MI_OK;
}

int mi_get_rng(mi_vecenv *v, uint64_t *pcg) {
    if (!v || !pcg) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (set_device(v)) return MI_ERR_HIP;
    const size_t N = (size_t)v->cfg.num_envs;
    if (v->shared_rng) {  // the base generator advanced by the draws the device has taken: every row reports the one generator
        uint64_t words[8];
        HIP_TRY(hipMemcpyAsync(words, v->shared.words, sizeof words, hipMemcpyDeviceToHost, v->stream));
        HIP_TRY(hipStreamSynchronize(v->stream));
        const PcgJump j = pcg_jump(v->shared_base.inc, (u128)words[4]);
        const u128 st = j.mult * v->shared_base.state + j.plus;
        for (size_t i = 0; i < N; i++) {
            pcg[4 * i] = (uint64_t)(st >> 64), pcg[4 * i + 1] = (uint64_t)st;
            pcg[4 * i + 2] = (uint64_t)(v->shared_base.inc >> 64), pcg[4 * i + 3] = (uint64_t)v->shared_base.inc;
        }
        return MI_OK;
    }
    std::vector<uint64_t> soa(4 * N);
    HIP_TRY(hipMemcpyAsync(soa.data(), v->d.rng, sizeof(uint64_t) * 4 * N, hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    for (size_t i = 0; i < N; i++)
        for (int k = 0; k < 4; k++) pcg[4 * i + k] = soa[k * N + i];
    return MI_OK;
}

int mi_reset(mi_vecenv *v, const uint8_t *mask, const double *bounds, void *obs, int loc) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (!v->seeded) return fail(MI_ERR_STATE, "reset before seeding");
    if (set_device(v)) return MI_ERR_HIP;
    const uint8_t *dm = mask;
    void *dobs = obs;
    // classic kinds, host caller: the pinned block is where the last observations are (the step kernel writes it directly), so that is what
    // a partial reset must leave untouched for the sub-environments it does not reset
    const bool pinned_obs = loc == MI_HOST && !is_mj(v->cfg.kind);
    if (loc == MI_HOST) {
        if (int rc = upload_mask(v, mask, &dm)) return rc;
        dobs = v->d_obs;  // persistent: rows of un-reset sub-envs keep their last observation (sync_vector_env.py:261)
        if (pinned_obs) dobs = v->h_out_dev + ((char *)v->d_obs - v->d_out);  // (pinned() is declared further down)
    }
    const int has_bounds = bounds != nullptr;
    const double b0 = has_bounds ? bounds[0] : 0.0, b1 = has_bounds ? bounds[1] : 0.0;
    if (is_tab(v->cfg.kind) && !v->tab_loaded) return fail(MI_ERR_STATE, "tabular environment without a table: call mi_tabular_load first");
    int rc = is_tab(v->cfg.kind)  ? mi_tabular::reset(v, dm, (int64_t *)dobs)
             : is_mj(v->cfg.kind) ? mi_mujoco::reset(v, dm, (double *)dobs)
             : v->shared_rng      ? (int)MI_OK
                                  : mi_classic::reset(v, dm, has_bounds, b0, b1, (float *)dobs);
    if (v->shared_rng) {  // CartPoleVectorEnv.reset (cartpole.py:481-503): every sub-environment, bounds kept for the autoresets
        if (mask) return fail(MI_ERR_UNSUPPORTED, "MI_CFG_SHARED_RNG: CartPoleVectorEnv.reset resets every sub-environment (no reset_mask)");
        v->shared.low = has_bounds ? b0 : -0.05, v->shared.high = has_bounds ? b1 : 0.05;
        rc = mi_classic::shared_reset(v, (float *)dobs);
    }
    if (rc) return rc;
    if (v->wrap_on && v->wrap.sticky_duration) {  // StickyAction.reset (stateful_action.py:107-116) of the rows that reset
        hipLaunchKernelGGL(sticky_clear_kernel, dim3(v->grid), dim3(kBlock), 0, v->stream, v->wrap.sticky_word, dm, v->cfg.num_envs);
        HIP_TRY(hipGetLastError());
    }
    v->was_reset = true;
    if (loc == MI_HOST) {
        if (obs && !pinned_obs) HIP_TRY(hipMemcpyAsync(obs, v->d_obs, v->obs_bytes, hipMemcpyDeviceToHost, v->stream));
        HIP_TRY(hipStreamSynchronize(v->stream));
        if (obs && pinned_obs && obs != v->h_io.obs) memcpy(obs, v->h_io.obs, v->obs_bytes);
    }
    return MI_OK;
}

// the address, as the device sees it, of the place in the page-locked block that mirrors `device_ptr` of the device block
static void *pinned(const mi_vecenv *v, const void *device_ptr) { return v->h_out_dev + ((const char *)device_ptr - v->d_out); }

// ---- the action stream's position: host copy (act_rng) <-> per-lane device states (d_act_lane) ------------------------------------------------
static ActionStream action_stream(const mi_vecenv *v) {
    ActionStream as;
    memset(&as, 0, sizeof as);
    as.state_hi = (uint64_t)(v->act_rng.state >> 64), as.state_lo = (uint64_t)v->act_rng.state;
    as.inc_hi = (uint64_t)(v->act_rng.inc >> 64), as.inc_lo = (uint64_t)v->act_rng.inc;
    as.pow2 = v->d_pow2, as.jump_n = v->jump_n;
    return as;
}
// bring the host copy up to date: lane 0's state is the position stepped once (the state whose output is the next draw)
static int action_sync_host(mi_vecenv *v) {
    if (!v->act_on_device) return MI_OK;
    uint64_t w[2];
    HIP_TRY(hipMemcpyAsync(&w[0], v->d_act_lane, sizeof(uint64_t), hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipMemcpyAsync(&w[1], v->d_act_lane + (size_t)v->cfg.num_envs, sizeof(uint64_t), hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    Pcg64 g;
    g.state = make_u128(w[0], w[1]), g.inc = v->act_rng.inc;
    g.unstep();
    v->act_rng.state = g.state;
    v->act_on_device = false;
    return MI_OK;
}
static bool stream_capturing(const mi_vecenv *v) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (v->stream && hipStreamIsCapturing(v->stream, &cap) != hipSuccess) {
        (void)hipGetLastError();
        cap = hipStreamCaptureStatusNone;
    }
    return cap != hipStreamCaptureStatusNone;
}
// per-lane states for the host copy's position (skip-ahead by i * act_dim + 1 draws per lane); a no-op while they are current
static int action_prepare_lanes(mi_vecenv *v) {
    if (v->act_lane_valid) return MI_OK;
    if (stream_capturing(v))
        return fail(MI_ERR_STATE, "the on-device policy's lane states must exist before a stream capture: call mi_action_sample(env, 0, NULL, MI_DEVICE) first");
    hipLaunchKernelGGL(act_init_kernel, dim3(v->grid), dim3(kBlock), 0, v->stream, action_stream(v), v->d_act_lane, v->cfg.num_envs, v->lay.act_dim);
    HIP_TRY(hipGetLastError());
    v->act_lane_valid = true;
    return MI_OK;
}
static int action_spec(const mi_vecenv *v, ActSpec *sp) {
    memset(sp, 0, sizeof *sp);
    sp->D = v->lay.act_dim;
    if (sp->D > 24) return fail(MI_ERR_UNSUPPORTED, "action rows wider than 24");
    const int kind = v->cfg.kind;
    if (is_tab(kind))
        sp->n = (double)v->d.tab.nA;
    else if (kind < kClassicKinds && kNumActions[kind])
        sp->n = (double)kNumActions[kind];
    else if (kind == MI_ENV_PENDULUM)
        sp->lo[0] = -2.0, sp->range[0] = 2.0 - (-2.0);  // Box(-max_torque, max_torque) (pendulum.py:112-114)
    else if (kind == MI_ENV_MOUNTAIN_CAR_CONTINUOUS)
        sp->lo[0] = -1.0, sp->range[0] = 1.0 - (-1.0);  // Box(min_action, max_action) (continuous_mountain_car.py:137-139)
    else if (!mi_mujoco::action_bounds(kind, sp->lo, sp->range))
        return fail(MI_ERR_UNSUPPORTED, "this MuJoCo kind is not built into the HIP engine yet");
    return MI_OK;
}
// T batches of action_space.sample() into `dst` (device), from the lane states
static int action_sample_device(mi_vecenv *v, int T, void *dst) {
    ActSpec sp;
    if (int rc = action_spec(v, &sp)) return rc;
    if (int rc = action_prepare_lanes(v)) return rc;
    hipLaunchKernelGGL(act_sample_kernel, dim3(v->grid), dim3(kBlock), 0, v->stream, sp, action_stream(v), v->d_act_lane, dst, T, v->cfg.num_envs);
    HIP_TRY(hipGetLastError());
    v->act_on_device = true;
    return MI_OK;
}

// StickyAction keeps each lane's last action in the element type it came in (WrapDev::last_action): a batch of another type would replay those bits
// as a value of its own type, so it is refused until the wrappers are set again.
static int sticky_action_kind(mi_vecenv *v, int act_kind) {
    if (!v->wrap_on || !v->wrap.sticky_duration) return MI_OK;
    if (v->wrap_act_kind >= 0 && v->wrap_act_kind != act_kind)
        return fail(MI_ERR_UNSUPPORTED, "StickyAction is on: the element type of the action rows (float32 / float64 / Python floats) must not change between steps");
    v->wrap_act_kind = act_kind;
    return MI_OK;
}

// Enqueue one vector step.  loc == MI_HOST: actions go through the pinned staging block (one H2D), the kernel writes the device output
// block, and ONE D2H brings back the prefix of it that the caller asked for -- or, for the classic kinds, the kernel works on the pinned block
// directly and there is no copy at all; nothing is synchronised here.
static int step_enqueue(mi_vecenv *v, const mi_step_io *io, int loc) {
    if (!v || !io) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (!v->was_reset) return fail(MI_ERR_STATE, "step before reset");
    const bool sample = io->actions == nullptr;  // the on-device policy: step(action_space.sample()) without the host
    if (sample && loc != MI_DEVICE) return fail(MI_ERR_INVALID_ARGUMENT, "actions is NULL (the on-device policy steps device buffers: loc == MI_DEVICE; host callers draw batches with mi_action_sample)");
    if (sample && !v->act_seeded) return fail(MI_ERR_STATE, "a step without actions needs mi_action_seed");
    if (v->has_pending) return fail(MI_ERR_STATE, "mi_step_async: the previous asynchronous step has not been waited for (mi_step_wait)");
    if (set_device(v)) return MI_ERR_HIP;
    // Device callers are asynchronous: an action outside the space (or a finished sub-environment stepped under DISABLED) is recorded by the
    // kernel in the page-locked error word and raised HERE, by the first later step that finds it -- a plain host read, no synchronisation.
    // The word is only CLEARED once the stream is idle (error path only: the common case stays a plain read).
    if (loc == MI_DEVICE && *v->h_err) return check_device_error(v);
    const size_t N = (size_t)v->cfg.num_envs;
    // element type of the action rows: Box kinds take float32 rows or un-rounded float64 rows (include/mi355env.h mi_step_io.actions_dtype)
    const bool box = v->lay.act_dtype == MI_F32;
    if (box && io->actions_dtype != MI_F32 && io->actions_dtype != MI_F64 && io->actions_dtype != MI_F64_WEAK)
        return fail(MI_ERR_INVALID_ARGUMENT, "actions_dtype must be MI_F32, MI_F64 or MI_F64_WEAK");
    const int act_kind = (box && !sample) ? io->actions_dtype : (int)MI_F32;
    if (int rc = sticky_action_kind(v, act_kind)) return rc;
    const size_t act_bytes = act_kind == MI_F32 ? v->act_bytes : v->act_bytes_max;
    StepPtrs p;
    memset(&p, 0, sizeof p);
    bool zc = false;
    // classic control (without a wrapper epilogue) and ToyText draw inside their step kernel; every other configuration runs the stand-alone
    // sampler first and steps on what it wrote
    const bool fused_sample = sample && !is_mj(v->cfg.kind) && !v->shared_rng && !v->has_epi;
    if (loc == MI_HOST) {
        // validate before anything is mutated (cartpole.py:165-167 asserts action_space.contains(action))
        const int na = is_tab(v->cfg.kind) ? v->d.tab.nA : kNumActions[v->cfg.kind];
        if (na) {
            const int64_t *a = (const int64_t *)io->actions;
            for (size_t i = 0; i < N; i++)
                if (a[i] < 0 || a[i] >= na) return fail(MI_ERR_INVALID_ARGUMENT, "action outside the action space");
        }
        if (io->actions != v->h_actions) memcpy(v->h_actions, io->actions, act_bytes);  // callers that fill the pinned array skip this
        // Classic control and ToyText: the step kernel reads the actions from and writes its outputs to the PINNED block itself (coalesced rows of at most
        // 24 bytes per lane stream over PCIe while the kernel runs): no copy-engine hand-offs, 97 -> 85 us per step at 65 536 sub-environments
        // (73 us when the caller's policy writes into the pinned action array).  MI355ENV_ZEROCOPY=0 restores the staged copies (A/B).  Not
        // with a finishing epilogue pass (it would re-read the batch over PCIe) and not for the wide float64 rows of the MuJoCo kinds.
        static const bool zero_copy = !(getenv("MI355ENV_ZEROCOPY") && getenv("MI355ENV_ZEROCOPY")[0] == '0');
        zc = zero_copy && !is_mj(v->cfg.kind) && !(v->has_epi && (v->epi.obs_on || v->epi.ret_on));
        if (zc) {
            void *da = nullptr;
            HIP_TRY(hipHostGetDevicePointer(&da, v->h_actions, 0));
            p.actions = da;
            p.obs = (float *)pinned(v, v->d_obs), p.reward = (double *)pinned(v, v->d_reward);
            p.terminated = (uint8_t *)pinned(v, v->d_term), p.truncated = (uint8_t *)pinned(v, v->d_trunc);
            p.final_obs = io->final_obs ? (float *)pinned(v, v->d_final) : nullptr;
            p.ep_ret = io->episode_return ? (double *)pinned(v, v->d_epret) : nullptr;
            p.ep_len = io->episode_length ? (int32_t *)pinned(v, v->d_eplen) : nullptr;
        } else {
            HIP_TRY(hipMemcpyAsync(v->d_actions, v->h_actions, act_bytes, hipMemcpyHostToDevice, v->stream));
            p.actions = v->d_actions;
            p.obs = (float *)v->d_obs, p.reward = v->d_reward, p.terminated = v->d_term, p.truncated = v->d_trunc;
            p.final_obs = io->final_obs ? (float *)v->d_final : nullptr;
            p.ep_ret = io->episode_return ? v->d_epret : nullptr;
            p.ep_len = io->episode_length ? v->d_eplen : nullptr;
        }
    } else {
        p.actions = io->actions;
        p.obs = (float *)io->obs, p.reward = io->reward, p.terminated = io->terminated, p.truncated = io->truncated;
        p.final_obs = (float *)io->final_obs, p.ep_ret = io->episode_return, p.ep_len = io->episode_length;
        if (fused_sample) {
            if (int rc = action_prepare_lanes(v)) return rc;
            p.act_lane = v->d_act_lane, p.actions_out = io->actions_out, p.act_jump = v->jump_n;
            v->act_on_device = true;
        } else if (sample) {
            void *dst = io->actions_out ? io->actions_out : (is_mj(v->cfg.kind) ? (void *)v->d_act_scratch : v->d_actions);
            if (int rc = action_sample_device(v, 1, dst)) return rc;
            p.actions = dst;
        }
    }
    double *dinfo = loc == MI_HOST ? (io->info ? v->d_info : nullptr) : io->info;
    double *dfinfo = loc == MI_HOST ? (io->final_info ? v->d_final_info : nullptr) : io->final_info;
    if (zc) dinfo = dinfo ? (double *)pinned(v, dinfo) : nullptr, dfinfo = dfinfo ? (double *)pinned(v, dfinfo) : nullptr;
    int rc;
    if (is_tab(v->cfg.kind)) {
        rc = mi_tabular::step(v, p, dinfo, dfinfo, fused_sample);
    } else if (is_mj(v->cfg.kind)) {
        rc = mi_mujoco::step(v, p, dinfo, dfinfo, act_kind);
    } else if (v->shared_rng) {
        if (p.final_obs) return fail(MI_ERR_INVALID_ARGUMENT, "MI_CFG_SHARED_RNG is NEXT_STEP only: no final_obs");
        rc = mi_classic::shared_step(v, p);
    } else {
        rc = mi_classic::step(v, p, act_kind);
    }
    if (rc) return rc;
    if (loc == MI_HOST) {
        // one copy: the block prefix up to the last section somebody wants (sections in h_io order: obs, reward, terminated, truncated,
        // info, episode_return, episode_length, final_obs, final_info)
        const void *want[9] = {io->obs, io->reward, io->terminated, io->truncated, io->info, io->episode_return, io->episode_length, io->final_obs, io->final_info};
        size_t n = 256;
        for (int k = 0; k < 9; k++)
            if (want[k]) n = v->off_end[k];
        if (!zc && n > 256) HIP_TRY(hipMemcpyAsync(v->h_out + 256, v->d_out + 256, n - 256, hipMemcpyDeviceToHost, v->stream));
        v->pending = *io, v->pending_bytes = n, v->has_pending = true;
    }
    return MI_OK;
}

// Wait for the step enqueued by step_enqueue(MI_HOST): synchronise, raise the device error word, and hand the
// sections to the caller's arrays (a plain memcpy out of pinned memory; skipped for arrays that ARE the pinned ones, mi_host_buffers).
static int step_finish(mi_vecenv *v) {
    if (!v->has_pending) return MI_OK;
    v->has_pending = false;
    HIP_TRY(hipStreamSynchronize(v->stream));
    if (int rc = raise_device_error(v)) return rc;
    const size_t N = (size_t)v->cfg.num_envs;
    const mi_step_io &u = v->pending, &h = v->h_io;
    auto out = [](void *dst, const void *src, size_t n) {
        if (dst && dst != src) memcpy(dst, src, n);
    };
    out(u.obs, h.obs, v->obs_bytes), out(u.reward, h.reward, sizeof(double) * N), out(u.terminated, h.terminated, N), out(u.truncated, h.truncated, N);
    out(u.info, h.info, v->info_bytes), out(u.episode_return, h.episode_return, sizeof(double) * N), out(u.episode_length, h.episode_length, sizeof(int32_t) * N);
    out(u.final_obs, h.final_obs, v->obs_bytes), out(u.final_info, h.final_info, v->info_bytes);
    return MI_OK;
}

int mi_step(mi_vecenv *v, const mi_step_io *io, int loc) {
    if (int rc = step_enqueue(v, io, loc)) return rc;
    return loc == MI_HOST ? step_finish(v) : (int)MI_OK;
}

int mi_step_async(mi_vecenv *v, const mi_step_io *io) { return step_enqueue(v, io, MI_HOST); }

int mi_step_wait(mi_vecenv *v) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (!v->has_pending) return fail(MI_ERR_STATE, "mi_step_wait without a pending mi_step_async");
    if (set_device(v)) return MI_ERR_HIP;
    return step_finish(v);
}

int mi_host_buffers(mi_vecenv *v, mi_step_io *out) {
    if (!v || !out) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    *out = v->h_io;
    return MI_OK;
}

int mi_tabular_load(mi_vecenv *v, const mi_tabular_table *t) {
    if (!v || !t) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (v->cfg.kind != MI_ENV_TABULAR) return fail(MI_ERR_INVALID_ARGUMENT, "not a tabular environment");
    if (t->num_states < 1 || t->num_actions < 1 || t->max_outcomes < 1 || t->num_tables < 0) return fail(MI_ERR_INVALID_ARGUMENT, "empty table");
    const size_t M = t->num_tables > 1 ? (size_t)t->num_tables : 1;
    if ((M > 1) != (t->env_table != nullptr)) return fail(MI_ERR_INVALID_ARGUMENT, "env_table goes with num_tables > 1");
    if (M > 1 && v->cfg.params[2] != 0.0) return fail(MI_ERR_UNSUPPORTED, "the fickle Taxi has one table");
    for (size_t i = 0; M > 1 && i < (size_t)v->cfg.num_envs; i++)
        if (t->env_table[i] < 0 || (size_t)t->env_table[i] >= M) return fail(MI_ERR_INVALID_ARGUMENT, "env_table entry out of range");
    if (set_device(v)) return MI_ERR_HIP;
    const size_t cells = M * (size_t)t->num_states * t->num_actions, n = cells * t->max_outcomes;
    const void *src[8] = {t->csprob, t->prob, t->reward, t->isd_csprob, t->next_state, t->count, t->terminated, t->env_table};
    const size_t bytes[8] = {n * 8, n * 8, n * 8, M * (size_t)t->num_states * 8, n * 4, cells * 4, n, (size_t)v->cfg.num_envs * 4};
    for (int k = 0; k < 8; k++) {
        if (k == 7 && M == 1) {
            if (v->tab_bufs[k]) (void)hipFree(v->tab_bufs[k]);
            v->tab_bufs[k] = nullptr;
            continue;
        }
        if (!src[k]) return fail(MI_ERR_INVALID_ARGUMENT, "null table array");
        if (v->tab_bufs[k]) (void)hipFree(v->tab_bufs[k]);
        HIP_TRY(hipMalloc(&v->tab_bufs[k], bytes[k]));
        HIP_TRY(hipMemcpyAsync(v->tab_bufs[k], src[k], bytes[k], hipMemcpyHostToDevice, v->stream));
    }
    HIP_TRY(hipStreamSynchronize(v->stream));
    TabTable &tab = v->d.tab;
    tab.nS = t->num_states, tab.nA = t->num_actions, tab.K = t->max_outcomes;
    tab.csprob = (const double *)v->tab_bufs[0], tab.prob = (const double *)v->tab_bufs[1], tab.reward = (const double *)v->tab_bufs[2];
    tab.isd = (const double *)v->tab_bufs[3], tab.next = (const int32_t *)v->tab_bufs[4], tab.count = (const int32_t *)v->tab_bufs[5];
    tab.term = (const uint8_t *)v->tab_bufs[6], tab.env_table = (const int32_t *)v->tab_bufs[7];
    v->tab_start_state = -1;
    if (M == 1) {  // "first state whose cumulative probability exceeds u" is the same state for every u < 1 when that state's sum is already >= 1
        int first = 0;
        while (first < t->num_states && !(t->isd_csprob[first] > 0.0)) first++;
        if (first < t->num_states && t->isd_csprob[first] >= 1.0) v->tab_start_state = first;
    }
    v->tab_loaded = true;
    return MI_OK;
}

int mi_action_seed(mi_vecenv *v, const uint64_t pcg[4]) {
    if (!v || !pcg) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (set_device(v)) return MI_ERR_HIP;
    const u128 inc = make_u128(pcg[2], pcg[3]);
    const bool same_inc = v->act_seeded && v->act_rng.inc == inc;
    v->act_rng.state = make_u128(pcg[0], pcg[1]);
    v->act_rng.inc = inc;
    v->act_lane_valid = false, v->act_on_device = false;  // the host copy IS the position again
    // a seeded generator has no pending 32-bit half (mi_action_set_buffered hands one over); the two words are adjacent in Ctl
    HIP_TRY(hipMemsetAsync(&v->d_act_ctl->has_uint32, 0, 2 * sizeof(uint32_t), v->stream));
    if (!same_inc) {
        PcgJump tab[64];
        for (int j = 0; j < 64; j++) tab[j] = pcg_jump(inc, (u128)1 << j);
        HIP_TRY(hipMemcpyAsync(v->d_pow2, tab, sizeof tab, hipMemcpyHostToDevice, v->stream));
        HIP_TRY(hipStreamSynchronize(v->stream));
        // per step a lane draws act_dim consecutive values, then skips to its slot in the next step's batch
        v->jump_n = pcg_jump(inc, (u128)v->cfg.num_envs * (u128)v->lay.act_dim - (u128)(v->lay.act_dim - 1));
    }
    v->act_seeded = true;
    // the per-lane states of the new position right away (one act_init_kernel): the first rollout or step(None) after a seed then starts from them.
    // Not inside a stream capture -- the lanes stay invalid there, and the next consumer prepares them or skips ahead as before.
    if (!stream_capturing(v))
        if (int rc = action_prepare_lanes(v)) return rc;
    return MI_OK;
}

// mi_rollout (ex == nullptr) and mi_rollout_infos (ex: the arrays to store besides, at least one of them set).  Every `ex` branch below is an addition:
// without it the dispatch is what it was before the extras existed.
static int rollout_impl(mi_vecenv *v, int T, const mi_rollout_io *io, const RolloutExtra *ex) {
    if (!v || !io) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (!v->was_reset) return fail(MI_ERR_STATE, "rollout before reset");
    if (T < 0) return fail(MI_ERR_INVALID_ARGUMENT, "T must be >= 0");
    if (v->cfg.autoreset_mode == MI_AUTORESET_DISABLED) return fail(MI_ERR_UNSUPPORTED, "rollout needs an autoreset mode");
    if (ex) {
        if ((ex->final_obs || ex->final_info) && v->cfg.autoreset_mode != MI_AUTORESET_SAME_STEP)
            return fail(MI_ERR_INVALID_ARGUMENT, "final_obs / final_info exist under SAME_STEP autoreset only");
        if ((ex->info || ex->final_info) && v->lay.info_dim == 0) return fail(MI_ERR_INVALID_ARGUMENT, "this env kind has no info columns (layout.info_dim == 0)");
    }
    const bool sample = io->actions_in == nullptr;
    if (sample && !v->act_seeded) return fail(MI_ERR_STATE, "rollout without actions needs mi_action_seed");
    if (T == 0) return MI_OK;
    if (set_device(v)) return MI_ERR_HIP;
    // The classic kinds' sampling kernels keep the per-lane states of the action stream (ActionStream::lane): they start from them when they are
    // current and leave them current for the next launch, so the position stays on the device.  Not inside a stream capture: a captured launch
    // skips ahead from the host copy baked into the graph and writes no lane states.
    const bool keep_lanes = sample && !is_tab(v->cfg.kind) && !is_mj(v->cfg.kind) && !v->shared_rng && !stream_capturing(v);
    if (sample && !(keep_lanes && v->act_on_device))  // (earlier steps / samples may have left the position on the device)
        if (int rc = action_sync_host(v)) return rc;
    RolloutPtrs p = {io->actions_in, io->actions_out, io->obs, io->reward, io->terminated, io->truncated};
    const bool box = v->lay.act_dtype == MI_F32;
    if (box && !sample && io->actions_in_dtype != MI_F32 && io->actions_in_dtype != MI_F64 && io->actions_in_dtype != MI_F64_WEAK)
        return fail(MI_ERR_INVALID_ARGUMENT, "actions_in_dtype must be MI_F32, MI_F64 or MI_F64_WEAK");
    const int in_kind = (box && !sample) ? io->actions_in_dtype : (int)MI_F32, in_f64 = in_kind != MI_F32;
    if (in_f64 && io->actions_out) return fail(MI_ERR_INVALID_ARGUMENT, "actions_out echoes float32 rows: not with float64 actions_in");
    if (int rc = sticky_action_kind(v, in_kind)) return rc;
    ActionStream as;
    memset(&as, 0, sizeof as);
    if (sample) {
        as = action_stream(v);
        if (keep_lanes) as.lane = v->d_act_lane, as.lane_valid = v->act_lane_valid ? 1 : 0;
    }
    int rc;
    if (is_tab(v->cfg.kind)) {
        rc = mi_tabular::rollout(v, p, as, T, sample, ex);
    } else if (is_mj(v->cfg.kind)) {
        rc = mi_mujoco::rollout(v, p, as, T, sample, in_f64, ex);
    } else if (v->shared_rng) {
        rc = mi_classic::shared_rollout(v, p, as, T, sample, ex);  // (T step launches: the step kernel's own outputs, row t of the caller's arrays)
    } else if (ex) {
        rc = mi_classic::rollout_infos(v, p, *ex, as, T, sample, in_kind);
    } else {
        rc = mi_classic::rollout(v, p, as, T, sample, in_kind);
    }
    if (rc) return rc;
    if (sample) {  // the host copy of the generator moves past the T*N draws the kernel consumes (stale, and harmlessly so, while act_on_device)
        const PcgJump j = pcg_jump(v->act_rng.inc, (u128)T * (u128)v->cfg.num_envs * (u128)v->lay.act_dim);
        v->act_rng.state = j.mult * v->act_rng.state + j.plus;
        v->act_lane_valid = keep_lanes;  // ... and the lane states with it, where the kernel wrote them
    }
    return MI_OK;
}

int mi_rollout(mi_vecenv *v, int T, const mi_rollout_io *io) { return rollout_impl(v, T, io, nullptr); }

int mi_rollout_infos(mi_vecenv *v, int T, const mi_rollout_io *io, const mi_rollout_extra *extra) {
    if (!extra || !(extra->final_obs || extra->episode_return || extra->episode_length || extra->info || extra->final_info)) return rollout_impl(v, T, io, nullptr);
    const RolloutExtra ex = {extra->final_obs, extra->episode_return, extra->episode_length, extra->info, extra->final_info};
    return rollout_impl(v, T, io, &ex);
}

// What mi_lookahead and mi_lookahead_policy (`who`) refuse alike, in the order both state it: the env's kind, modes and state ...
static int lookahead_env_checks(const mi_vecenv *v, const char *who) {
    if (v->cfg.kind < 0 || v->cfg.kind >= kClassicKinds) return fail(MI_ERR_UNSUPPORTED, "%s: the five classic-control kinds only", who);
    if (v->shared_rng) return fail(MI_ERR_UNSUPPORTED, "%s: not with MI_CFG_SHARED_RNG (CartPoleVectorEnv has no sub-environment generators to copy)", who);
    if (v->cfg.reserved[0] & MI_CFG_FAST_MATH) return fail(MI_ERR_UNSUPPORTED, "%s: not with MI_CFG_FAST_MATH", who);
    if (v->wrap_on) return fail(MI_ERR_UNSUPPORTED, "%s: not with mi_set_step_wrappers / mi_set_max_and_skip on", who);
    if (v->has_epi) return fail(MI_ERR_UNSUPPORTED, "%s: not with a step epilogue attached (mi_set_step_epilogue)", who);
    if (v->has_pending) return fail(MI_ERR_STATE, "an asynchronous step is pending (mi_step_wait)");
    if (!v->was_reset) return fail(MI_ERR_STATE, "%s before reset", who + 3);  // (without the "mi_")
    return MI_OK;
}
// ... and, after the entry point's own check of its input, horizon, candidates and gamma.
static int lookahead_shape_checks(const mi_vecenv *v, const char *who, int horizon, int candidates, double gamma) {
    if (horizon < 1 || candidates < 1) return fail(MI_ERR_INVALID_ARGUMENT, "%s: horizon and candidates must be >= 1", who);
    if ((int64_t)candidates * (int64_t)v->cfg.num_envs >= ((int64_t)1 << 31)) return fail(MI_ERR_INVALID_ARGUMENT, "%s: candidates * num_envs must be < 2^31", who);
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(MI_ERR_INVALID_ARGUMENT, "%s: gamma must be in [0, 1]", who);
    return MI_OK;
}

// The return of K candidate action sequences from every sub-environment's present state (include/mi355env.h mi_lookahead; device side: lookahead.hip).
int mi_lookahead(mi_vecenv *v, const mi_lookahead_io *io) {
    if (!v || !io) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (io->struct_size != (int32_t)sizeof(mi_lookahead_io)) return fail(MI_ERR_INVALID_ARGUMENT, "mi_lookahead: struct_size != sizeof(mi_lookahead_io)");
    if (int rc = lookahead_env_checks(v, "mi_lookahead")) return rc;
    if (!io->actions) return fail(MI_ERR_INVALID_ARGUMENT, "mi_lookahead: actions must not be NULL");
    if (int rc = lookahead_shape_checks(v, "mi_lookahead", io->horizon, io->candidates, io->gamma)) return rc;
    const bool box = v->lay.act_dtype == MI_F32;
    if (box && io->actions_dtype != MI_F32 && io->actions_dtype != MI_F64 && io->actions_dtype != MI_F64_WEAK)
        return fail(MI_ERR_INVALID_ARGUMENT, "actions_dtype must be MI_F32, MI_F64 or MI_F64_WEAK");
    if (set_device(v)) return MI_ERR_HIP;
    return mi_lookahead_unit::launch(v, io->actions, box ? io->actions_dtype : (int)MI_F32, io->horizon, io->candidates, io->gamma, io->returns, io->steps, io->terminated,
                                io->truncated, static_cast<float *>(io->final_obs));
}

// ... and of K candidate POLICIES, evaluated in the lane from the observation of every step (include/mi355env.h mi_lookahead_policy; device side:
// lookahead_policy.hip).
int mi_lookahead_policy(mi_vecenv *v, const mi_lookahead_policy_io *io) {
    if (!v || !io) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (io->struct_size != (int32_t)sizeof(mi_lookahead_policy_io))
        return fail(MI_ERR_INVALID_ARGUMENT, "mi_lookahead_policy: struct_size != sizeof(mi_lookahead_policy_io)");
    if (int rc = lookahead_env_checks(v, "mi_lookahead_policy")) return rc;
    if (!io->params) return fail(MI_ERR_INVALID_ARGUMENT, "mi_lookahead_policy: params must not be NULL");
    if (io->hidden < 0 || io->hidden > 256) return fail(MI_ERR_INVALID_ARGUMENT, "mi_lookahead_policy: hidden must be in [0, 256]");
    if (int rc = lookahead_shape_checks(v, "mi_lookahead_policy", io->horizon, io->candidates, io->gamma)) return rc;
    if (set_device(v)) return MI_ERR_HIP;
    return mi_lookahead_policy_unit::launch(v, io->params, io->hidden, io->horizon, io->candidates, io->gamma, io->returns, io->steps, io->terminated, io->truncated,
                                            static_cast<float *>(io->final_obs));
}

int mi_action_sample(mi_vecenv *v, int T, void *out, int loc) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (T < 0 || (T > 0 && !out)) return fail(MI_ERR_INVALID_ARGUMENT, "mi_action_sample: T >= 0 batches into a non-null array");
    if (!v->act_seeded) return fail(MI_ERR_STATE, "mi_action_sample needs mi_action_seed");
    if (set_device(v)) return MI_ERR_HIP;
    if (T == 0) return action_prepare_lanes(v);
    if (loc == MI_DEVICE) return action_sample_device(v, T, out);
    const size_t bytes = (size_t)T * v->act_bytes;
    if (bytes > v->act_stage_bytes) {
        HIP_TRY(hipStreamSynchronize(v->stream));
        if (v->d_act_stage) (void)hipFree(v->d_act_stage);
        v->d_act_stage = nullptr, v->act_stage_bytes = 0;
        HIP_TRY(hipMalloc(&v->d_act_stage, bytes));
        v->act_stage_bytes = bytes;
    }
    if (int rc = action_sample_device(v, T, v->d_act_stage)) return rc;
    HIP_TRY(hipMemcpyAsync(out, v->d_act_stage, bytes, hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    return MI_OK;
}

int mi_action_get(mi_vecenv *v, uint64_t pcg[4]) {
    if (!v || !pcg) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (!v->act_seeded) return fail(MI_ERR_STATE, "mi_action_get needs mi_action_seed");
    if (set_device(v)) return MI_ERR_HIP;
    if (int rc = action_sync_host(v)) return rc;
    pcg[0] = (uint64_t)(v->act_rng.state >> 64), pcg[1] = (uint64_t)v->act_rng.state;
    pcg[2] = (uint64_t)(v->act_rng.inc >> 64), pcg[3] = (uint64_t)v->act_rng.inc;
    return MI_OK;
}

int mi_action_skip(mi_vecenv *v, int64_t draws) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (!v->act_seeded) return fail(MI_ERR_STATE, "mi_action_skip needs mi_action_seed");
    if (set_device(v)) return MI_ERR_HIP;
    if (int rc = action_sync_host(v)) return rc;
    if (draws == 0) return MI_OK;
    // backwards = forwards by 2^128 - n: the generator's period
    const u128 delta = draws > 0 ? (u128)(uint64_t)draws : (u128)0 - (u128)((uint64_t)0 - (uint64_t)draws);
    const PcgJump j = pcg_jump(v->act_rng.inc, delta);
    v->act_rng.state = j.mult * v->act_rng.state + j.plus;
    v->act_lane_valid = false;
    return MI_OK;
}

// ---- sample(mask=...) / sample(probability=...) (action_mask.hip) ---------------------------------------------------------------------------------
static mi_actmask::Work actmask_work(const mi_vecenv *v, int A) {
    mi_actmask::Work w;
    memset(&w, 0, sizeof w);
    w.ctl = v->d_act_ctl, w.partial = v->d_act_partial, w.slot = v->d_act_slot, w.lane = v->d_act_lane, w.pow2 = v->d_pow2, w.jump_n = v->jump_n;
    w.inc_hi = (uint64_t)(v->act_rng.inc >> 64), w.inc_lo = (uint64_t)v->act_rng.inc;
    w.error = v->d.error, w.N = v->cfg.num_envs, w.A = A, w.force_repair = v->masked_force_repair ? 1 : 0, w.stream = v->stream;
    return w;
}
// weighted == false: `arg` = int8 masks [N][A]; true: float64 probabilities [N][A]
static int action_sample_arg(mi_vecenv *v, const void *arg, void *out, int loc, bool weighted) {
    const char *what = weighted ? "mi_action_sample_weighted" : "mi_action_sample_masked";
    if (!v || !arg || !out) return fail(MI_ERR_INVALID_ARGUMENT, "%s: null argument", what);
    if (loc != MI_HOST && loc != MI_DEVICE) return fail(MI_ERR_INVALID_ARGUMENT, "%s: loc must be MI_HOST or MI_DEVICE", what);
    if (v->lay.act_dim != 1 || v->lay.act_dtype != MI_I64 || !v->d_act_slot) return fail(MI_ERR_UNSUPPORTED, "%s: Discrete action spaces only", what);
    if (!v->act_seeded) return fail(MI_ERR_STATE, "%s needs mi_action_seed", what);
    const int A = is_tab(v->cfg.kind) ? v->d.tab.nA : kNumActions[v->cfg.kind];
    if (A < 1 || A > (weighted ? mi_actmask::kMaxWeightedActions : mi_actmask::kMaxMaskActions))
        return fail(MI_ERR_UNSUPPORTED, weighted ? "%s: up to 7 actions (np.sum's order changes beyond)" : "%s: up to 64 actions", what);
    if (set_device(v)) return MI_ERR_HIP;
    if (*v->h_err) return check_device_error(v);  // an earlier asynchronous call left an error: raise it before anything is consumed
    if (int rc = action_prepare_lanes(v)) return rc;
    const size_t N = (size_t)v->cfg.num_envs, arg_bytes = N * (size_t)A * (weighted ? sizeof(double) : sizeof(int8_t));
    const void *d_arg = arg;
    int64_t *d_out = (int64_t *)out;
    if (loc == MI_HOST) {
        if (arg_bytes > v->arg_stage_bytes) {
            HIP_TRY(hipStreamSynchronize(v->stream));
            if (v->d_arg_stage) (void)hipFree(v->d_arg_stage);
            v->d_arg_stage = nullptr, v->arg_stage_bytes = 0;
            HIP_TRY(hipMalloc(&v->d_arg_stage, arg_bytes));
            v->arg_stage_bytes = arg_bytes;
        }
        HIP_TRY(hipMemcpyAsync(v->d_arg_stage, arg, arg_bytes, hipMemcpyHostToDevice, v->stream));
        d_arg = v->d_arg_stage, d_out = (int64_t *)v->d_actions;
    }
    const mi_actmask::Work w = actmask_work(v, A);
    HIP_TRY(weighted ? mi_actmask::sample_weighted(w, (const double *)d_arg, d_out) : mi_actmask::sample_masked(w, (const int8_t *)d_arg, d_out));
    v->act_on_device = true;  // (a refused batch leaves the lane states where they were: still the position)
    if (loc == MI_HOST) {
        if (int rc = check_device_error(v)) return rc;  // a refused batch: `out` is not written
        HIP_TRY(hipMemcpyAsync(out, d_out, N * sizeof(int64_t), hipMemcpyDeviceToHost, v->stream));
        HIP_TRY(hipStreamSynchronize(v->stream));
    }
    return MI_OK;
}

int mi_action_sample_masked(mi_vecenv *v, const int8_t *mask, void *out, int loc) { return action_sample_arg(v, mask, out, loc, false); }
int mi_action_sample_weighted(mi_vecenv *v, const double *prob, void *out, int loc) { return action_sample_arg(v, prob, out, loc, true); }

int mi_action_get_buffered(mi_vecenv *v, uint32_t *has_uint32, uint32_t *uinteger) {
    if (!v || !has_uint32 || !uinteger) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (!v->act_seeded) return fail(MI_ERR_STATE, "mi_action_get_buffered needs mi_action_seed");
    if (set_device(v)) return MI_ERR_HIP;
    uint32_t w[2];
    HIP_TRY(hipMemcpyAsync(w, &v->d_act_ctl->has_uint32, sizeof w, hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    *has_uint32 = w[0], *uinteger = w[1];
    return MI_OK;
}

int mi_action_set_buffered(mi_vecenv *v, uint32_t has_uint32, uint32_t uinteger) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (!v->act_seeded) return fail(MI_ERR_STATE, "mi_action_set_buffered follows mi_action_seed");
    if (set_device(v)) return MI_ERR_HIP;
    HIP_TRY(mi_actmask::set_buffered(actmask_work(v, 0), has_uint32, uinteger));
    return MI_OK;
}

int mi_get_stats(mi_vecenv *v, mi_stats *out) {
    if (!v || !out) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (set_device(v)) return MI_ERR_HIP;
    std::vector<uint64_t> c(4 * (size_t)v->grid);
    std::vector<double> r((size_t)v->grid);
    HIP_TRY(hipMemcpyAsync(c.data(), v->d.blk_count, sizeof(uint64_t) * c.size(), hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipMemcpyAsync(r.data(), v->d.blk_ret, sizeof(double) * r.size(), hipMemcpyDeviceToHost, v->stream));
    if (int rc = check_device_error(v)) return rc;
    memset(out, 0, sizeof *out);
    for (int b = 0; b < v->grid; b++) {
        out->env_steps += c[4 * b], out->reset_steps += c[4 * b + 1], out->episodes += c[4 * b + 2];
        out->length_sum += c[4 * b + 3], out->return_sum += r[b];
    }
    return MI_OK;
}

int mi_reset_stats(mi_vecenv *v) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (set_device(v)) return MI_ERR_HIP;
    HIP_TRY(hipMemsetAsync(v->d.blk_count, 0, sizeof(uint64_t) * 4 * v->grid, v->stream));
    HIP_TRY(hipMemsetAsync(v->d.blk_ret, 0, sizeof(double) * v->grid, v->stream));
    return MI_OK;
}

int mi_get_state(mi_vecenv *v, double *state, int32_t *elapsed, uint8_t *flags) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (set_device(v)) return MI_ERR_HIP;
    const size_t N = (size_t)v->cfg.num_envs, S = (size_t)v->lay.state_dim;
    std::vector<double> soa(S * N);
    std::vector<uint32_t> meta(N);
    HIP_TRY(hipMemcpyAsync(soa.data(), v->d.state, sizeof(double) * S * N, hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipMemcpyAsync(meta.data(), v->d.meta, sizeof(uint32_t) * N, hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    for (size_t i = 0; i < N; i++) {
        if (state)
            for (size_t k = 0; k < S; k++) state[i * S + k] = soa[k * N + i];
        if (elapsed) elapsed[i] = (int32_t)(meta[i] & kElapsedMask);
        if (flags) flags[i] = (uint8_t)(meta[i] >> kFlagShift);
    }
    return MI_OK;
}

int mi_set_state(mi_vecenv *v, const double *state, const int32_t *elapsed, const uint8_t *flags) {
    if (!v) return fail(MI_ERR_INVALID_ARGUMENT, "null env");
    if (set_device(v)) return MI_ERR_HIP;
    const size_t N = (size_t)v->cfg.num_envs, S = (size_t)v->lay.state_dim;
    if (state) {
        std::vector<double> soa(S * N);
        for (size_t i = 0; i < N; i++)
            for (size_t k = 0; k < S; k++) soa[k * N + i] = state[i * S + k];
        HIP_TRY(hipMemcpyAsync(v->d.state, soa.data(), sizeof(double) * S * N, hipMemcpyHostToDevice, v->stream));
        HIP_TRY(hipStreamSynchronize(v->stream));
    }
    if (elapsed || flags) {
        std::vector<uint32_t> meta(N);
        HIP_TRY(hipMemcpyAsync(meta.data(), v->d.meta, sizeof(uint32_t) * N, hipMemcpyDeviceToHost, v->stream));
        HIP_TRY(hipStreamSynchronize(v->stream));
        for (size_t i = 0; i < N; i++) {
            uint32_t e = meta[i] & kElapsedMask, f = meta[i] >> kFlagShift;
            if (elapsed) e = (uint32_t)elapsed[i] & kElapsedMask;
            if (flags) f = flags[i] & 3u;
            meta[i] = e | (f << kFlagShift);
        }
        HIP_TRY(hipMemcpyAsync(v->d.meta, meta.data(), sizeof(uint32_t) * N, hipMemcpyHostToDevice, v->stream));
        HIP_TRY(hipStreamSynchronize(v->stream));
        if (v->shared_rng && flags)  // the per-workgroup counts of finished sub-environments follow the new flag words
            if (int rc = mi_classic::shared_recount(v)) return rc;
    }
    v->was_reset = true;
    return MI_OK;
}

}  // extern "C"
#pragma GCC visibility pop
