// wrappers.hip -- the reference's stateful vector wrappers as device epilogues of the step path.
//
// What it replaces (gymnasium v1.4.0; all NumPy passes over the (N, ...) batch on one host core in the reference):
//   gymnasium/wrappers/utils.py:33-71                     RunningMeanStd.update / update_mean_var_count_from_moments
//   gymnasium/wrappers/vector/stateful_observation.py     NormalizeObservation.observations: (obs - mean) / sqrt(var + eps)
//   gymnasium/wrappers/vector/stateful_reward.py:140-176  NormalizeReward.step: discounted return per env, its running variance
//   gymnasium/wrappers/vector/vectorize_reward.py:115-151 ClipReward
// The batch never leaves HBM: the statistics of one batch are two column sums (shifted by the running mean, float64) reduced by
// a grid of partial sums + one combine kernel; the normalisation is fused into the pass that follows.  Arithmetic follows the
// reference expression by expression in the dtype NumPy uses there (float32 running statistics for float32 observations,
// float64 otherwise); only the batch mean / variance themselves are computed more accurately than the reference's float32 sums,
// which is why parity of these wrappers is stated as a tolerance (tests/test_gpu_wrappers.py), not bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <new>

#include "../../include/mi355env.h"
#include "wrappers_internal.h"

namespace mi_internal {
int set_error(int code, const char *msg);
}


namespace {
constexpr int kBlock = 256, kMaxGrid = 256;  // 64 Ki partial sums: the one-workgroup-per-column fold costs 85 us with 256 Ki of them

#define W_TRY(expr)                                                                                             \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) {                                                                                 \
            char buf[400];                                                                                      \
            snprintf(buf, sizeof buf, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return mi_internal::set_error(MI_ERR_HIP, buf);                                                     \
        }                                                                                                       \
    } while (0)

using mi_wrap::rd;

// Column sums of (x - shift_c) and (x - shift_c)^2 over the rows selected by `active` (nullptr = all), float64.
// Thread t owns flattened elements t, t + S, t + 2S, ... with S a multiple of `dim`, so it always sees column t % dim and
// consecutive threads read consecutive addresses.
template <class T>
__global__ __launch_bounds__(kBlock) void partial_sums(const T *x, const uint8_t *active, int active_is_done, const double *shift, int N, int dim,
                                                       long S, double *partial) {
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= S) return;
    const int c = (int)(t % dim);
    const double sh = shift[c];
    double s1 = 0, s2 = 0, cnt = 0;
    const long total = (long)N * dim;
    for (long e = t; e < total; e += S) {
        const long row = e / dim;
        if (active && ((active[row] != 0) == (active_is_done != 0))) continue;
        const double v = (double)x[e] - sh;
        s1 += v, s2 += v * v, cnt += 1;
    }
    partial[t] = s1, partial[S + t] = s2, partial[2 * S + t] = cnt;
}

// One block per column: combine the partials, then RunningMeanStd.update_from_moments in the dtype T of the running statistics.
// X = dtype of the batch (np.mean / np.var return it), T = dtype the running statistics are updated in.
template <class T, class X>
__global__ __launch_bounds__(kBlock) void combine_update(const double *partial, long S, int dim, double *mean, double *var, double *count,
                                                         int *rows_out) {
    __shared__ double sh[3][kBlock];
    const int c = blockIdx.x;
    double s1 = 0, s2 = 0, n = 0;
    for (long t = c + (long)threadIdx.x * dim; t < S; t += (long)kBlock * dim) s1 += partial[t], s2 += partial[S + t], n += partial[2 * S + t];
    sh[0][threadIdx.x] = s1, sh[1][threadIdx.x] = s2, sh[2][threadIdx.x] = n;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int k = 0; k < 3; k++) sh[k][threadIdx.x] += sh[k][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double rows = sh[2][0];
    if (c == 0) *rows_out = (int)rows;
    if (rows == 0) return;  // `if self._update_running_mean and np.any(active)`
    double m = mean[c], v = var[c];
    mi_wrap::update_column<T, X>(m, v, *count, sh[0][0], sh[1][0], rows);
    mean[c] = m, var[c] = v;
}
__global__ void bump_count(double *count, const int *rows) {
    if (*rows > 0) *count += (double)*rows;
}

// NormalizeObservation.observations: (obs - mean) / np.sqrt(var + epsilon) in the observation dtype, float32 output for float32
// statistics (stateful_observation.py: new_single_space dtype float32)
template <class XT, class T, class O>
__global__ __launch_bounds__(kBlock) void normalize_obs(const XT *x, const double *mean, const double *var, double eps, long total, int dim, O *out) {
    const long e = (long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % dim);
    const T num = (T)((T)x[e] - (T)mean[c]);
    const T den = (T)sqrt((double)(T)((T)var[c] + (T)eps));  // np.sqrt of a T array is correctly rounded in T
    out[e] = (O)(T)(num / den);
}

// NormalizeReward.step, stateful_reward.py:150-176
__global__ __launch_bounds__(kBlock) void accumulate_return(float *acc, const uint8_t *prev_done, const double *reward, const uint8_t *term, int N,
                                                            float gamma, int same_step) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const bool active = same_step || !prev_done[i];
    if (!active) return;
    // float32 array * Python float -> float32; * (1 - terminated) (int64) -> float64; + reward -> float64; stored as float32
    const float a = acc[i] * gamma;
    acc[i] = (float)((double)a * (term[i] ? 0.0 : 1.0) + reward[i]);
}
__global__ __launch_bounds__(kBlock) void finish_reward(float *acc, uint8_t *prev_done, const double *reward, const uint8_t *term,
                                                        const uint8_t *trunc, const double *var, double eps, int N, int same_step, double *out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const uint8_t done = (term[i] || trunc[i]) ? 1 : 0;
    prev_done[i] = done;
    if (same_step && done) acc[i] = 0.0f;
    out[i] = reward[i] / sqrt(var[0] + eps);
}
__global__ __launch_bounds__(kBlock) void clip_reward(const double *r, int N, double lo, double hi, int has_lo, int has_hi, double *out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    double v = r[i];
    if (has_lo) v = v < lo ? lo : v;  // np.clip(reward, min_reward, max_reward)
    if (has_hi) v = v > hi ? hi : v;
    out[i] = v;
}

long stride_for(int N, int dim) {
    long want = (long)kBlock * kMaxGrid;
    const long total = (long)N * dim;
    if (want > total) want = total;
    return ((want + dim - 1) / dim) * dim;
}

// x: [N][dim] device array of dtype xdtype; rows with active/done semantics as in partial_sums
int update_stats(mi_running_stats *s, hipStream_t st, const void *x, int xdtype, const uint8_t *mask, int mask_is_done, int N) {
    const long S = stride_for(N, s->dim);
    const int grid = (int)((S + kBlock - 1) / kBlock);
    if (xdtype == MI_F32)
        hipLaunchKernelGGL(partial_sums<float>, dim3(grid), dim3(kBlock), 0, st, (const float *)x, mask, mask_is_done, s->mean, N, s->dim, S, s->partial);
    else
        hipLaunchKernelGGL(partial_sums<double>, dim3(grid), dim3(kBlock), 0, st, (const double *)x, mask, mask_is_done, s->mean, N, s->dim, S, s->partial);
    if (s->dtype == MI_F32 && xdtype == MI_F32)
        hipLaunchKernelGGL((combine_update<float, float>), dim3(s->dim), dim3(kBlock), 0, st, s->partial, S, s->dim, s->mean, s->var, s->count, s->flag);
    else if (xdtype == MI_F32)
        hipLaunchKernelGGL((combine_update<double, float>), dim3(s->dim), dim3(kBlock), 0, st, s->partial, S, s->dim, s->mean, s->var, s->count, s->flag);
    else  // float64 batch: the statistics are float64 from the first update on (NumPy promotion)
        hipLaunchKernelGGL((combine_update<double, double>), dim3(s->dim), dim3(kBlock), 0, st, s->partial, S, s->dim, s->mean, s->var, s->count, s->flag);
    hipLaunchKernelGGL(bump_count, dim3(1), dim3(1), 0, st, s->count, s->flag);
    W_TRY(hipGetLastError());
    return MI_OK;
}

// ---- whole trajectories: T consecutive calls of the passes above in a fixed number of launches (mi_normalize_*_steps) -----------------------
// The reference is sequential in t, but nothing in step t depends on the NORMALISED values of earlier steps: the batch moments of every
// step are summed in parallel (shifted by the running mean at entry -- step t - 1's mean is not known yet), one thread per column then
// walks t through RunningMeanStd.update and tabulates the statistics after every step, and one pass normalises each element with the
// statistics of its step.
//   steps_partial_sums  grid (S / kBlock, T)   partial_sums with the step as second grid dimension, S <= kStepPartials + dim sums per step
//   steps_fold          grid (dim, T)          one workgroup per (step, column): its sums, and from them the batch mean and variance
//   steps_scan          dim wavefronts         the only sequential part: T dependent updates per column, no reduction or moment inside
//   steps_normalize_*   grid (elements, T)     normalize_obs / finish_reward's division, statistics indexed by the element's step
constexpr int kStepPartials = 4096;  // per step and moment: the scratch is O(T * partials), the fold stays short
constexpr int kStepBatch = 8;        // the sequential walks fetch this many steps ahead of the arithmetic that depends on them

long steps_stride(int N, int dim) {
    long want = kStepPartials;
    const long total = (long)N * dim;
    if (want > total) want = total;
    return ((want + dim - 1) / dim) * dim;  // <= total, which is a multiple of dim
}

// active: [T][N], 1 = the row counts (nullptr = every row); partial: [T][3][S]
template <class XT>
__global__ __launch_bounds__(kBlock) void steps_partial_sums(const XT *__restrict__ x, const uint8_t *__restrict__ active, const double *__restrict__ shift,
                                                             int N, int dim, int S, double *__restrict__ partial) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= S) return;
    const long step = blockIdx.y, total = (long)N * dim;
    x += step * total, partial += step * 3 * S;
    if (active) active += step * N;
    const double sh = shift[t % dim];
    double s1 = 0, s2 = 0, cnt = 0;
#pragma unroll 4
    for (long e = t; e < total; e += S) {
        if (active && !active[e / dim]) continue;
        const double v = (double)x[e] - sh;
        s1 += v, s2 += v * v, cnt += 1;
    }
    partial[t] = s1, partial[S + t] = s2, partial[2 * S + t] = cnt;
}

// sums: [T][dim][3] = (batch mean, batch variance, rows) in the dtype X of the batch (np.mean / np.var return it), as update_column forms them
template <class X>
__global__ __launch_bounds__(kBlock) void steps_fold(const double *__restrict__ partial, const double *__restrict__ shift, int S, int dim,
                                                     double *__restrict__ sums) {
    __shared__ double sh[3][kBlock];
    const int c = blockIdx.x;
    const long step = blockIdx.y;
    partial += step * 3 * S;
    double s1 = 0, s2 = 0, n = 0;
    for (long t = c + (long)threadIdx.x * dim; t < S; t += (long)kBlock * dim) s1 += partial[t], s2 += partial[S + t], n += partial[2 * S + t];
    sh[0][threadIdx.x] = s1, sh[1][threadIdx.x] = s2, sh[2][threadIdx.x] = n;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int k = 0; k < 3; k++) sh[k][threadIdx.x] += sh[k][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double rows = sh[2][0], m1 = rows > 0 ? sh[0][0] / rows : 0.0;
    double *o = sums + (step * dim + c) * 3;
    o[0] = rd<X>(shift[c] + m1), o[1] = rows > 0 ? rd<X>(fmax(sh[1][0] / rows - m1 * m1, 0.0)) : 0.0, o[2] = rows;
}

template <class T>
__device__ __forceinline__ double normalizer(double var, double eps) {  // np.sqrt(var + epsilon) in the statistics dtype (normalize_obs)
    return (double)(T)sqrt((double)(T)((T)var + (T)eps));
}

// One wavefront per column.  Lane 0: RunningMeanStd.update for t = 0..steps-1 from the folded batch moments (T = dtype the running statistics are
// updated in, as combine_update), the mean and variance after every step into table [steps][2][dim], the final statistics into the handle's second
// buffer set (the count is shared by the columns, so it cannot be rewritten while other workgroups still read it).  Then all lanes turn the
// variances into np.sqrt(var + epsilon), side by side: a lone wavefront pays for every instruction it issues, so only the dependent chain stays
// sequential.  update == 0: table is one row, the statistics as they are.
template <class T>
__global__ __launch_bounds__(64) void steps_scan(const double *__restrict__ sums, int steps, int dim, int update, double eps, const double *mean,
                                                 const double *var, const double *count, double *mean2, double *var2, double *count2, double *table) {
    const int c = blockIdx.x;
    if (!update) {
        if (threadIdx.x == 0) table[c] = mean[c], table[dim + c] = normalizer<T>(var[c], eps);
        return;
    }
    if (threadIdx.x == 0) {
        double m = mean[c], v = var[c], n = *count;
        for (int t0 = 0; t0 < steps; t0 += kStepBatch) {
            double s[kStepBatch][3];
#pragma unroll
            for (int k = 0; k < kStepBatch; k++) {
                if (t0 + k >= steps) break;
                const double *p = sums + ((long)(t0 + k) * dim + c) * 3;
                s[k][0] = p[0], s[k][1] = p[1], s[k][2] = p[2];
            }
#pragma unroll
            for (int k = 0; k < kStepBatch; k++) {
                if (t0 + k >= steps) break;
                if (s[k][2] > 0) {  // `if self._update_running_mean and np.any(active)`
                    mi_wrap::update_column_from_moments<T>(m, v, n, s[k][0], s[k][1], s[k][2]);
                    n += s[k][2];
                }
                double *row = table + (long)(t0 + k) * 2 * dim;
                row[c] = m, row[dim + c] = v;
            }
        }
        mean2[c] = m, var2[c] = v;
        if (c == 0) *count2 = n;
    }
    __syncthreads();  // (orders lane 0's table rows before the other lanes' reads)
    for (int t = threadIdx.x; t < steps; t += 64) {
        double *row = table + (long)t * 2 * dim;
        row[dim + c] = normalizer<T>(row[dim + c], eps);
    }
}

template <class T>
__device__ __forceinline__ float normalized(T x, const double *row, int dim, int c) {  // normalize_obs, the square root taken in steps_scan
    const T num = (T)(x - (T)row[c]);
    return (float)(T)(num / (T)row[dim + c]);
}

// table_stride: 2 * dim (a row per step) or 0 (frozen statistics); total = N * dim elements per step
template <class XT, class T>
__global__ __launch_bounds__(kBlock) void steps_normalize_obs(const XT *x, const double *__restrict__ table, long table_stride, int total, int dim,
                                                              float *out) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    const long step = blockIdx.y, g = step * total + e;
    out[g] = normalized<T>((T)x[g], table + step * table_stride, dim, e % dim);
}
// float32 observations with N * dim a multiple of 4 and 16-byte aligned arrays: four elements per thread, 128-bit loads and stores
template <class T>
__global__ __launch_bounds__(kBlock) void steps_normalize_obs4(const float4 *x, const double *__restrict__ table, long table_stride, int quads, int dim,
                                                               float4 *out) {
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= quads) return;
    const long step = blockIdx.y, g = step * quads + q;
    const double *row = table + step * table_stride;
    const float4 v = x[g];
    float r[4] = {v.x, v.y, v.z, v.w};
    int c = (int)(4u * (unsigned)q % (unsigned)dim);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        r[k] = normalized<T>((T)r[k], row, dim, c);
        c = c + 1 == dim ? 0 : c + 1;
    }
    out[g] = make_float4(r[0], r[1], r[2], r[3]);
}

// NormalizeReward.step for t = 0..steps-1, one thread per sub-environment: accumulate_return and the prev_done / same_step bookkeeping of
// finish_reward, operation by operation.  acc_traj[t][i]: the discounted return the statistics of step t see, active_traj[t][i]: whether they
// see it (nullptr under SAME_STEP: every row counts); both nullptr when the statistics are frozen.
__global__ __launch_bounds__(kBlock) void steps_accumulate_return(float *acc, uint8_t *prev_done, const double *__restrict__ reward,
                                                                  const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc, int steps, int N,
                                                                  float gamma, int same_step, float *__restrict__ acc_traj,
                                                                  uint8_t *__restrict__ active_traj) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    float a = acc[i];
    bool pd = prev_done[i] != 0;
    for (int t0 = 0; t0 < steps; t0 += kStepBatch) {
        double r[kStepBatch];
        uint8_t te[kStepBatch], tr[kStepBatch];
#pragma unroll
        for (int k = 0; k < kStepBatch; k++) {
            if (t0 + k >= steps) break;
            const long g = (long)(t0 + k) * N + i;
            r[k] = reward[g], te[k] = term[g], tr[k] = trunc[g];
        }
#pragma unroll
        for (int k = 0; k < kStepBatch; k++) {
            if (t0 + k >= steps) break;
            const long g = (long)(t0 + k) * N + i;
            const bool active = same_step || !pd;
            if (active) {
                // float32 array * Python float -> float32; * (1 - terminated) (int64) -> float64; + reward -> float64; stored as float32
                const float d = a * gamma;
                a = (float)((double)d * (te[k] ? 0.0 : 1.0) + r[k]);
            }
            if (acc_traj) acc_traj[g] = a;
            if (active_traj) active_traj[g] = active ? 1 : 0;
            pd = te[k] || tr[k];
            if (same_step && pd) a = 0.0f;
        }
    }
    acc[i] = a, prev_done[i] = pd ? 1 : 0;
}
// reward / np.sqrt(return_rms.var + epsilon) with the variance after the element's step (table rows: [mean, sqrt(var + epsilon)])
__global__ __launch_bounds__(kBlock) void steps_scale_reward(const double *reward, const double *__restrict__ table, long table_stride, int N, double *out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const long step = blockIdx.y, g = step * N + i;
    out[g] = reward[g] / table[step * table_stride + 1];
}

// the caller's scratch, in doubles first: partial [T][3][S], sums [T][dim][3], table [T][2][dim]; then (dim 1: the reward pass) the
// accumulated-return trajectory [T][rows] float32 and its activity mask [T][rows] uint8
struct StepsLayout {
    long S;
    size_t partial, sums, table, traj, mask, bytes;
};
bool steps_layout(int T, int rows, int dim, StepsLayout *l) {
    if (T < 1 || T > 65535 || rows < 1 || dim < 1 || (long)rows * dim > 0x7fffffffL - kStepPartials) return false;
    l->S = steps_stride(rows, dim);
    size_t at = 0;
    l->partial = at, at += sizeof(double) * 3 * (size_t)T * l->S;
    l->sums = at, at += sizeof(double) * 3 * (size_t)T * dim;
    l->table = at, at += sizeof(double) * 2 * (size_t)T * dim;
    l->traj = at, at += dim == 1 ? sizeof(float) * (size_t)T * rows : 0;
    l->mask = at, at += dim == 1 ? (size_t)T * rows : 0;
    l->bytes = (at + 255) & ~(size_t)255;
    return true;
}
void swap_sets(mi_running_stats *s) {  // steps_scan wrote the second buffer set (as the step epilogue does, classic.hip epilogue_swap)
    double *t;
    t = s->mean, s->mean = s->mean2, s->mean2 = t;
    t = s->var, s->var = s->var2, s->var2 = t;
    t = s->count, s->count = s->count2, s->count2 = t;
}

// sums + fold + scan over x: [T][N][dim] (update != 0), or the one-row table of the statistics as they are; returns the table's row stride
int steps_statistics(mi_running_stats *s, hipStream_t st, const void *x, int xdtype, const uint8_t *active, int T, int N, double eps, int update,
                     const StepsLayout &l, char *ws, long *table_stride) {
    double *partial = (double *)(ws + l.partial), *sums = (double *)(ws + l.sums), *table = (double *)(ws + l.table);
    const int dim = s->dim, S = (int)l.S;
    if (update) {
        const dim3 g((unsigned)((S + kBlock - 1) / kBlock), (unsigned)T);
        if (xdtype == MI_F32)
            hipLaunchKernelGGL(steps_partial_sums<float>, g, dim3(kBlock), 0, st, (const float *)x, active, s->mean, N, dim, S, partial);
        else
            hipLaunchKernelGGL(steps_partial_sums<double>, g, dim3(kBlock), 0, st, (const double *)x, active, s->mean, N, dim, S, partial);
        if (xdtype == MI_F32)
            hipLaunchKernelGGL(steps_fold<float>, dim3((unsigned)dim, (unsigned)T), dim3(kBlock), 0, st, partial, s->mean, S, dim, sums);
        else
            hipLaunchKernelGGL(steps_fold<double>, dim3((unsigned)dim, (unsigned)T), dim3(kBlock), 0, st, partial, s->mean, S, dim, sums);
    }
    // float64 batch: the statistics are float64 from the first update on (NumPy promotion), as update_stats
    if (s->dtype == MI_F32 && xdtype == MI_F32)
        hipLaunchKernelGGL(steps_scan<float>, dim3((unsigned)dim), dim3(64), 0, st, sums, T, dim, update, eps, s->mean, s->var, s->count, s->mean2, s->var2, s->count2, table);
    else
        hipLaunchKernelGGL(steps_scan<double>, dim3((unsigned)dim), dim3(64), 0, st, sums, T, dim, update, eps, s->mean, s->var, s->count, s->mean2, s->var2, s->count2, table);
    W_TRY(hipGetLastError());
    if (update) swap_sets(s);
    *table_stride = update ? 2L * dim : 0;
    return MI_OK;
}
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int mi_rms_create(int device, int dim, int dtype, double epsilon, mi_running_stats **out) {
    if (!out || dim < 1 || (dtype != MI_F32 && dtype != MI_F64)) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "bad mi_rms_create argument");
    if (mi_device_count() == 0) return mi_internal::set_error(MI_ERR_NO_DEVICE, "no HIP device visible: the wrappers run on the GPU only");
    W_TRY(hipSetDevice(device));
    mi_running_stats *s = new (std::nothrow) mi_running_stats();
    if (!s) return mi_internal::set_error(MI_ERR_HIP, "out of host memory");
    s->device = device, s->dim = dim, s->dtype = dtype;
    W_TRY(hipMalloc(&s->mean, sizeof(double) * dim));
    W_TRY(hipMalloc(&s->var, sizeof(double) * dim));
    W_TRY(hipMalloc(&s->count, sizeof(double)));
    W_TRY(hipMalloc(&s->mean2, sizeof(double) * dim));
    W_TRY(hipMalloc(&s->var2, sizeof(double) * dim));
    W_TRY(hipMalloc(&s->count2, sizeof(double)));
    W_TRY(hipMalloc(&s->flag, sizeof(int)));
    W_TRY(hipMalloc(&s->partial, sizeof(double) * 3 * ((size_t)kBlock * kMaxGrid + dim)));
    // RunningMeanStd.__init__ (wrappers/utils.py:37-41): mean = 0, var = 1, count = epsilon
    double *h = new double[2 * (size_t)dim + 1];
    for (int k = 0; k < dim; k++) h[k] = 0.0, h[dim + k] = 1.0;
    h[2 * dim] = epsilon;
    W_TRY(hipMemcpy(s->mean, h, sizeof(double) * dim, hipMemcpyHostToDevice));
    W_TRY(hipMemcpy(s->var, h + dim, sizeof(double) * dim, hipMemcpyHostToDevice));
    W_TRY(hipMemcpy(s->count, h + 2 * dim, sizeof(double), hipMemcpyHostToDevice));
    delete[] h;
    *out = s;
    return MI_OK;
}

void mi_rms_destroy(mi_running_stats *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(s->mean), (void)hipFree(s->var), (void)hipFree(s->count), (void)hipFree(s->partial), (void)hipFree(s->flag);
    (void)hipFree(s->mean2), (void)hipFree(s->var2), (void)hipFree(s->count2);
    delete s;
}

int mi_rms_get(mi_running_stats *s, void *hip_stream, double *mean, double *var, double *count) {
    if (!s) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "null statistics handle");
    W_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (mean) W_TRY(hipMemcpyAsync(mean, s->mean, sizeof(double) * s->dim, hipMemcpyDeviceToHost, st));
    if (var) W_TRY(hipMemcpyAsync(var, s->var, sizeof(double) * s->dim, hipMemcpyDeviceToHost, st));
    if (count) W_TRY(hipMemcpyAsync(count, s->count, sizeof(double), hipMemcpyDeviceToHost, st));
    W_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_rms_set(mi_running_stats *s, void *hip_stream, const double *mean, const double *var, const double *count) {
    if (!s) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "null statistics handle");
    W_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (mean) W_TRY(hipMemcpyAsync(s->mean, mean, sizeof(double) * s->dim, hipMemcpyHostToDevice, st));
    if (var) W_TRY(hipMemcpyAsync(s->var, var, sizeof(double) * s->dim, hipMemcpyHostToDevice, st));
    if (count) W_TRY(hipMemcpyAsync(s->count, count, sizeof(double), hipMemcpyHostToDevice, st));
    W_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_normalize_observation(mi_running_stats *s, void *hip_stream, const void *obs, int obs_dtype, int num_rows, double epsilon, int update,
                             void *out) {
    if (!s || !obs || !out || num_rows < 1) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "bad mi_normalize_observation argument");
    if (obs_dtype != MI_F32 && obs_dtype != MI_F64) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "observations must be float32 or float64");
    W_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (update) {
        const int rc = update_stats(s, st, obs, obs_dtype, nullptr, 0, num_rows);
        if (rc) return rc;
    }
    const long total = (long)num_rows * s->dim;
    const dim3 g((unsigned)((total + kBlock - 1) / kBlock)), b(kBlock);
    // arithmetic in the NumPy-promoted dtype of (observation, statistics); the result is cast to float32 (`.astype(np.float32)`)
    if (obs_dtype == MI_F32 && s->dtype == MI_F32)
        hipLaunchKernelGGL((normalize_obs<float, float, float>), g, b, 0, st, (const float *)obs, s->mean, s->var, epsilon, total, s->dim, (float *)out);
    else if (obs_dtype == MI_F32)
        hipLaunchKernelGGL((normalize_obs<float, double, float>), g, b, 0, st, (const float *)obs, s->mean, s->var, epsilon, total, s->dim, (float *)out);
    else
        hipLaunchKernelGGL((normalize_obs<double, double, float>), g, b, 0, st, (const double *)obs, s->mean, s->var, epsilon, total, s->dim, (float *)out);
    W_TRY(hipGetLastError());
    return MI_OK;
}

int mi_normalize_reward(mi_running_stats *return_rms, void *hip_stream, float *accumulated, uint8_t *prev_done, const double *reward,
                        const uint8_t *terminated, const uint8_t *truncated, int num_envs, double gamma, double epsilon, int same_step,
                        int update, double *out) {
    if (!return_rms || return_rms->dim != 1 || !accumulated || !prev_done || !reward || !terminated || !truncated || !out || num_envs < 1)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "bad mi_normalize_reward argument");
    W_TRY(hipSetDevice(return_rms->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const dim3 g((unsigned)((num_envs + kBlock - 1) / kBlock)), b(kBlock);
    hipLaunchKernelGGL(accumulate_return, g, b, 0, st, accumulated, prev_done, reward, terminated, num_envs, (float)gamma, same_step);
    if (update) {
        const int rc = update_stats(return_rms, st, accumulated, MI_F32, same_step ? nullptr : prev_done, 1, num_envs);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(finish_reward, g, b, 0, st, accumulated, prev_done, reward, terminated, truncated, return_rms->var, epsilon, num_envs, same_step,
                       out);
    W_TRY(hipGetLastError());
    return MI_OK;
}

int mi_clip_reward(int device, void *hip_stream, const double *reward, int num_envs, const double *min_reward, const double *max_reward, double *out) {
    if (!reward || !out || num_envs < 1) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "bad mi_clip_reward argument");
    W_TRY(hipSetDevice(device));
    const dim3 g((unsigned)((num_envs + kBlock - 1) / kBlock)), b(kBlock);
    hipLaunchKernelGGL(clip_reward, g, b, 0, (hipStream_t)hip_stream, reward, num_envs, min_reward ? *min_reward : 0.0, max_reward ? *max_reward : 0.0,
                       min_reward != nullptr, max_reward != nullptr, out);
    W_TRY(hipGetLastError());
    return MI_OK;
}

int64_t mi_wrapper_steps_workspace(int T, int rows, int dim) {
    StepsLayout l;
    if (!steps_layout(T, rows, dim, &l)) {
        mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_wrapper_steps_workspace: T in [1, 65535], rows >= 1, dim >= 1, rows * dim below 2^31");
        return -1;
    }
    return (int64_t)l.bytes;
}

int mi_normalize_observation_steps(mi_running_stats *s, void *hip_stream, const void *obs, int obs_dtype, int T, int num_rows, double epsilon,
                                   int update, void *out, void *workspace, int64_t workspace_bytes) {
    StepsLayout l;
    if (!s || !obs || !out || !workspace || !steps_layout(T, num_rows, s ? s->dim : 0, &l))
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "bad mi_normalize_observation_steps argument");
    if (obs_dtype != MI_F32 && obs_dtype != MI_F64) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "observations must be float32 or float64");
    if (workspace_bytes < (int64_t)l.bytes || ((uintptr_t)workspace & 7))
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_normalize_observation_steps: the workspace is smaller than mi_wrapper_steps_workspace asks for, or not 8-byte aligned");
    W_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)hip_stream;
    long stride = 0;
    const int rc = steps_statistics(s, st, obs, obs_dtype, nullptr, T, num_rows, epsilon, update, l, (char *)workspace, &stride);
    if (rc) return rc;
    const double *table = (const double *)((char *)workspace + l.table);
    const int total = num_rows * s->dim, dim = s->dim;
    const dim3 g((unsigned)((total + kBlock - 1) / kBlock), (unsigned)T), b(kBlock);
    // arithmetic in the NumPy-promoted dtype of (observation, statistics), as mi_normalize_observation
    if (obs_dtype == MI_F32 && total % 4 == 0 && (((uintptr_t)obs | (uintptr_t)out) & 15) == 0) {
        const dim3 g4((unsigned)((total / 4 + kBlock - 1) / kBlock), (unsigned)T);
        if (s->dtype == MI_F32)
            hipLaunchKernelGGL(steps_normalize_obs4<float>, g4, b, 0, st, (const float4 *)obs, table, stride, total / 4, dim, (float4 *)out);
        else
            hipLaunchKernelGGL(steps_normalize_obs4<double>, g4, b, 0, st, (const float4 *)obs, table, stride, total / 4, dim, (float4 *)out);
    } else if (obs_dtype == MI_F32 && s->dtype == MI_F32)
        hipLaunchKernelGGL((steps_normalize_obs<float, float>), g, b, 0, st, (const float *)obs, table, stride, total, dim, (float *)out);
    else if (obs_dtype == MI_F32)
        hipLaunchKernelGGL((steps_normalize_obs<float, double>), g, b, 0, st, (const float *)obs, table, stride, total, dim, (float *)out);
    else
        hipLaunchKernelGGL((steps_normalize_obs<double, double>), g, b, 0, st, (const double *)obs, table, stride, total, dim, (float *)out);
    W_TRY(hipGetLastError());
    return MI_OK;
}

int mi_normalize_reward_steps(mi_running_stats *return_rms, void *hip_stream, float *accumulated, uint8_t *prev_done, const double *reward,
                              const uint8_t *terminated, const uint8_t *truncated, int T, int num_envs, double gamma, double epsilon,
                              int same_step, int update, double *out, void *workspace, int64_t workspace_bytes) {
    StepsLayout l;
    if (!return_rms || return_rms->dim != 1 || !accumulated || !prev_done || !reward || !terminated || !truncated || !out || !workspace ||
        !steps_layout(T, num_envs, 1, &l))
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "bad mi_normalize_reward_steps argument");
    if (workspace_bytes < (int64_t)l.bytes || ((uintptr_t)workspace & 7))
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_normalize_reward_steps: the workspace is smaller than mi_wrapper_steps_workspace asks for, or not 8-byte aligned");
    W_TRY(hipSetDevice(return_rms->device));
    hipStream_t st = (hipStream_t)hip_stream;
    char *ws = (char *)workspace;
    float *traj = update ? (float *)(ws + l.traj) : nullptr;
    uint8_t *mask = update && !same_step ? (uint8_t *)(ws + l.mask) : nullptr;
    const dim3 g((unsigned)((num_envs + kBlock - 1) / kBlock)), b(kBlock);
    hipLaunchKernelGGL(steps_accumulate_return, g, b, 0, st, accumulated, prev_done, reward, terminated, truncated, T, num_envs, (float)gamma, same_step,
                       traj, mask);
    long stride = 0;
    const int rc = steps_statistics(return_rms, st, traj, MI_F32, mask, T, num_envs, epsilon, update, l, ws, &stride);
    if (rc) return rc;
    hipLaunchKernelGGL(steps_scale_reward, dim3(g.x, (unsigned)T), b, 0, st, reward, (const double *)(ws + l.table), stride, num_envs, out);
    W_TRY(hipGetLastError());
    return MI_OK;
}

}  // extern "C"
#pragma GCC visibility pop
