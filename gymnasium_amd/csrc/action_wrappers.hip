// action_wrappers.hip -- the arithmetic of the vector action wrappers ClipAction and RescaleAction over an action block that stays in HBM
// (mi_transform_actions, include/mi355env.h).
//
// What it replaces (gymnasium v1.4.0: a Python loop over the sub-environments, one NumPy call per row, then np.stack into a float32 array):
//   gymnasium/wrappers/vector/vectorize_action.py:183-213   VectorizeTransformAction.actions
//   gymnasium/wrappers/transform_action.py:118-120          ClipAction:    np.clip(action, low, high)
//   gymnasium/wrappers/utils.py:263-264                     RescaleAction: (action - intercept) / gradient
// The arithmetic runs in the dtype of the rows that came in (NumPy's promotion with the float32 bounds: float32 rows in float32, float64 rows
// in float64) and is rounded ONCE to the dtype it is stored in.  np.clip is NumPy's clip loop restated with compares and selects:
//   max(x, lo) = x > lo ? x : lo,  min(t, hi) = t < hi ? t : hi,  a NaN operand is returned as it is
// so clip(-0.0, 0.0, hi) is +0.0 and NaN stays NaN -- fminf / fmaxf would return the bound.  Subtraction and division are the correctly rounded
// IEEE operations with denormals kept (no fast-math flag, -ffp-contract=off).
//
// One elementwise pass, HBM-bound: every thread takes groups of four consecutive elements with 128-bit loads and stores (a float64 group is two
// of each), grid-stride; the elements in front of the first 16-byte boundary and behind the last whole group go one by one.  When the input's
// and the output's boundaries cannot both be met by one head (an input VIEW that starts mid-row, say) the whole block goes one by one: still
// coalesced, a quarter of the width.  The per-dimension parameters travel in the kernel's arguments and are spread into LDS once per workgroup;
// element i reads entry i % act_dim, which every thread computes once with a 64-bit remainder and then moves along by the stride's remainder.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mi355env.h"

namespace mi_internal {
int set_error(int code, const char *msg);
}

namespace {

constexpr int kBlock = 256, kMaxGrid = 2048, kGroup = 4;

struct Params {
    double p0[MI_TRANSFORM_MAX_ACT_DIM], p1[MI_TRANSFORM_MAX_ACT_DIM];
};

template <int KIND, class C>
__device__ __forceinline__ C transform(C x, C a, C b) {
    if (KIND == MI_TRANSFORM_CLIP) {
        const C t = (x != x) ? x : (x > a ? x : a);
        return (t != t) ? t : (t < b ? t : b);
    }
    return (x - a) / b;
}

template <class T>
struct Vec;
template <>
struct Vec<float> {
    float4 v;
    __device__ __forceinline__ void load(const float *p) { v = *reinterpret_cast<const float4 *>(p); }
    __device__ __forceinline__ void store(float *p) const { *reinterpret_cast<float4 *>(p) = v; }
    __device__ __forceinline__ float get(int k) const { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
    __device__ __forceinline__ void set(int k, float x) { (k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w) = x; }
};
template <>
struct Vec<double> {
    double2 a, b;
    __device__ __forceinline__ void load(const double *p) {
        a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2);
    }
    __device__ __forceinline__ void store(double *p) const { *reinterpret_cast<double2 *>(p) = a, *reinterpret_cast<double2 *>(p + 2) = b; }
    __device__ __forceinline__ double get(int k) const { return k == 0 ? a.x : k == 1 ? a.y : k == 2 ? b.x : b.y; }
    __device__ __forceinline__ void set(int k, double x) { (k == 0 ? a.x : k == 1 ? a.y : k == 2 ? b.x : b.y) = x; }
};

// in / out: [elements]; [0, head) and [head + 4 * groups, elements) go one by one, the `groups` groups in between as vectors (in + head and
// out + head are 16-byte aligned whenever groups > 0: the launcher's business).
template <int KIND, class In, class Out>
__global__ __launch_bounds__(kBlock) void transform_actions_kernel(const In *__restrict__ in, Out *__restrict__ out, int64_t elements, int64_t head,
                                                                  int64_t groups, int act_dim, Params p) {
    __shared__ In s0[MI_TRANSFORM_MAX_ACT_DIM], s1[MI_TRANSFORM_MAX_ACT_DIM];
    if ((int)threadIdx.x < act_dim) s0[threadIdx.x] = (In)p.p0[threadIdx.x], s1[threadIdx.x] = (In)p.p1[threadIdx.x];
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, threads = (int64_t)gridDim.x * kBlock;

    {  // the groups: thread t takes groups t, t + threads, ...
        const int step = (int)((threads * kGroup) % act_dim);
        int j = (int)((head + tid * kGroup) % act_dim);
        for (int64_t g = tid; g < groups; g += threads) {
            const int64_t e = head + g * kGroup;
            Vec<In> x;
            Vec<Out> y;
            x.load(in + e);
            int jj = j;
#pragma unroll
            for (int k = 0; k < kGroup; k++) {
                y.set(k, (Out)transform<KIND, In>(x.get(k), s0[jj], s1[jj]));
                jj = jj + 1 == act_dim ? 0 : jj + 1;
            }
            y.store(out + e);
            j += step;
            j = j >= act_dim ? j - act_dim : j;
        }
    }
    {  // the head and the tail as one sequence of `rest` single elements
        const int64_t body = groups * kGroup, rest = elements - body;
        const int step = (int)(threads % act_dim);
        int64_t r = tid;
        if (r < rest) {
            int64_t e = r < head ? r : r + body;
            int j = (int)(e % act_dim);
            for (;;) {
                out[e] = (Out)transform<KIND, In>(in[e], s0[j], s1[j]);
                r += threads;
                if (r >= rest) break;
                const int64_t e2 = r < head ? r : r + body;
                // e2 - e = threads, or threads + body where the sequence crosses from the head to the tail (at most once per thread)
                j = e2 - e == threads ? j + step : (int)(e2 % act_dim);
                j = j >= act_dim ? j - act_dim : j;
                e = e2;
            }
        }
    }
}

template <int KIND, class In, class Out>
hipError_t launch(hipStream_t st, const void *in, void *out, int64_t elements, int act_dim, const Params &p) {
    // a head h < 4 with (in + h) and (out + h) on 16-byte boundaries exists iff the two pointers ask for the same h modulo the coarser of
    // their granularities (4 float32 / 2 float64 elements per 16 bytes)
    constexpr int64_t gin = 16 / (int64_t)sizeof(In), gout = 16 / (int64_t)sizeof(Out);
    const int64_t hin = (gin - (int64_t)(((uintptr_t)in / sizeof(In)) % gin)) % gin;
    const int64_t hout = (gout - (int64_t)(((uintptr_t)out / sizeof(Out)) % gout)) % gout;
    const int64_t h = gin >= gout ? hin : hout;
    int64_t head = elements, groups = 0;
    if (h % gin == hin && h % gout == hout && elements >= h + kGroup) head = h, groups = (elements - h) / kGroup;
    const int64_t work = groups > 0 ? groups : elements;
    int64_t blocks = (work + kBlock - 1) / kBlock;
    if (blocks > kMaxGrid) blocks = kMaxGrid;
    hipLaunchKernelGGL((transform_actions_kernel<KIND, In, Out>), dim3((unsigned)blocks), dim3(kBlock), 0, st, (const In *)in, (Out *)out, elements, head,
                       groups, act_dim, p);
    return hipGetLastError();
}

template <int KIND>
hipError_t launch_kind(hipStream_t st, const void *in, int in_dtype, void *out, int out_dtype, int64_t elements, int act_dim, const Params &p) {
    if (in_dtype == MI_F32) return launch<KIND, float, float>(st, in, out, elements, act_dim, p);
    if (out_dtype == MI_F32) return launch<KIND, double, float>(st, in, out, elements, act_dim, p);
    return launch<KIND, double, double>(st, in, out, elements, act_dim, p);
}

}  // namespace

#pragma GCC visibility push(default)

int mi_transform_actions(int device, void *hip_stream, const void *in, int in_dtype, void *out, int out_dtype, int64_t elements, int act_dim, int kind,
                         const double *p0, const double *p1) {
    if (!in || !out || !p0 || !p1 || elements < 0 || act_dim < 1 || act_dim > MI_TRANSFORM_MAX_ACT_DIM)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "bad mi_transform_actions argument (act_dim in [1, 32])");
    if (kind != MI_TRANSFORM_CLIP && kind != MI_TRANSFORM_AFFINE_INVERSE)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_transform_actions: kind is MI_TRANSFORM_CLIP or MI_TRANSFORM_AFFINE_INVERSE");
    const bool dtypes_ok = (in_dtype == MI_F32 && out_dtype == MI_F32) || (in_dtype == MI_F64 && (out_dtype == MI_F32 || out_dtype == MI_F64));
    if (!dtypes_ok)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_transform_actions: float32 -> float32, float64 -> float32 or float64 -> float64");
    if ((uintptr_t)in % (in_dtype == MI_F32 ? 4 : 8) || (uintptr_t)out % (out_dtype == MI_F32 ? 4 : 8))
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_transform_actions: a pointer is not aligned to its element type");
    if (elements == 0) return MI_OK;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) {
        Params p;
        for (int k = 0; k < MI_TRANSFORM_MAX_ACT_DIM; k++) p.p0[k] = k < act_dim ? p0[k] : 0.0, p.p1[k] = k < act_dim ? p1[k] : 1.0;
        const hipStream_t st = (hipStream_t)hip_stream;
        e = kind == MI_TRANSFORM_CLIP ? launch_kind<MI_TRANSFORM_CLIP>(st, in, in_dtype, out, out_dtype, elements, act_dim, p)
                                      : launch_kind<MI_TRANSFORM_AFFINE_INVERSE>(st, in, in_dtype, out, out_dtype, elements, act_dim, p);
    }
    if (e != hipSuccess) {
        char buf[300];
        snprintf(buf, sizeof buf, "mi_transform_actions failed: %s", hipGetErrorString(e));
        return mi_internal::set_error(MI_ERR_HIP, buf);
    }
    return MI_OK;
}

#pragma GCC visibility pop
