// observation_wrappers.hip -- the stateless observation transforms of the vector wrappers RescaleObservation, DtypeObservation and
// FlattenObservation over an observation block that stays in HBM (mi_transform_observations, mi_one_hot; include/mi355env.h).
//
// What it replaces (gymnasium v1.4.0: a Python loop over the sub-environments, one NumPy call per row, then concatenate into a new array):
//   gymnasium/wrappers/vector/vectorize_observation.py:234-257   VectorizeTransformObservation.observations
//   gymnasium/wrappers/utils.py:260-261                          RescaleObservation: gradient * obs + intercept
//   gymnasium/wrappers/transform_observation.py:633              DtypeObservation:   dtype(obs)
//   gymnasium/spaces/utils.py:167-195                            FlattenObservation: one-hot rows of Discrete / Tuple-of-Discrete spaces
//
// MI_OBS_AFFINE is NumPy's two ufuncs: the product rounded once, then the sum rounded once, in the dtype of the box (float32 or float64) --
// never an FMA (this unit is built with -ffp-contract=off like the rest, and the two operations are written as two statements).  Components
// with gradient 1 and intercept 0 go through the same arithmetic, so -0.0 comes out as +0.0 and NaN / +-inf propagate as IEEE says.
// MI_OBS_CAST is NumPy's C cast: float -> float rounded ONCE to nearest-even (float64 -> float16 directly, see f64_to_f16_bits below: the
// conversion is written out on the bits, because a route through float32 rounds twice), integer -> float rounded once, integer -> integer
// keeps the low bits, float -> integer truncates (NaN and out-of-range values: undefined, as in C and NumPy).
//
// Both are one elementwise pass, HBM-bound, laid out like action_wrappers.hip: every thread takes groups of four consecutive elements --
// 128-bit loads / stores on the wider of the two types (an 8-byte type: two of them), one narrower access on the other side -- grid-stride;
// the elements in front of the first boundary and behind the last whole group go one by one.  When the input's and the output's boundaries
// cannot both be met by one head (an input VIEW that starts mid-row, say) the whole block goes one by one: still coalesced, a quarter of
// the width.  gradient / intercept are DEVICE arrays of obs_dim entries (Humanoid-v5 has 348: too many for kernel arguments), staged into
// LDS once per workgroup; element i reads entry i % obs_dim, which every thread computes once with a 64-bit remainder and then moves along
// by the stride's remainder.
//
// mi_one_hot is a pure write stream: thread t produces the two adjacent int64 at flat positions head + 2t, head + 2t + 1 of out[rows][W]
// with one 128-bit store (head = 1 when `out` sits 8 bytes off a 16-byte boundary), so rows of an odd width W -- Blackjack's 45 columns,
// 360 bytes: every other row starts 8 bytes off -- need no per-row treatment; (row, column) of a position are computed once and moved along
// by the stride's quotient and remainder.  A state outside its segment matches no column: the segment stays zero.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mi355env.h"

namespace mi_internal {
int set_error(int code, const char *msg);
}

namespace {

constexpr int kBlock = 256, kMaxGrid = 2048, kGroup = 4;

// float64 -> float16, round to nearest even, ONE rounding (NumPy's npy_double_to_half); the bits of the result.
__host__ __device__ inline uint16_t f64_to_f16_bits(uint64_t b) {
    const uint16_t sign = (uint16_t)((b >> 48) & 0x8000u);
    const int exp = (int)((b >> 52) & 0x7ff);
    const uint64_t man = b & 0xfffffffffffffull;
    if (exp == 0x7ff) return (uint16_t)(sign | 0x7c00u | (man ? 0x200u | (uint16_t)(man >> 42) : 0u));  // inf; NaN (quiet, payload's top bits)
    const int e = exp - 1023 + 15;  // the float16 exponent field of a normal result
    if (e >= 31) return (uint16_t)(sign | 0x7c00u);  // 2^16 and above: inf (65520 <= |x| < 65536 gets there by the carry below)
    if (e < -10) return sign;  // below 2^-25, half of the smallest denormal: zero (float64 denormals included)
    uint64_t m = man;
    int shift = 42;
    uint32_t h = (uint32_t)e << 10;
    if (e <= 0) m |= 1ull << 52, shift = 43 - e, h = 0;  // a float16 denormal: the leading one joins the digits, 43 <= shift <= 53
    const uint64_t kept = m >> shift, rest = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    h += (uint32_t)kept;
    if (rest > half || (rest == half && (kept & 1))) h++;  // a carry moves into the exponent, up to inf: what rounding asks for
    return (uint16_t)(sign | h);
}

template <class Out, class In>
__device__ __forceinline__ Out cast(In x) {
    return (Out)x;
}
template <>
__device__ __forceinline__ _Float16 cast<_Float16, double>(double x) {
    const uint16_t h = f64_to_f16_bits((uint64_t)__double_as_longlong(x));
    _Float16 r;
    __builtin_memcpy(&r, &h, 2);
    return r;
}
template <>
__device__ __forceinline__ _Float16 cast<_Float16, int64_t>(int64_t x) {
    return (_Float16)(float)x;  // NumPy's own route; exact below 2^24 and float16 is inf from 65520 on, so nothing rounds twice
}

// four consecutive elements, accessed as one 16-byte vector (two for an 8-byte type) or one narrower one
template <class T>
struct alignas(sizeof(T) * kGroup > 16 ? 16 : sizeof(T) * kGroup) Pack {
    T v[kGroup];
};

template <int KIND, class In, class Out>
__device__ __forceinline__ Out apply(In x, In g, In c) {
    if (KIND == MI_OBS_AFFINE) {
        const In p = g * x;  // rounded ...
        return (Out)(p + c);  // ... and rounded again: no FMA (-ffp-contract=off)
    }
    return cast<Out, In>(x);
}

// in / out: [elements]; [0, head) and [head + 4 * groups, elements) go one by one, the `groups` groups in between as vectors (in + head and
// out + head are aligned for their Pack whenever groups > 0: the launcher's business).
template <int KIND, class In, class Out>
__global__ __launch_bounds__(kBlock) void transform_observations_kernel(const In *__restrict__ in, Out *__restrict__ out, int64_t elements, int64_t head,
                                                                       int64_t groups, int obs_dim, const In *__restrict__ gradient,
                                                                       const In *__restrict__ intercept) {
    __shared__ In sg[KIND == MI_OBS_AFFINE ? MI_OBS_MAX_DIM : 1], sc[KIND == MI_OBS_AFFINE ? MI_OBS_MAX_DIM : 1];
    if (KIND == MI_OBS_AFFINE) {
        for (int k = threadIdx.x; k < obs_dim; k += kBlock) sg[k] = gradient[k], sc[k] = intercept[k];
        __syncthreads();
    }
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, threads = (int64_t)gridDim.x * kBlock;

    {  // the groups: thread t takes groups t, t + threads, ...
        const int step = KIND == MI_OBS_AFFINE ? (int)((threads * kGroup) % obs_dim) : 0;
        int j = KIND == MI_OBS_AFFINE ? (int)((head + tid * kGroup) % obs_dim) : 0;
        for (int64_t g = tid; g < groups; g += threads) {
            const int64_t e = head + g * kGroup;
            const Pack<In> x = *reinterpret_cast<const Pack<In> *>(in + e);
            Pack<Out> y;
            int jj = j;
#pragma unroll
            for (int k = 0; k < kGroup; k++) {
                y.v[k] = KIND == MI_OBS_AFFINE ? apply<KIND, In, Out>(x.v[k], sg[jj], sc[jj]) : apply<KIND, In, Out>(x.v[k], In(0), In(0));
                if (KIND == MI_OBS_AFFINE) jj = jj + 1 == obs_dim ? 0 : jj + 1;
            }
            *reinterpret_cast<Pack<Out> *>(out + e) = y;
            j += step;
            j = j >= obs_dim ? j - obs_dim : j;
        }
    }
    {  // the head and the tail as one sequence of `rest` single elements
        const int64_t body = groups * kGroup, rest = elements - body;
        const int step = KIND == MI_OBS_AFFINE ? (int)(threads % obs_dim) : 0;
        int64_t r = tid;
        if (r < rest) {
            int64_t e = r < head ? r : r + body;
            int j = KIND == MI_OBS_AFFINE ? (int)(e % obs_dim) : 0;
            for (;;) {
                out[e] = KIND == MI_OBS_AFFINE ? apply<KIND, In, Out>(in[e], sg[j], sc[j]) : apply<KIND, In, Out>(in[e], In(0), In(0));
                r += threads;
                if (r >= rest) break;
                const int64_t e2 = r < head ? r : r + body;
                if (KIND == MI_OBS_AFFINE) {
                    // e2 - e = threads, or threads + body where the sequence crosses from the head to the tail (at most once per thread)
                    j = e2 - e == threads ? j + step : (int)(e2 % obs_dim);
                    j = j >= obs_dim ? j - obs_dim : j;
                }
                e = e2;
            }
        }
    }
}

template <int KIND, class In, class Out>
hipError_t launch(hipStream_t st, const void *in, void *out, int64_t elements, int obs_dim, const void *gradient, const void *intercept) {
    // a head h < 4 with (in + h) and (out + h) on their Pack's boundaries exists iff the two pointers ask for the same h modulo the coarser
    // of their granularities (elements per boundary: 4 for the types of up to 4 bytes, 2 for the 8-byte ones)
    constexpr int64_t gin = (int64_t)(alignof(Pack<In>) / sizeof(In)), gout = (int64_t)(alignof(Pack<Out>) / sizeof(Out));
    const int64_t hin = (gin - (int64_t)(((uintptr_t)in / sizeof(In)) % gin)) % gin;
    const int64_t hout = (gout - (int64_t)(((uintptr_t)out / sizeof(Out)) % gout)) % gout;
    const int64_t h = gin >= gout ? hin : hout;
    int64_t head = elements, groups = 0;
    if (h % gin == hin && h % gout == hout && elements >= h + kGroup) head = h, groups = (elements - h) / kGroup;
    const int64_t work = groups > 0 ? groups : elements;
    int64_t blocks = (work + kBlock - 1) / kBlock;
    if (blocks > kMaxGrid) blocks = kMaxGrid;
    hipLaunchKernelGGL((transform_observations_kernel<KIND, In, Out>), dim3((unsigned)blocks), dim3(kBlock), 0, st, (const In *)in, (Out *)out, elements,
                       head, groups, obs_dim, (const In *)gradient, (const In *)intercept);
    return hipGetLastError();
}

template <class In>
hipError_t launch_cast(hipStream_t st, const void *in, void *out, int out_dtype, int64_t elements) {
    switch (out_dtype) {
    case MI_F16: return launch<MI_OBS_CAST, In, _Float16>(st, in, out, elements, 1, nullptr, nullptr);
    case MI_F32: return launch<MI_OBS_CAST, In, float>(st, in, out, elements, 1, nullptr, nullptr);
    case MI_F64: return launch<MI_OBS_CAST, In, double>(st, in, out, elements, 1, nullptr, nullptr);
    case MI_I32: return launch<MI_OBS_CAST, In, int32_t>(st, in, out, elements, 1, nullptr, nullptr);
    case MI_I64: return launch<MI_OBS_CAST, In, int64_t>(st, in, out, elements, 1, nullptr, nullptr);
    default: return launch<MI_OBS_CAST, In, uint8_t>(st, in, out, elements, 1, nullptr, nullptr);  // MI_U8
    }
}

int dtype_size(int dtype) {
    switch (dtype) {
    case MI_U8: return 1;
    case MI_F16: return 2;
    case MI_F32: case MI_I32: return 4;
    case MI_F64: case MI_I64: return 8;
    default: return 0;
    }
}

struct OneHotParts {
    const int64_t *col[MI_ONE_HOT_MAX_PARTS];
    int64_t start[MI_ONE_HOT_MAX_PARTS];
    int32_t offset[MI_ONE_HOT_MAX_PARTS + 1];  // first column of segment k (W for the unused ones); the last entry: the row width W
    int32_t num;
};

// the value at (row, column c) of the one-hot block (the segment is picked with selects: the parts live in the kernel's arguments)
__device__ __forceinline__ int64_t one_hot_at(const OneHotParts &p, int64_t row, int c) {
    const int64_t *col = p.col[0];
    int64_t start = p.start[0];
    int offset = 0;
#pragma unroll
    for (int q = 1; q < MI_ONE_HOT_MAX_PARTS; q++) {
        const bool later = q < p.num && c >= p.offset[q];
        col = later ? p.col[q] : col, start = later ? p.start[q] : start, offset = later ? p.offset[q] : offset;
    }
    return col[row] - start == (int64_t)(c - offset) ? 1 : 0;
}

// out: [rows][W] as total = rows * W flat int64; [0, head) and the last element of an odd remainder go alone, the `pairs` pairs in between as
// 128-bit stores (out + head is 16-byte aligned whenever pairs > 0)
__global__ __launch_bounds__(kBlock) void one_hot_kernel(OneHotParts p, int64_t total, int64_t head, int64_t pairs, int64_t *__restrict__ out) {
    const int W = p.offset[MI_ONE_HOT_MAX_PARTS];
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, threads = (int64_t)gridDim.x * kBlock;
    const int64_t stride = threads * 2, row_step = stride / W;
    const int col_step = (int)(stride % W);
    const int64_t first = head + tid * 2;
    int64_t row = first / W;
    int c = (int)(first % W);
    for (int64_t g = tid; g < pairs; g += threads) {
        const int64_t e = head + g * 2;
        const bool wraps = c + 1 == W;  // the pair's second element opens the next row
        longlong2 y;
        y.x = one_hot_at(p, row, c);
        y.y = one_hot_at(p, wraps ? row + 1 : row, wraps ? 0 : c + 1);
        *reinterpret_cast<longlong2 *>(out + e) = y;
        row += row_step, c += col_step;
        if (c >= W) c -= W, row++;
    }
    if (tid < 2) {  // the element in front of the first boundary (thread 0) and the one behind the last pair (thread 1)
        const int64_t e = tid == 0 ? 0 : head + pairs * 2;
        if ((tid == 0 && head > 0) || (tid == 1 && e < total)) out[e] = one_hot_at(p, e / W, (int)(e % W));
    }
}

int hip_failure(const char *what, hipError_t e) {
    char buf[300];
    snprintf(buf, sizeof buf, "%s failed: %s", what, hipGetErrorString(e));
    return mi_internal::set_error(MI_ERR_HIP, buf);
}

}  // namespace

#pragma GCC visibility push(default)

int mi_transform_observations(int device, void *hip_stream, const void *in, int in_dtype, void *out, int out_dtype, int64_t elements, int obs_dim, int kind,
                              const void *gradient, const void *intercept) {
    if (!in || !out || elements < 0) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "bad mi_transform_observations argument");
    if (kind != MI_OBS_AFFINE && kind != MI_OBS_CAST)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_transform_observations: kind is MI_OBS_AFFINE or MI_OBS_CAST");
    if (kind == MI_OBS_AFFINE) {
        if (obs_dim < 1 || obs_dim > MI_OBS_MAX_DIM || !gradient || !intercept)
            return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_transform_observations: MI_OBS_AFFINE takes obs_dim in [1, 1024] and device arrays gradient, intercept");
        if ((in_dtype != MI_F32 && in_dtype != MI_F64) || out_dtype != in_dtype)
            return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_transform_observations: MI_OBS_AFFINE is float32 -> float32 or float64 -> float64");
    } else {
        if (in_dtype != MI_F32 && in_dtype != MI_F64 && in_dtype != MI_I64)
            return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_transform_observations: MI_OBS_CAST reads float32, float64 or int64");
        if (out_dtype != MI_F16 && out_dtype != MI_F32 && out_dtype != MI_F64 && out_dtype != MI_I32 && out_dtype != MI_I64 && out_dtype != MI_U8)
            return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_transform_observations: MI_OBS_CAST writes float16, float32, float64, int32, int64 or uint8");
    }
    if ((uintptr_t)in % dtype_size(in_dtype) || (uintptr_t)out % dtype_size(out_dtype) ||
        (kind == MI_OBS_AFFINE && ((uintptr_t)gradient % dtype_size(in_dtype) || (uintptr_t)intercept % dtype_size(in_dtype))))
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_transform_observations: a pointer is not aligned to its element type");
    if (elements == 0) return MI_OK;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) {
        const hipStream_t st = (hipStream_t)hip_stream;
        if (kind == MI_OBS_AFFINE)
            e = in_dtype == MI_F32 ? launch<MI_OBS_AFFINE, float, float>(st, in, out, elements, obs_dim, gradient, intercept)
                                   : launch<MI_OBS_AFFINE, double, double>(st, in, out, elements, obs_dim, gradient, intercept);
        else
            e = in_dtype == MI_F32   ? launch_cast<float>(st, in, out, out_dtype, elements)
                : in_dtype == MI_F64 ? launch_cast<double>(st, in, out, out_dtype, elements)
                                     : launch_cast<int64_t>(st, in, out, out_dtype, elements);
    }
    return e == hipSuccess ? MI_OK : hip_failure("mi_transform_observations", e);
}

int mi_one_hot(int device, void *hip_stream, const int64_t *const *parts, int num_parts, const int64_t *start, const int32_t *width, int64_t rows,
               int64_t *out) {
    if (!parts || !start || !width || !out || rows < 0 || num_parts < 1 || num_parts > MI_ONE_HOT_MAX_PARTS)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "bad mi_one_hot argument (num_parts in [1, 4])");
    OneHotParts p;
    int64_t W = 0;
    for (int k = 0; k < MI_ONE_HOT_MAX_PARTS; k++) {
        const bool used = k < num_parts;
        if (used && (!parts[k] || (uintptr_t)parts[k] % 8 || width[k] < 1))
            return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_one_hot: every part is an 8-byte aligned device array and every width is positive");
        p.col[k] = used ? parts[k] : parts[0], p.start[k] = used ? start[k] : 0, p.offset[k] = (int32_t)W;
        W += used ? width[k] : 0;
        if (W >= (1 << 30)) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_one_hot: the widths add up to 2^30 or more");
    }
    p.offset[MI_ONE_HOT_MAX_PARTS] = (int32_t)W, p.num = num_parts;
    if ((uintptr_t)out % 8) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_one_hot: out is not aligned to int64");
    if (rows > INT64_MAX / W) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_one_hot: rows * width overflows");
    const int64_t total = rows * W;
    if (total == 0) return MI_OK;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) {
        const int64_t head = ((uintptr_t)out % 16) ? 1 : 0, pairs = (total - head) / 2;
        int64_t blocks = ((pairs > 0 ? pairs : 1) + kBlock - 1) / kBlock;
        if (blocks > kMaxGrid) blocks = kMaxGrid;
        hipLaunchKernelGGL(one_hot_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)hip_stream, p, total, head, pairs, out);
        e = hipGetLastError();
    }
    return e == hipSuccess ? MI_OK : hip_failure("mi_one_hot", e);
}

#pragma GCC visibility pop
