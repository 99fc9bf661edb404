// discretize.hip -- gymnasium.wrappers.DiscretizeObservation / DiscretizeAction around every sub-environment, over an observation / index block that
// stays in HBM (mi_discretize_observations, mi_discretize_actions; include/mi355env.h).
//
// What it replaces (gymnasium v1.4.0; the reference has no vector form, so SyncVectorEnv runs these per sub-environment in Python):
//   gymnasium/wrappers/transform_observation.py:863-877   DiscretizeObservation.observation: np.clip, one np.digitize per dimension, the mixed-radix sum
//   gymnasium/wrappers/transform_action.py:317-345        DiscretizeAction.action: _unflatten_index (floor % and //), clamp, bin_centers look-up
//
// The device does NO floating-point arithmetic beyond compare and select: the clip bounds (low, high - 1e-8 in the Box's dtype), the concatenated
// interior edges and the concatenated bin centres are the reference's own NumPy expressions, computed on the host and uploaded once.
//
// mi_discretize_observations.  One workgroup takes tiles of kBlock rows.  The tile's nrows * obs_dim values are ONE contiguous piece of the block, read
// element by element -- lane l of a wavefront at base + l, whole cache lines, never a stride of the row size.  Every element is clipped and binned on its
// own (its dimension is its position modulo obs_dim, moved along by the stride's remainder): the bin is the number of edges e with !(x < e), found by an
// upper-bound bisection of the dimension's edges in LDS (the table is read log2(bins) times per element; MI_DISCRETIZE_MAX_TABLE entries fit, a longer
// table is refused; the bisection is branch-free, its trip count depends on bins alone).  np.digitize(right=False) on non-decreasing edges counts exactly those edges -- duplicates (low == high) included -- and NaN, which
// is below no edge, counts them all: the last bin.  Multidiscrete: the bin is stored at the element's own position, a coalesced int64 stream.  Flat: it
// goes to LDS (uint16: bins <= MI_DISCRETIZE_MAX_TABLE + 1), and after a barrier thread r folds row r's obs_dim digits, idx = idx * bins[d] + i_d, and
// stores one int64, coalesced again.  The LDS rows are obs_dim uint16 apart: lanes r, r + 1 read dwords (r * obs_dim) / 2 apart, a conflict of at most
// obs_dim / 2 ways on reads that are a tenth of the work.
//
// mi_discretize_actions.  One thread per OUTPUT element, grid-stride, (row, dimension) moved along by the stride's quotient and remainder, so stores are
// coalesced and the act_dim lanes of a row read the same index (one broadcast load).  Flat: digit d of index f is floor_mod(floor_div(f, s_d), bins[d])
// with s_d = bins[d + 1] * ... * bins[A - 1] -- nested floor divisions by positive numbers equal one floor division by their product, so this IS
// _unflatten_index's loop, last dimension first, for negative f as well (Python's % and //).  64-bit division is a software routine on this hardware
// (~100 instructions), so an index with 0 <= f < 2^31 under a prod(bins) < 2^31 takes two 32-bit unsigned divisions instead; everything else -- a
// negative index, one at or above 2^31, a wider product -- takes the 64-bit path.  Multidiscrete: clamp to [0, bins[d] - 1].  The centre comes from the
// concatenated table in LDS (same cap).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mi355env.h"

namespace mi_internal {
int set_error(int code, const char *msg);
}

namespace {

constexpr int kBlock = 256, kMaxGrid = 2048;

struct ObsDims {
    int32_t bins[MI_DISCRETIZE_MAX_DIM];
    int32_t offset[MI_DISCRETIZE_MAX_DIM + 1];  // first edge of dimension d in the concatenated table; the last entry: its length
    int32_t narrow;                             // prod(bins) < 2^31
};

struct ActDims {
    int64_t stride[MI_DISCRETIZE_MAX_DIM];  // bins[d + 1] * ... * bins[A - 1]
    int32_t bins[MI_DISCRETIZE_MAX_DIM];
    int32_t offset[MI_DISCRETIZE_MAX_DIM + 1];  // first centre of dimension d; the last entry: the table's length
    int32_t narrow;                             // prod(bins) < 2^31: indices in [0, 2^31) may take the 32-bit path
};

// the number of edges e in edges[0, n) with !(x < e): an upper bound by bisection (NaN: n).  Branch-free: the trip count depends on n alone, so the
// lanes of one dimension run in step, and a trip is one LDS read, one compare, one select.
template <class T>
__device__ __forceinline__ int count_not_below(const T *edges, int n, T x) {
    int base = 0;  // the count lies in [base, base + len]
    for (int len = n; len > 1;) {
        const int half = len >> 1;
        base = !(x < edges[base + half - 1]) ? base + half : base;
        len -= half;
    }
    return n > 0 && !(x < edges[base]) ? base + 1 : base;
}

template <class T>
struct Bounds {
    T lo, hi;
};

template <class T, bool MULTI>
__global__ __launch_bounds__(kBlock) void discretize_observations_kernel(const T *__restrict__ in, int64_t rows, int obs_dim, ObsDims dims,
                                                                        const T *__restrict__ lo, const T *__restrict__ hi_clip,
                                                                        const T *__restrict__ edges, int64_t *__restrict__ out) {
    __shared__ T s_edges[MI_DISCRETIZE_MAX_TABLE];
    __shared__ Bounds<T> s_clip[MI_DISCRETIZE_MAX_DIM];  // (one LDS read per element for the pair)
    __shared__ uint16_t s_bin[MULTI ? 1 : kBlock * MI_DISCRETIZE_MAX_DIM];
    __shared__ int2 s_dim[MI_DISCRETIZE_MAX_DIM];  // {first edge, bins} (indexed per lane: kernel arguments would go through scratch)
    const int tid = (int)threadIdx.x, total_edges = dims.offset[MI_DISCRETIZE_MAX_DIM];
    for (int k = tid; k < total_edges; k += kBlock) s_edges[k] = edges[k];
    if (tid < obs_dim) s_clip[tid].lo = lo[tid], s_clip[tid].hi = hi_clip[tid];
    if (tid < MI_DISCRETIZE_MAX_DIM) s_dim[tid] = make_int2(dims.offset[tid], dims.bins[tid]);
    __syncthreads();
    const int64_t tiles = (rows + kBlock - 1) / kBlock;
    const bool narrow = dims.narrow != 0;
    const int first_dim = tid % obs_dim, dim_step = kBlock % obs_dim;  // (a tile starts at a row, so its element tid is dimension tid % obs_dim)
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * kBlock;
        const int nrows = (int)(rows - row0 < kBlock ? rows - row0 : kBlock), nelem = nrows * obs_dim;
        const T *src = in + row0 * obs_dim;
        int d = first_dim;
        for (int e = tid; e < nelem; e += kBlock) {
            T x = src[e];
            const Bounds<T> clip = s_clip[d];
            const int2 dim = s_dim[d];
            x = x < clip.lo ? clip.lo : x;  // np.clip as maximum then minimum; NaN passes both
            x = x > clip.hi ? clip.hi : x;
            const int bin = count_not_below(s_edges + dim.x, dim.y - 1, x);
            if (MULTI)
                out[row0 * obs_dim + e] = bin;
            else
                s_bin[e] = (uint16_t)bin;
            d += dim_step;
            d = d >= obs_dim ? d - obs_dim : d;
        }
        if (!MULTI) {
            __syncthreads();
            if (tid < nrows) {
                int64_t idx = 0;
                if (narrow) {  // prod(bins) < 2^31: the same sum in 32 bits
                    uint32_t small = 0;
                    for (int k = 0; k < obs_dim; k++) small = small * (uint32_t)s_dim[k].y + s_bin[tid * obs_dim + k];
                    idx = small;
                } else {
                    for (int k = 0; k < obs_dim; k++) idx = idx * s_dim[k].y + s_bin[tid * obs_dim + k];
                }
                out[row0 + tid] = idx;
            }
            __syncthreads();  // (the next tile overwrites s_bin)
        }
    }
}

// Python's (f // s) % b for s, b > 0
__device__ __forceinline__ int digit_wide(int64_t f, int64_t s, int32_t b) {
    int64_t q = f / s;
    q = (f % s) < 0 ? q - 1 : q;
    const int64_t r = q % b;
    return (int)(r < 0 ? r + b : r);
}

template <class I, class T, bool MULTI>
__global__ __launch_bounds__(kBlock) void discretize_actions_kernel(const I *__restrict__ in, int64_t rows, int act_dim, ActDims dims,
                                                                   const T *__restrict__ centres, T *__restrict__ out) {
    __shared__ T s_centres[MI_DISCRETIZE_MAX_TABLE];
    __shared__ int64_t s_stride[MI_DISCRETIZE_MAX_DIM];
    __shared__ int32_t s_bins[MI_DISCRETIZE_MAX_DIM], s_offset[MI_DISCRETIZE_MAX_DIM];  // (indexed per lane: kernel arguments would go through scratch)
    const int total = dims.offset[MI_DISCRETIZE_MAX_DIM];
    for (int k = (int)threadIdx.x; k < total; k += kBlock) s_centres[k] = centres[k];
    if (threadIdx.x < MI_DISCRETIZE_MAX_DIM)
        s_stride[threadIdx.x] = dims.stride[threadIdx.x], s_bins[threadIdx.x] = dims.bins[threadIdx.x], s_offset[threadIdx.x] = dims.offset[threadIdx.x];
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, threads = (int64_t)gridDim.x * kBlock, elements = rows * act_dim;
    const int64_t row_step = threads / act_dim;
    const int dim_step = (int)(threads % act_dim);
    int64_t row = tid / act_dim;
    int d = (int)(tid % act_dim);
    for (int64_t e = tid; e < elements; e += threads) {
        int digit;
        if (MULTI) {
            const int64_t i = (int64_t)in[e];
            digit = (int)(i < 0 ? 0 : i > s_bins[d] - 1 ? s_bins[d] - 1 : i);  // min(max(idx, 0), bins - 1)
        } else {
            const int64_t f = (int64_t)in[row];
            if (dims.narrow && (uint64_t)f < (1ull << 31))
                digit = (int)(((uint32_t)f / (uint32_t)s_stride[d]) % (uint32_t)s_bins[d]);
            else
                digit = digit_wide(f, s_stride[d], s_bins[d]);
        }
        out[e] = s_centres[s_offset[d] + digit];
        row += row_step, d += dim_step;
        if (d >= act_dim) d -= act_dim, row++;
    }
}

int hip_failure(const char *what, hipError_t e) {
    char buf[300];
    snprintf(buf, sizeof buf, "%s failed: %s", what, hipGetErrorString(e));
    return mi_internal::set_error(MI_ERR_HIP, buf);
}

int grid_for(int64_t work) {
    int64_t blocks = (work + kBlock - 1) / kBlock;
    return (int)(blocks > kMaxGrid ? kMaxGrid : blocks);
}

template <class T>
hipError_t launch_observations(hipStream_t st, const void *in, int64_t rows, int obs_dim, const ObsDims &dims, const void *lo, const void *hi_clip,
                               const void *edges, int multidiscrete, int64_t *out) {
    const dim3 grid((unsigned)grid_for(rows)), block(kBlock);  // one tile of kBlock rows per workgroup and trip
    if (multidiscrete)
        hipLaunchKernelGGL((discretize_observations_kernel<T, true>), grid, block, 0, st, (const T *)in, rows, obs_dim, dims, (const T *)lo,
                           (const T *)hi_clip, (const T *)edges, out);
    else
        hipLaunchKernelGGL((discretize_observations_kernel<T, false>), grid, block, 0, st, (const T *)in, rows, obs_dim, dims, (const T *)lo,
                           (const T *)hi_clip, (const T *)edges, out);
    return hipGetLastError();
}

template <class I, class T>
hipError_t launch_actions(hipStream_t st, const void *in, int64_t rows, int act_dim, const ActDims &dims, const void *centres, int multidiscrete,
                          void *out) {
    const dim3 grid((unsigned)grid_for(rows * act_dim)), block(kBlock);
    if (multidiscrete)
        hipLaunchKernelGGL((discretize_actions_kernel<I, T, true>), grid, block, 0, st, (const I *)in, rows, act_dim, dims, (const T *)centres, (T *)out);
    else
        hipLaunchKernelGGL((discretize_actions_kernel<I, T, false>), grid, block, 0, st, (const I *)in, rows, act_dim, dims, (const T *)centres, (T *)out);
    return hipGetLastError();
}

}  // namespace

#pragma GCC visibility push(default)

int mi_discretize_observations(int device, void *hip_stream, const void *in, int in_dtype, int64_t rows, int obs_dim, const int32_t *bins,
                               const void *lo, const void *hi_clip, const void *edges, int multidiscrete, int64_t *out) {
    if (!in || !out || !bins || !lo || !hi_clip || rows < 0)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "bad mi_discretize_observations argument");
    if (in_dtype != MI_F32 && in_dtype != MI_F64)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_observations reads float32 or float64 observations");
    if (obs_dim < 1 || obs_dim > MI_DISCRETIZE_MAX_DIM)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_observations: obs_dim in [1, 32]");
    ObsDims dims;
    int64_t table = 0, prod = 1;
    for (int d = 0; d < MI_DISCRETIZE_MAX_DIM; d++) {
        const int32_t b = d < obs_dim ? bins[d] : 1;
        if (b < 1) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_observations: every entry of bins is positive");
        dims.bins[d] = b, dims.offset[d] = (int32_t)table;
        table += b - 1;
        if (table > MI_DISCRETIZE_MAX_TABLE)
            return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_observations: more than MI_DISCRETIZE_MAX_TABLE (2048) interior edges");
        if (!multidiscrete && prod > (INT64_C(1) << 62) / b)
            return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_observations: prod(bins) does not fit in 2^62");
        prod = multidiscrete ? 1 : prod * b;
    }
    dims.offset[MI_DISCRETIZE_MAX_DIM] = (int32_t)table;
    dims.narrow = !multidiscrete && prod < (INT64_C(1) << 31);
    if (table > 0 && !edges) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_observations: edges is NULL");
    const uintptr_t size = in_dtype == MI_F32 ? 4 : 8;
    if ((uintptr_t)in % size || (uintptr_t)lo % size || (uintptr_t)hi_clip % size || (uintptr_t)edges % size || (uintptr_t)out % 8)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_observations: a pointer is not aligned to its element type");
    if (rows > INT64_MAX / obs_dim) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_observations: rows * obs_dim overflows");
    if (rows == 0) return MI_OK;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess)
        e = in_dtype == MI_F32 ? launch_observations<float>((hipStream_t)hip_stream, in, rows, obs_dim, dims, lo, hi_clip, edges, multidiscrete, out)
                               : launch_observations<double>((hipStream_t)hip_stream, in, rows, obs_dim, dims, lo, hi_clip, edges, multidiscrete, out);
    return e == hipSuccess ? MI_OK : hip_failure("mi_discretize_observations", e);
}

int mi_discretize_actions(int device, void *hip_stream, const void *in, int in_dtype, int64_t rows, int act_dim, const int32_t *bins,
                          const void *centres, int multidiscrete, void *out, int out_dtype) {
    if (!in || !out || !bins || !centres || rows < 0) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "bad mi_discretize_actions argument");
    if (in_dtype != MI_I64 && in_dtype != MI_I32)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_actions reads int64 or int32 indices");
    if (out_dtype != MI_F32 && out_dtype != MI_F64)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_actions writes float32 or float64 actions");
    if (act_dim < 1 || act_dim > MI_TRANSFORM_MAX_ACT_DIM)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_actions: act_dim in [1, 32]");
    ActDims dims;
    int64_t table = 0;
    for (int d = 0; d < MI_DISCRETIZE_MAX_DIM; d++) {
        const int32_t b = d < act_dim ? bins[d] : 1;
        if (b < 1) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_actions: every entry of bins is positive");
        dims.bins[d] = b, dims.offset[d] = (int32_t)table;
        table += d < act_dim ? b : 0;
        if (table > MI_DISCRETIZE_MAX_TABLE)
            return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_actions: more than MI_DISCRETIZE_MAX_TABLE (2048) bin centres");
    }
    dims.offset[MI_DISCRETIZE_MAX_DIM] = (int32_t)table;
    int64_t prod = 1;
    for (int d = MI_DISCRETIZE_MAX_DIM - 1; d >= 0; d--) {
        dims.stride[d] = prod;
        if (!multidiscrete && prod > (INT64_C(1) << 62) / dims.bins[d])
            return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_actions: prod(bins) does not fit in 2^62");
        prod = multidiscrete ? 1 : prod * dims.bins[d];
    }
    dims.narrow = prod < (INT64_C(1) << 31);
    const uintptr_t isize = in_dtype == MI_I64 ? 8 : 4, osize = out_dtype == MI_F32 ? 4 : 8;
    if ((uintptr_t)in % isize || (uintptr_t)centres % osize || (uintptr_t)out % osize)
        return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_actions: a pointer is not aligned to its element type");
    if (rows > INT64_MAX / act_dim) return mi_internal::set_error(MI_ERR_INVALID_ARGUMENT, "mi_discretize_actions: rows * act_dim overflows");
    if (rows == 0) return MI_OK;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) {
        const hipStream_t st = (hipStream_t)hip_stream;
        if (in_dtype == MI_I64)
            e = out_dtype == MI_F32 ? launch_actions<int64_t, float>(st, in, rows, act_dim, dims, centres, multidiscrete, out)
                                    : launch_actions<int64_t, double>(st, in, rows, act_dim, dims, centres, multidiscrete, out);
        else
            e = out_dtype == MI_F32 ? launch_actions<int32_t, float>(st, in, rows, act_dim, dims, centres, multidiscrete, out)
                                    : launch_actions<int32_t, double>(st, in, rows, act_dim, dims, centres, multidiscrete, out);
    }
    return e == hipSuccess ? MI_OK : hip_failure("mi_discretize_actions", e);
}

#pragma GCC visibility pop
