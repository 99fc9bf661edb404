// per_env_normalize_internal.h -- the arithmetic of gymnasium.wrappers.NormalizeObservation / NormalizeReward around ONE scalar env, as the
// reference's NumPy expressions evaluate it for a batch of one (gymnasium v1.4.0):
//   gymnasium/wrappers/utils.py:33-71                     RunningMeanStd.update -> update_mean_var_count_from_moments
//   gymnasium/wrappers/stateful_observation.py:555-561    NormalizeObservation.observation
//   gymnasium/wrappers/stateful_reward.py:127-142         NormalizeReward.step
//
// Plain C++ for the host and the device alike: one statement per NumPy ufunc call, every operation rounded once in the type NumPy computes it in,
// IEEE division and square root, no intrinsics.  Whoever includes this compiles with -ffp-contract=off (a fused multiply-add rounds once where
// NumPy rounds twice) and without fast-math; the device unit needs hipcc's default correctly rounded float32 division and sqrtf.
//
// The batch is np.array([x]): its mean is x and its variance 0 exactly, batch_count is the Python int 1 (x * 1 is exact and drops out), and
// `m_a + m_b` adds +0.0 to a non-negative product, which changes nothing.  `count` is a Python float: it accumulates in float64 and, under NEP 50, is a WEAK
// scalar wherever it meets a float32 array -- rounded to float32 at every such use.
#ifndef MI_PER_ENV_NORMALIZE_INTERNAL_H
#define MI_PER_ENV_NORMALIZE_INTERNAL_H

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MI_PEN_FN __host__ __device__ inline
#else
#define MI_PEN_FN inline
#endif

namespace mi_per_env {

// float32 observations: mean / var are float32 arrays from construction on.  RunningMeanStd.update(np.array([x])), one column.
MI_PEN_FN void update_f32(float x, float &mean, float &var, double &count) {
    const double tot = count + 1.0;             // tot_count = count + batch_count            (Python floats)
    const float cf = (float)count, tf = (float)tot;
    const float d = x - mean;                   // delta = batch_mean - mean
    const float q = d / tf;                     // delta * batch_count / tot_count
    const float ma = var * cf;                  // m_a = var * count
    const float sq = d * d;                     // np.square(delta)
    const float sc = sq * cf;                   //   * count
    const float mc = sc / tf;                   //   * batch_count / tot_count
    const float m2 = ma + mc;                   // M2 = m_a + m_b + ...                       (m_b = 0)
    mean = mean + q;
    var = m2 / tf;
    count = tot;
}

// float64 observations: the same recurrence in float64.  `first`: this is the first update since construction -- the reference's arrays are still
// float32 then (mean 0, var 1), so m_a = var * count is a float32 product with the weak `count`, widened afterwards; everything else already
// promotes to float64 against the float64 batch.
MI_PEN_FN void update_f64(double x, double &mean, double &var, double &count, bool first) {
    const double tot = count + 1.0;
    const double d = x - mean;
    const double q = d / tot;
    const double ma = first ? (double)((float)var * (float)count) : var * count;
    const double sq = d * d;
    const double sc = sq * count;
    const double mc = sc / tot;
    const double m2 = ma + mc;
    mean = mean + q;
    var = m2 / tot;
    count = tot;
}

// NormalizeReward.step of a step the scalar env really took: the discounted return, then -- if `update` -- return_rms.update(discounted_reward);
// return_rms is float64 from construction on.  (1 - terminated) is a factor, not a select: a negative return times 0 is -0.0.
MI_PEN_FN void reward_step(double reward, bool terminated, double gamma, bool update, double &acc, double &mean, double &var, double &count) {
    const double g = acc * gamma;
    const double k = g * (double)(1 - (int)terminated);
    acc = k + reward;
    if (update) update_f64(acc, mean, var, count, false);
}

// np.float32((observation - mean) / np.sqrt(var + epsilon)) with float32 arrays: epsilon is weak.
MI_PEN_FN float normalize_f32(float x, float mean, float var, double epsilon) {
    const float c = x - mean;
    const float v = var + (float)epsilon;
    const float s = sqrtf(v);
    return c / s;
}

// ... with float64 arrays: the quotient is rounded once to float32.
MI_PEN_FN float normalize_f64(double x, double mean, double var, double epsilon) {
    const double c = x - mean;
    const double v = var + epsilon;
    const double s = sqrt(v);
    return (float)(c / s);
}

// reward / np.sqrt(return_rms.var + epsilon)
MI_PEN_FN double normalize_reward(double reward, double var, double epsilon) {
    const double v = var + epsilon;
    const double s = sqrt(v);
    return reward / s;
}

// the two element types behind one name, for the kernels' templates
MI_PEN_FN void update(float x, float &mean, float &var, double &count, bool) { update_f32(x, mean, var, count); }
MI_PEN_FN void update(double x, double &mean, double &var, double &count, bool first) { update_f64(x, mean, var, count, first); }
MI_PEN_FN float normalize(float x, float mean, float var, double epsilon) { return normalize_f32(x, mean, var, epsilon); }
MI_PEN_FN float normalize(double x, double mean, double var, double epsilon) { return normalize_f64(x, mean, var, epsilon); }

}  // namespace mi_per_env

#endif
