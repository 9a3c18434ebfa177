// What the evaluation kernels (eval_metrics.hip, eval_plans.hip) share: the quantised distance every displacement sum is made of, the
// wave sum of such quanta and the "first maximum" of a forecast's six mode scores.  One definition, so that the two kernels and their
// NumPy specifications (lav_amd.train.evaluate._quanta) cannot drift apart.
//
// Floating point: float64 from the float32 inputs, contraction off (here and in lav_amd/build.py), so that dx * dx + dy * dy and
// sqrt(.) * 2^20 round as NumPy rounds them; llrint rounds to nearest even like np.rint.
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)

namespace lav {
constexpr int EVAL_CMDS = 6;                // LAV's commands: the plan's per-command counters and the modes of a forecast
constexpr double EVAL_Q = 1048576.0;        // 2^20 quanta per metre
constexpr double EVAL_FAR = 4294967296.0;   // 2^32 m: a distance that is not below it (NaN, Inf, absurd) makes its plan "non-finite"

// q = llrint(|a - b| * 2^20) in float64; false where the distance is not below 2^32 m
__device__ __forceinline__ bool quantum(const float *a, const float *b, long long &q) {
    const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1];
    const double d = sqrt(dx * dx + dy * dy);
    const bool ok = d < EVAL_FAR;
    q = ok ? llrint(d * EVAL_Q) : 0;
    return ok;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// np.argmax of six scores: the first maximum, and a NaN counts as one
__device__ __forceinline__ int first_max(const float *v) {
    float bv = v[0];
    int top = 0;
    for (int m = 1; m < EVAL_CMDS && bv == bv; ++m) {
        const float x = v[m];
        if (x > bv || x != x) { bv = x; top = m; }
    }
    return top;
}

// the gap of two scores (eval_distill.hip): g = llrint(|a - b| * 2^20) in float64; false where the difference is not below 2^32 - a NaN,
// an Inf, or a pair of absurd scores whose quanta would not fit the 64-bit sums
__device__ __forceinline__ bool scalar_gap(float a, float b, long long &g) {
    const double d = fabs((double)a - (double)b);
    const bool ok = d < EVAL_FAR;
    g = ok ? llrint(d * EVAL_Q) : 0;
    return ok;
}
}  // namespace lav
