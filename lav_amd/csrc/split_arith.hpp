// The split-operand arithmetic ("bf16x6" / "f16x3"): fp32 dot products on the matrix cores.  Every convolution kernel of the hot
// path (conv_split_kernel.hpp, conv_pair.hip, conv_run.hip, conv_wgrad.hip) and every host packer (conv_split.hpp, conv_pair.hip)
// takes its pieces, scales and product order from here; tests/test_gpu_f16x3_contract.py, test_gpu_conv.py, test_gpu_conv_run.py,
// test_gpu_conv_exact.py (bit for bit against float64 on exactly representable data) and tests/test_capi_host.py hold them to it.
//
// bf16x6   v_mfma_f32_32x32x2_f32 runs at the fp32 VECTOR rate (157 TFLOP/s, 1/16 of the bf16 matrix rate).  Every fp32 value is the
//          exact sum of three bf16 pieces, x = x0 + x1 + x2 (8 + 8 + 8 significant bits; x1 = bf16(x - x0), ...: x - bf16(x) and the
//          second remainder are exact, the third piece has at most 8 significant bits left), so
//              a*b = a0b0 + (a0b1 + a1b0) + (a0b2 + a2b0 + a1b1) + O(2^-24 |ab|)
//          is six v_mfma_f32_32x32x16_bf16 (products exact, fp32 accumulate) per 16 k-steps instead of eight fp32 MFMAs of 64 cycles,
//          with the error of an fp32 dot product (tools/probes/split_mfma_probe.hip on MI355X, K = 1152, 2^12 dynamic range: max
//          |err| / sum|ab| 3.1e-7 against 6.3e-7 for the fp32 MFMA chain).  fp32 range is kept (bf16 has the fp32 exponent); no finite
//          input overflows: the first piece never rounds up into the Inf exponent (split3 truncates there, split3_pair clamps at the
//          largest finite bf16 and the remainder carries the rest).  Non-finite x: the first piece keeps Inf / NaN and the rest become
//          NaN (Inf - Inf), so the output is NaN where the fp32 kernels (and the reference) propagate Inf - documented in lav_amd.h.
//          fp32 SUBNORMAL inputs are flushed by the bf16 matrix pipe.
// f16x3    (LAV_CONV_F16X3) x = s (h0 + h1) with two fp16 pieces of u = x / s: u = h0 + h1 + O(2^-22 |u|) (round to nearest; what is
//          below fp16's subnormal quantum 2^-24 - 2^-39 of the tensor's largest value - is lost).  a . b ~ a0 b0 + a0 b1 + a1 b0 is
//          THREE v_mfma_f32_32x32x16_f16 per 16 k-steps instead of six bf16 ones, at 22 instead of 24 bits per operand: the error of
//          the dot product stays at the level of its fp32 accumulation (tests/test_gpu_conv.py).
// scale    s = f16_scale_of(m): the power of two that puts the tensor's largest finite magnitude m into [16384, 32768) - fp16
//          overflows at 65504, so |u| <= 32768 and nothing overflows; 1 / s is a power of two: exact.  The exponent is floored at
//          -100: a tensor whose largest value is below 2^-100 - or subnormal - would give a subnormal scale and an infinite
//          reciprocal.  With the floor such a tensor is divided by 2^-115: its values, fp32 subnormals included, are kept down to
//          2^-140.  Inf / NaN do not enter the maximum and propagate through the data path as they are.
// epilogue The accumulators are in units of (activation scale x weight scale).  f16_out_scales: the epilogue multiplies by two powers
//          of two one after the other: sx * sw alone can overflow (2^113 * 2^113), and so can acc * sx when the weights are small
//          (activations near FLT_MAX: acc ~ 2^32, sx = 2^113).  Both factors are therefore the halves of sx * sw's exponent:
//          acc * out_sx lies between acc and y, so it over- or underflows only where y does, and y is rounded once, as with any other
//          split of the exponent.
// order    The partial products of a k-block are added smallest terms first (BF16X6_A / _B, F16X3_A / _B: which piece of either
//          operand the k-th matrix instruction takes); consecutive instructions go to different accumulators.  conv_run.hip spells
//          the same order out by hand; conv_wgrad.hip's mma_pieces adds largest first and stays as it is (its results would change).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"

namespace lav {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// which piece of the A / B operand the k-th product of a k-block takes (forward kernels: smallest terms first)
constexpr int BF16X6_A[6] = {1, 2, 0, 1, 0, 0}, BF16X6_B[6] = {1, 0, 2, 0, 1, 0};
constexpr int F16X3_A[3] = {1, 0, 0}, F16X3_B[3] = {0, 1, 0};   // fp16 pieces: a1 b0, a0 b1, a0 b0

// x -> three bf16 pieces (round half up on the dropped bits), returned in the HIGH halves of p0..p2.  Where the round-up would
// carry into the Inf / NaN exponent (|x| within half a bf16 ulp of FLT_MAX) the first piece is truncated instead: the pieces still
// sum to x exactly.
__device__ __forceinline__ void split3(float x, unsigned &p0, unsigned &p1, unsigned &p2) {
    const unsigned u = __float_as_uint(x), r = u + 0x8000u;
    p0 = ((r & 0x7f800000u) == 0x7f800000u ? u : r) & 0xffff0000u;
    const float r1 = x - __uint_as_float(p0);          // exact
    p1 = (__float_as_uint(r1) + 0x8000u) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(p1);         // exact
    p2 = __float_as_uint(r2) + 0x8000u;                // low half is dropped by the pack
}
// the same rounding on the host (the weight packers): the bf16 nearest to x by split3's rule, rest = x - that piece (exact)
inline unsigned short bf16_round(float x, float &rest) {
    unsigned u;
    memcpy(&u, &x, 4);
    const unsigned r = u + 0x8000u;
    u = ((r & 0x7f800000u) == 0x7f800000u ? u : r) & 0xffff0000u;   // as split3: no round-up into the Inf exponent
    float b;
    memcpy(&b, &u, 4);
    rest = x - b;
    return (unsigned short)(u >> 16);
}
// Two values at once on the conversion unit (round 4): v_cvt_pk_bf16_f32 rounds both to bf16 (nearest even) and packs them, so a
// pair costs 13 instructions instead of ~25 - the activation loaders' conversion of a chunk sat in the critical path of its
// barrier interval (in-kernel trace of the BEV layers: 2.4 k cycles per chunk).  q0..q2 = the three pieces of (x0, x1), x0 in the
// low half.  The first piece of |x| > the largest finite bf16 is that bound (the remainder carries the rest).
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned &q0, unsigned &q1, unsigned &q2) {
    constexpr float M = 3.3895313892515355e38f;   // 0x7f7f0000
    const float c0 = __builtin_amdgcn_fmed3f(x0, -M, M), c1 = __builtin_amdgcn_fmed3f(x1, -M, M);
    q0 = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{c0, c1}, bf16x2));
    const float r0 = x0 - __uint_as_float(q0 << 16), r1 = x1 - __uint_as_float(q0 & 0xffff0000u);
    q1 = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, bf16x2));
    const float s0 = r0 - __uint_as_float(q1 << 16), s1 = r1 - __uint_as_float(q1 & 0xffff0000u);
    q2 = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{s0, s1}, bf16x2));
}
// two values -> two fp16 pieces each (u0 in the low half); |u| <= 32768 by the caller's power-of-two scale
__device__ __forceinline__ void split2h_pair(float u0, float u1, unsigned &q0, unsigned &q1) {
    const f16x2 h0 = __builtin_convertvector(f32x2{u0, u1}, f16x2);
    const f32x2 f0 = __builtin_convertvector(h0, f32x2);
    const f16x2 h1 = __builtin_convertvector(f32x2{u0 - f0[0], u1 - f0[1]}, f16x2);
    q0 = __builtin_bit_cast(unsigned, h0);
    q1 = __builtin_bit_cast(unsigned, h1);
}
// the pieces of two values (x0 in the low half): three bf16 pieces of x exactly, or two fp16 pieces of x * inv
template <bool F16>
__device__ __forceinline__ void split_pair(float x0, float x1, float inv, unsigned (&q)[F16 ? 2 : 3]) {
    if constexpr (F16) split2h_pair(x0 * inv, x1 * inv, q[0], q[1]);
    else split3_pair(x0, x1, q[0], q[1], q[2]);
}
// {hi half of odd, hi half of even} -> one dword of two bf16 (even in the low half)
__device__ __forceinline__ unsigned pack_hi(unsigned even, unsigned odd) { return __builtin_amdgcn_perm(odd, even, 0x07060302u); }

// the scale of a tensor whose largest finite magnitude is m (device kernels and host packers: device re-packs compare equal).  Two
// overloads of one expression, not one __host__ __device__ function: as such hipcc allocates the registers of k_conv_split_f16 and
// k_conv1d_pair_chain_f16 differently (same arithmetic, other code), and the kernels are to stay instruction for instruction what they were.
__device__ __forceinline__ float f16_scale_of(float m) {
    int e = 0;
    (void)frexpf(m, &e);                           // m = f 2^e, f in [0.5, 1): m / 2^(e - 15) in [16384, 32768)
    return ldexpf(1.f, m > 0.f ? max(e, -100) - 15 : 0);
}
__host__ inline float f16_scale_of(float m) {
    int e = 0;
    (void)frexpf(m, &e);
    return ldexpf(1.f, m > 0.f ? std::max(e, -100) - 15 : 0);
}
// the epilogue's two factors: out_sx * out_sw = sx * sw = 2^et (both are powers of two in [2^-115, 2^113]), the exponent in halves
__device__ __forceinline__ void f16_out_scales(float sx, float sw, float &out_sx, float &out_sw) {
    int ex = 0, ew = 0;
    (void)frexpf(sx, &ex);
    (void)frexpf(sw, &ew);
    const int et = ex + ew - 2;
    out_sx = ldexpf(1.f, et >> 1); out_sw = ldexpf(1.f, et - (et >> 1));
}

}  // namespace lav
