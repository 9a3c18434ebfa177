// Shared host/device helpers for liblav_amd (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <thread>
#include <vector>

#include "lav_amd.h"

namespace lav {

inline char *error_buffer() {
    static thread_local char buf[512] = {0};
    return buf;
}

inline int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

// Packed fp32 with op_sel (profiles/r05_coresidency.md): on gfx950 a v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 with an
// op_sel bit set - the low result takes the HIGH register of a 64-bit source pair - returns wrong values in lanes 48-63 while waves of
// a bf16-matrix + LDS heavy kernel share its SIMD, and never alone.  hipcc's SLP vectoriser emits that form freely, so the library is
// built with -fno-slp-vectorize (lav_amd/build.py), writes the packed instructions it wants by hand with op_sel = 0 (deconv.hip), and
// tests/test_capi_host.py rejects any packed fp32 instruction with an op_sel bit in the disassembly.
//
// Round 4 took those wrong results for an LDS effect; its helpers stay where they are used (they cost nothing): lds_store_fence keeps
// two 64-bit LDS stores from being merged into a ds_write2_b64 (tools/lds_hazard.py could not make that instruction fail; the CPU test
// that forbids it is a tripwire, not a known hazard), lds_commit / lds_keep wait for a wave's LDS stores with the stored values pinned.
__device__ __forceinline__ void lds_store_fence() { asm volatile("" ::: "memory"); }
__device__ __forceinline__ void lds_commit() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <class T>
__device__ __forceinline__ void lds_keep(T &v) { asm volatile("" : "+v"(v)); }

// ---- LAV_CONV_F16X3's scale hand-off (conv_f16.hip, conv_wgrad.hip): maxima of the finite |values| of a tensor, in parts
// the largest finite |v| of the wave's lanes, in every lane
__device__ __forceinline__ float wave_finite_absmax(float m) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    return m;
}
__device__ __forceinline__ float finite_abs(float v) {
    const float a = fabsf(v);
    return a <= 3.4028235e38f ? a : 0.f;
}
// max over parts[0 .. n) in every lane of the wave.  Every load of the pass is in flight at once: a loop of dependent-looking scalar
// loads paid one memory round trip per 64 parts (round 6, first version: 57 round trips for the feature map's 3648 parts - the head
// convolution got SLOWER than with its measuring launch).
__device__ __forceinline__ float parts_absmax(const float *__restrict__ parts, int n, int lane) {
    float m = 0.f;
    int i0 = 0;
    if ((reinterpret_cast<uintptr_t>(parts) & 15) == 0) {
        const float4 *p4 = reinterpret_cast<const float4 *>(parts);
        const int n4 = n >> 2;
        float4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        for (int j = lane; j < n4; j += 256) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = p4[min(j + 64 * u, n4 - 1)];   // (clamped: a repeated part changes no maximum)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc[u].x = fmaxf(acc[u].x, v[u].x); acc[u].y = fmaxf(acc[u].y, v[u].y);
                acc[u].z = fmaxf(acc[u].z, v[u].z); acc[u].w = fmaxf(acc[u].w, v[u].w);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) m = fmaxf(m, fmaxf(fmaxf(acc[u].x, acc[u].y), fmaxf(acc[u].z, acc[u].w)));
        i0 = n4 << 2;
    }
    for (int i = i0 + lane; i < n; i += 64) m = fmaxf(m, parts[i]);
    return wave_finite_absmax(m);
}

// ---- NaN through every epilogue (lav_amd.h: a non-finite value "gives NaN in the outputs it reaches"; tests/test_gpu_nonfinite.py)
// IEEE 754-2019 maximum: a NaN operand gives NaN and -0 < +0.  On gfx950 it is ONE v_maximum3_f32, where fmaxf (maxNum: the NaN is
// dropped) costs a canonicalising v_max_f32 and the v_max_f32 itself, and `(v > m || v != v) ? v : m` - k_maxpool3s2's idiom, the
// same function but for the sign of a zero - a compare and a select.  Finite operands give the bits fmaxf gives.
__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }
// The ReLU as torch.relu: a NaN stays a NaN (`v > 0.f ? v : 0.f` and fmaxf(v, 0.f) both turn it into 0, finite garbage that no health
// check counts).  -0 and every negative still give +0: finite data keeps its bits.
__device__ __forceinline__ float relu_nan(float v) { return max_nan(v, 0.f); }
// The 2x2 maximum as F.max_pool2d (two v_maximum3_f32)
__device__ __forceinline__ float max_nan4(float a, float b, float c, float d) { return max_nan(max_nan(a, b), max_nan(c, d)); }

#define LAV_HIP(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t lav_e_ = (expr);                                                                        \
        if (lav_e_ != hipSuccess)                                                                          \
            return lav::fail(LAV_EHIP, "%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(lav_e_)); \
    } while (0)

#define LAV_REQUIRE(cond, ...)                                     \
    do {                                                           \
        if (!(cond)) return lav::fail(LAV_EINVAL, __VA_ARGS__);    \
    } while (0)

// launch errors are sticky until queried; call after every kernel launch
#define LAV_LAUNCH_CHECK() LAV_HIP(hipGetLastError())

// Launch of a kernel with dynamic LDS beyond the 64 KB default: the first launch of every kernel instantiation raises its
// hipFuncAttributeMaxDynamicSharedMemorySize to `attr_bytes` (the attribute is per function; set once, it stays).
template <auto Kernel, class... A>
int launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, int attr_bytes, const A &...args) {
    static bool attr = false;
    if (!attr) {
        LAV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, attr_bytes));
        attr = true;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}

// For a kernel that also holds `static_bytes` of static LDS and wants the rest of the CU's 160 KB: asks for 160 KB minus the static
// part, settles for 152 KB where the runtime refuses, and clamps the launch's dynamic LDS to the cap it was granted (*cap_out).
template <auto Kernel, class... A>
int launch_lds_capped(dim3 grid, dim3 block, size_t lds, hipStream_t st, size_t static_bytes, size_t *cap_out, const A &...args) {
    static size_t cap = 0;
    if (!cap) {
        size_t c = (160 * 1024 - static_bytes) / 16 * 16;
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c) != hipSuccess) {
            (void)hipGetLastError();
            c = 152 * 1024;
            LAV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c));
        }
        cap = c;
    }
    if (cap_out) *cap_out = cap;
    hipLaunchKernelGGL(Kernel, grid, block, std::min(cap, lds), st, args...);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}

// CUs of the device that was current at the first call (256 where it cannot be asked): one workgroup per CU is what a persistent
// launch may count on to be resident at once
inline int cu_count() {
    static const int cus = [] {
        int dev = 0, v = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
        return v > 0 ? v : 256;
    }();
    return cus;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// bump allocator over the caller's workspace
struct Arena {
    char *base;
    size_t cap, used;
    Arena(void *p, size_t bytes) : base(static_cast<char *>(p)), cap(bytes), used(0) {}
    template <typename T>
    T *take(size_t count) {
        used = align_up(used, 256);
        T *p = reinterpret_cast<T *>(base + used);
        used += count * sizeof(T);
        return p;
    }
    bool ok() const { return used <= cap; }
};

constexpr int WAVE = 64;

// host-side parallel loop (weight repacking: a training run that logs through the inference engines repacks every layer per step)
template <typename F>
inline void parallel_for(int n, F fn) {
    unsigned nt = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
    if (n < 2 || nt < 2) {
        for (int i = 0; i < n; ++i) fn(i);
        return;
    }
    nt = std::min<unsigned>(nt, (unsigned)n);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([=] { for (int i = (int)t; i < n; i += (int)nt) fn(i); });
    for (auto &x : th) x.join();
}

// lav_batch_limit: device-resident row count honoured by the batch-aware launches of this thread (see lav_amd.h)
inline const int *&batch_limit() {
    static thread_local const int *p = nullptr;
    return p;
}

// Optional per-kernel HIP-event timers (lav_profile_enable / lav_profile_read in include/lav_amd.h).
// timer_begin returns a slot token (< 0 when profiling is off); both calls only record events on `st`.
int timer_begin(const char *name, hipStream_t st);
void timer_end(int token, hipStream_t st);

}  // namespace lav
