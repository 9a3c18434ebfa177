// The GRU cell as every decoder kernel evaluates it (gru.hip, gru_seq.hip): one sigmoid, one gate function, one wave butterfly.
// Gate order r, z, n as in torch.nn.GRU; precise expf / tanhf (no fast-math).  Kernels that must agree bit for bit (k_plan_wave and
// k_plan_step, tests/test_gpu_gru_paths.py) agree because they call the same expressions here.
#pragma once
#include <hip/hip_runtime.h>

namespace lav {

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

struct GruGates {
    float r, z, n, h;   // the three gates (the training tape keeps them) and the new state
};

// x_*: input-side pre-activations W_ih u + b_ih;  gh_*: recurrent side W_hh h + b_hh;  h' = (1 - z) n + z h
__device__ __forceinline__ GruGates gru_gates(float x_r, float x_z, float x_n, float gh_r, float gh_z, float gh_n, float h_prev) {
    GruGates g;
    g.r = gru_sigmoid(x_r + gh_r);
    g.z = gru_sigmoid(x_z + gh_z);
    g.n = tanhf(x_n + g.r * gh_n);
    g.h = (1.f - g.z) * g.n + g.z * h_prev;
    return g;
}

// Every lane ends up with the sum over the wave's 64 lanes of each of N values: xor butterfly 32, 16, 8, 4, 2, 1, the N independent
// reductions interleaved level by level so that their shuffle latencies overlap.
template <int N>
__device__ __forceinline__ void wave_allsum(float (&v)[N]) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] += __shfl_xor(v[j], d, 64);
}

}  // namespace lav
