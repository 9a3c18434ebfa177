// Multi-tensor gradient statistics and a guarded Adam step (ABI 46), which can keep a moving average of the weights (ABI 48): the
// device half of lav_amd.train.optim.FusedAdam.  The specification is lav_amd.train.optim.fused_adam_numpy and the two agree in every
// stored bit (tests/test_gpu_optim.py, tests/test_gpu_ema.py); the sum of squares alone is pinned by a bound, n * 2^-53 relative,
// because its order of summation is this file's business.
//
// The work is cut into chunks of OPTIM_CHUNK elements, one workgroup per chunk; a row of the descriptor table carries the index of its
// tensor's first chunk, so a workgroup finds its tensor by a binary search over the rows.  Three launches, and every dependency between
// workgroups is a launch boundary (no workgroup waits for another inside a launch, no float atomic, no counter to clean):
//   k_optim_stats     per chunk of every gradient: the count of elements that are not finite and the float64 sum of the squares of the
//                     finite ones, into the chunk's slot of the partials; the chunks behind them scan the watched buffers.
//   k_optim_finalise  one workgroup: the partials in a fixed order, norm, clip factor, apply = no gradient element was not finite; when
//                     applying, one thread per tensor advances its step count and running powers and leaves the two float32 factors.
//   k_optim_update    per chunk, when apply is set: the Adam update in float32, every operation rounded on its own (this file is compiled
//                     with contraction off and correctly rounded division and square root).  When skipping it stores nothing.
//                     Its <true> instantiation (lav_optim_adam_ema_step) also moves a shadow e of every tensor towards the parameter it
//                     has just computed and still holds in registers: e = e + omd * (p - e), omd = float32(1 - min(decay, (1 + k) /
//                     (10 + k))) from the tensor's step count k in float64, once per workgroup.  One load and one store more per element.
// Pointers are 4-byte aligned only: a chunk runs on 16-byte accesses where p, m and v (and e) share a misalignment (g too, or g on
// 4-byte loads beside them), heads and tails on 4-byte accesses; otherwise on 4-byte accesses throughout.
#include "common.hpp"

namespace {
using namespace lav;
constexpr int OPTIM_CHUNK = 4096;                    // elements per workgroup: 256 threads, four 16-byte accesses per array each
constexpr int THREADS = 256;

// the row of the largest chunk0 <= chunk: rows are in chunk order, and a row without elements shares its chunk0 with the next
template <class Row>
__device__ __forceinline__ int find_row(const Row *__restrict__ rows, int n, int chunk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool finite32(float x) { return fabsf(x) <= 3.4028235e38f; }

// elements of a chunk in front of the first 16-byte boundary of `p`
__device__ __forceinline__ int head_of(const void *p, int n) {
    const int h = (int)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2;
    return min(h, n);
}

struct Acc {
    double sumsq;
    int bad;
    __device__ __forceinline__ void take(float x) {
        if (finite32(x)) sumsq += (double)x * (double)x; else ++bad;
    }
};

// every element of one chunk exactly once: the head and the tail on the first lanes, the 16-byte groups strided over the workgroup
__device__ __forceinline__ Acc scan_chunk(const float *__restrict__ g, int n, int tid) {
    Acc a = {0.0, 0};
    const int head = head_of(g, n), nv = (n - head) >> 2, tail = head + 4 * nv;
    if (tid < head) a.take(g[tid]);
    const float4 *g4 = reinterpret_cast<const float4 *>(g + head);
    for (int k = tid; k < nv; k += THREADS) {
        const float4 x = g4[k];
        a.take(x.x); a.take(x.y); a.take(x.z); a.take(x.w);
    }
    if (tail + tid < n) a.take(g[tail + tid]);
    return a;
}

__global__ __launch_bounds__(THREADS) void k_optim_stats(const lav_optim_tensor *__restrict__ table, int ntensors, int total_chunks,
                                                         const lav_optim_watch *__restrict__ watch, int nwatch,
                                                         double *__restrict__ part_sumsq, int *__restrict__ part_bad) {
    __shared__ double s_sum[THREADS / WAVE];
    __shared__ int s_bad[THREADS / WAVE];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const float *src;
    long long numel, first;
    if (chunk < total_chunks) {
        const lav_optim_tensor &row = table[find_row(table, ntensors, chunk)];
        src = row.g; numel = row.numel; first = (long long)(chunk - row.chunk0) * OPTIM_CHUNK;
    } else {
        const lav_optim_watch &row = watch[find_row(watch, nwatch, chunk - total_chunks)];
        src = row.data; numel = row.numel; first = (long long)(chunk - total_chunks - row.chunk0) * OPTIM_CHUNK;
    }
    const long long left = numel - first;
    const int n = left <= 0 ? 0 : (int)(left < OPTIM_CHUNK ? left : OPTIM_CHUNK);
    Acc a = scan_chunk(src + first, n, tid);
#pragma unroll
    for (int o = WAVE / 2; o >= 1; o >>= 1) {        // lane l takes lane l + o: a fixed tree
        a.sumsq += __shfl_down(a.sumsq, o, WAVE);
        a.bad += __shfl_down(a.bad, o, WAVE);
    }
    if ((tid & (WAVE - 1)) == 0) { s_sum[tid / WAVE] = a.sumsq; s_bad[tid / WAVE] = a.bad; }
    __syncthreads();
    if (tid == 0) {
        double s = s_sum[0];
        int b = s_bad[0];
        for (int w = 1; w < THREADS / WAVE; ++w) { s += s_sum[w]; b += s_bad[w]; }
        part_sumsq[chunk] = chunk < total_chunks ? s : 0.0;
        part_bad[chunk] = b;
    }
}

// advance != 0: the step's decision, counters and per-tensor words; 0: the statistics words of `global` alone
__global__ __launch_bounds__(THREADS) void k_optim_finalise(const lav_optim_tensor *__restrict__ table, int ntensors, int total_chunks,
                                                            int watch_chunks, const double *__restrict__ part_sumsq,
                                                            const int *__restrict__ part_bad, double max_norm, int advance,
                                                            lav_optim_state *__restrict__ state, lav_optim_global *__restrict__ global) {
    __shared__ double s_sum[THREADS];
    __shared__ long long s_bad[THREADS], s_watch[THREADS];
    __shared__ int s_apply;
    const int tid = threadIdx.x;
    double sum = 0.0;
    long long bad = 0, wbad = 0;
    for (int i = tid; i < total_chunks; i += THREADS) { sum += part_sumsq[i]; bad += part_bad[i]; }
    for (int i = tid; i < watch_chunks; i += THREADS) wbad += part_bad[total_chunks + i];
    s_sum[tid] = sum; lds_store_fence(); s_bad[tid] = bad; lds_store_fence(); s_watch[tid] = wbad;      // (no ds_write2_b64: common.hpp)
    __syncthreads();
    for (int o = THREADS / 2; o >= 1; o >>= 1) {
        if (tid < o) {
            s_sum[tid] += s_sum[tid + o]; lds_store_fence();
            s_bad[tid] += s_bad[tid + o]; lds_store_fence();
            s_watch[tid] += s_watch[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double sumsq = s_sum[0], norm = sqrt(sumsq);
        double clip = 1.0;
        if (max_norm > 0.0) clip = fmin(1.0, max_norm / (norm + 1e-6));
        const int apply = s_bad[0] == 0;
        global->nonfinite = s_bad[0];
        global->sumsq = sumsq;
        global->clip = (float)clip;
        global->apply = apply;
        global->watch_nonfinite = s_watch[0];
        if (advance) {
            if (apply) global->applied += 1; else global->skipped += 1;
        }
        s_apply = apply && advance;
    }
    __syncthreads();
    if (!s_apply) return;
    for (int r = tid; r < ntensors; r += THREADS) {
        const lav_optim_tensor &row = table[r];
        lav_optim_state &st = state[row.state];
        const double b1 = st.beta1_power * row.beta1, b2 = st.beta2_power * row.beta2;
        st.step += 1;
        st.beta1_power = b1;
        st.beta2_power = b2;
        st.step_size = (float)(row.lr / (1.0 - b1));
        st.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - b2));
    }
}

struct Coef {
    float clip, beta1, beta2, om1, om2, step_size, inv, eps;
    float omd;      // EMA alone: 1 - d_k
};

__device__ __forceinline__ void adam1(float g, float &p, float &m, float &v, const Coef &c) {
    const float gs = g * c.clip;
    m = c.beta1 * m + c.om1 * gs;
    v = c.beta2 * v + (c.om2 * gs) * gs;
    p = p - c.step_size * (m / (sqrtf(v) * c.inv + c.eps));
}

__device__ __forceinline__ void ema1(float p, float &e, const Coef &c) { e = e + c.omd * (p - e); }

template <bool EMA>
__device__ __forceinline__ void adam_scalar(const float *__restrict__ g, float *__restrict__ p, float *__restrict__ m, float *__restrict__ v,
                                            float *__restrict__ e, int i, const Coef &c) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam1(g[i], pi, mi, vi, c);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if constexpr (EMA) {
        float ei = e[i];
        ema1(pi, ei, c);
        e[i] = ei;
    }
}

// EMA: `shadow` holds one pointer per row of the table, to the tensor's moving average e
template <bool EMA>
__global__ __launch_bounds__(THREADS) void k_optim_update(const lav_optim_tensor *__restrict__ table, int ntensors,
                                                          const lav_optim_state *__restrict__ state,
                                                          const lav_optim_global *__restrict__ global, float *const *__restrict__ shadow,
                                                          double ema_decay) {
    if (!global->apply) return;
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const int r = find_row(table, ntensors, chunk);
    const lav_optim_tensor &row = table[r];
    const long long first = (long long)(chunk - row.chunk0) * OPTIM_CHUNK, left = row.numel - first;
    const int n = left <= 0 ? 0 : (int)(left < OPTIM_CHUNK ? left : OPTIM_CHUNK);
    const lav_optim_state &st = state[row.state];
    Coef c;
    c.clip = global->clip;
    c.beta1 = (float)row.beta1; c.beta2 = (float)row.beta2;
    c.om1 = (float)(1.0 - row.beta1); c.om2 = (float)(1.0 - row.beta2);      // constants: float64, rounded once
    c.step_size = st.step_size; c.inv = st.inv_sqrt_bc2; c.eps = (float)row.eps;
    c.omd = 0.0f;
    const float *__restrict__ g = row.g + first;
    float *__restrict__ p = row.p + first, *__restrict__ m = row.m + first, *__restrict__ v = row.v + first;
    float *__restrict__ e = nullptr;
    if constexpr (EMA) {
        const double k = (double)st.step;           // (advanced by k_optim_finalise: >= 1)
        c.omd = (float)(1.0 - fmin(ema_decay, (1.0 + k) / (10.0 + k)));
        e = shadow[r] + first;
    }
    const uintptr_t ap = reinterpret_cast<uintptr_t>(p) & 15;
    bool same = ap == (reinterpret_cast<uintptr_t>(m) & 15) && ap == (reinterpret_cast<uintptr_t>(v) & 15);
    if constexpr (EMA) same = same && ap == (reinterpret_cast<uintptr_t>(e) & 15);
    if (!same) {
        for (int i = tid; i < n; i += THREADS) adam_scalar<EMA>(g, p, m, v, e, i, c);
        return;
    }
    const bool g16 = (reinterpret_cast<uintptr_t>(g) & 15) == ap;     // a gradient that is a view into a bucket is often not
    const int head = head_of(p, n), nv = (n - head) >> 2, tail = head + 4 * nv;
    if (tid < head) adam_scalar<EMA>(g, p, m, v, e, tid, c);
    float4 *p4 = reinterpret_cast<float4 *>(p + head), *m4 = reinterpret_cast<float4 *>(m + head), *v4 = reinterpret_cast<float4 *>(v + head);
    for (int k = tid; k < nv; k += THREADS) {
        float4 gg;
        if (g16) {
            gg = reinterpret_cast<const float4 *>(g + head)[k];
        } else {
            const float *gs = g + head + 4 * k;
            gg.x = gs[0]; gg.y = gs[1]; gg.z = gs[2]; gg.w = gs[3];
        }
        float4 pp = p4[k], mm = m4[k], vv = v4[k];
        adam1(gg.x, pp.x, mm.x, vv.x, c);
        adam1(gg.y, pp.y, mm.y, vv.y, c);
        adam1(gg.z, pp.z, mm.z, vv.z, c);
        adam1(gg.w, pp.w, mm.w, vv.w, c);
        p4[k] = pp; m4[k] = mm; v4[k] = vv;
        if constexpr (EMA) {
            float4 *e4 = reinterpret_cast<float4 *>(e + head);
            float4 ee = e4[k];
            ema1(pp.x, ee.x, c); ema1(pp.y, ee.y, c); ema1(pp.z, ee.z, c); ema1(pp.w, ee.w, c);
            e4[k] = ee;
        }
    }
    if (tail + tid < n) adam_scalar<EMA>(g, p, m, v, e, tail + tid, c);
}

int check_args(const void *table, int ntensors, int total_chunks, const void *watch, int nwatch, int watch_chunks, const void *global,
               const void *workspace, size_t workspace_bytes) {
    LAV_REQUIRE(ntensors >= 0 && total_chunks >= 0 && nwatch >= 0 && watch_chunks >= 0, "lav_optim: negative counts");
    LAV_REQUIRE((ntensors == 0) == (total_chunks == 0) && (nwatch == 0) == (watch_chunks == 0), "lav_optim: a table without chunks, or chunks without a table");
    LAV_REQUIRE(total_chunks >= ntensors && watch_chunks >= nwatch, "lav_optim: fewer chunks than rows (a row has at least one element)");
    LAV_REQUIRE((long long)total_chunks + watch_chunks <= 0x7fffffffLL, "lav_optim: %lld chunks", (long long)total_chunks + watch_chunks);
    LAV_REQUIRE((ntensors == 0 || table) && (nwatch == 0 || watch) && global, "lav_optim: null table or words");
    LAV_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "lav_optim: workspace must be 256-byte aligned");
    LAV_REQUIRE(workspace_bytes >= lav_optim_workspace_bytes(total_chunks, watch_chunks), "lav_optim: workspace of %zu bytes, needs %zu",
                workspace_bytes, lav_optim_workspace_bytes(total_chunks, watch_chunks));
    return LAV_OK;
}

int run(const lav_optim_tensor *table, int ntensors, int total_chunks, const lav_optim_watch *watch, int nwatch, int watch_chunks,
        lav_optim_state *state, lav_optim_global *global, double max_norm, int advance, float *const *shadow, double ema_decay,
        void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_args(table, ntensors, total_chunks, watch, nwatch, watch_chunks, global, workspace, workspace_bytes)) return rc;
    LAV_REQUIRE(!advance || ntensors == 0 || state, "lav_optim_adam_step: null state words");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int chunks = total_chunks + watch_chunks;
    double *part_sumsq = static_cast<double *>(workspace);
    int *part_bad = reinterpret_cast<int *>(static_cast<char *>(workspace) + align_up((size_t)std::max(chunks, 1) * sizeof(double), 256));
    const int tok_stats = timer_begin("optim_stats", st);        // (lav_profile_read: statistics + finalise, and the update, apart)
    if (chunks > 0)
        hipLaunchKernelGGL(k_optim_stats, dim3(chunks), dim3(THREADS), 0, st, table, ntensors, total_chunks, watch, nwatch, part_sumsq, part_bad);
    hipLaunchKernelGGL(k_optim_finalise, dim3(1), dim3(THREADS), 0, st, table, ntensors, total_chunks, watch_chunks, part_sumsq, part_bad, max_norm,
                       advance, state, global);
    timer_end(tok_stats, st);
    LAV_LAUNCH_CHECK();
    if (advance && total_chunks > 0) {
        const int tok = timer_begin("optim_update", st);
        if (shadow)
            hipLaunchKernelGGL(k_optim_update<true>, dim3(total_chunks), dim3(THREADS), 0, st, table, ntensors, state, global, shadow, ema_decay);
        else
            hipLaunchKernelGGL(k_optim_update<false>, dim3(total_chunks), dim3(THREADS), 0, st, table, ntensors, state, global, shadow, 0.0);
        timer_end(tok, st);
        LAV_LAUNCH_CHECK();
    }
    return LAV_OK;
}
}  // namespace

extern "C" int lav_optim_chunk(void) { return OPTIM_CHUNK; }

extern "C" size_t lav_optim_workspace_bytes(long long total_chunks, long long watch_chunks) {
    if (total_chunks < 0 || watch_chunks < 0 || total_chunks + watch_chunks > 0x7fffffffLL) return 0;
    const size_t chunks = (size_t)std::max(total_chunks + watch_chunks, 1LL);
    return lav::align_up(chunks * sizeof(double), 256) + lav::align_up(chunks * sizeof(int), 256);
}

extern "C" int lav_optim_grad_stats(const lav_optim_tensor *table, int ntensors, int total_chunks, const lav_optim_watch *watch, int nwatch,
                                    int watch_chunks, lav_optim_global *global, double max_norm, void *workspace, size_t workspace_bytes,
                                    void *stream) {
    return run(table, ntensors, total_chunks, watch, nwatch, watch_chunks, nullptr, global, max_norm, 0, nullptr, 0.0, workspace, workspace_bytes, stream);
}

extern "C" int lav_optim_adam_step(const lav_optim_tensor *table, int ntensors, int total_chunks, const lav_optim_watch *watch, int nwatch,
                                   int watch_chunks, lav_optim_state *state, lav_optim_global *global, double max_norm, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    return run(table, ntensors, total_chunks, watch, nwatch, watch_chunks, state, global, max_norm, 1, nullptr, 0.0, workspace, workspace_bytes, stream);
}

extern "C" int lav_optim_adam_ema_step(const lav_optim_tensor *table, int ntensors, int total_chunks, const lav_optim_watch *watch, int nwatch,
                                       int watch_chunks, lav_optim_state *state, lav_optim_global *global, double max_norm,
                                       float *const *shadow, double ema_decay, void *workspace, size_t workspace_bytes, void *stream) {
    LAV_REQUIRE(ema_decay > 0.0 && ema_decay < 1.0, "lav_optim_adam_ema_step: ema_decay %g (0 < decay < 1)", ema_decay);
    LAV_REQUIRE(ntensors <= 0 || shadow, "lav_optim_adam_ema_step: null shadow pointers");
    return run(table, ntensors, total_chunks, watch, nwatch, watch_chunks, state, global, max_norm, 1, shadow, ema_decay, workspace, workspace_bytes,
               stream);
}
