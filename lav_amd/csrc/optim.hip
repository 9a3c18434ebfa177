// Multi-tensor gradient statistics and a guarded Adam step (ABI 46), which can keep a moving average of the weights (ABI 48), and the
// per-tensor view of such a step with the ring that names who made one skip (ABI 50): the device half of lav_amd.train.optim.FusedAdam.  The specification is lav_amd.train.optim.fused_adam_numpy and the two agree in every
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
//
// The per-tensor view of a step (ABI 50, lav_optim_tensor_stats; specification lav_amd.train.optim.tensor_stats_numpy) runs behind it over
// the same table, watch rows and state words, and stores into none of them:
//   k_tensor_stats    per chunk, one pass over g, p, m, v: of g the elements that are not finite, the zeros, the float64 sum of squares
//                     and the largest bit pattern of the finite |g|, and 64 bins of its exponent field; of p the same without zeros
//                     and bins; of u = step_size * (m / (sqrtf(v) * inv_sqrt_bc2 + eps)), adam1's term from the words and moments as
//                     they stand, the sum of squares and the maximum.  The partials go to the chunk's slot; the chunks behind the
//                     table's scan the watched buffers.  Each wave keeps its own bins in LDS and adds to them with LDS atomics (DESIGN 4.7o
//                     has the measurement and the forms that lost).
//   k_tensor_reduce   one wave per tensor and per watched buffer: its chunks' partials in chunk order, integers as int64.
// lav_optim_blame (k_optim_blame, one workgroup behind a step) reads the counts k_optim_stats left per chunk: when the step was skipped
// one thread appends the first four tensors and watched buffers that hold elements that are not finite to two rings of 16 records.
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

// ---- the per-tensor view (lav_optim_tensor_stats) --------------------------------------------------------------------------------
constexpr int BINS = LAV_OPTIM_HIST_BINS;
constexpr int WAVES = THREADS / WAVE;

// what one chunk leaves for its tensor: [0] g, [1] p, [2] u.  A chunk has at most OPTIM_CHUNK elements: its bins fit 16 bits
struct TensorPart {
    double sumsq[3];
    int count[3];                   // g not finite, g zero, p not finite
    unsigned maxbits[3];            // the largest bit pattern of a finite |x|
    unsigned short hist[BINS];
};
static_assert(sizeof(TensorPart) == 176 && OPTIM_CHUNK < 65536, "the layout lav_optim_tensor_stats_workspace_bytes counts on");
struct WatchPart {
    int bad;
    unsigned maxbits;
};

struct UCoef {
    float step_size, inv, eps;
    bool stepped;
};

struct TAcc {
    double sumsq[3];
    int count[3];
    unsigned maxbits[3];
};

// the bin of a finite |x| given as its bit pattern: a function of the exponent field alone
__device__ __forceinline__ int bin_of(unsigned a) { return min(max((int)(a >> 23) - 86, 0), BINS - 1); }

// One count per finite gradient element into the wave's own 64 bins in LDS (ds_add_u32 without a return value).  Each wave has its own
// copy, so no two waves meet on an address; lanes of one wave that share a bin are serialised by the LDS, which on Gaussian
// gradients costs less than counting them with ballots first (measured, with the forms that lost).
__device__ __forceinline__ void hist_add(unsigned *__restrict__ wave_bins, int bin, bool valid) {
    if (valid) atomicAdd(&wave_bins[bin], 1u);
}

// one element of a tensor; `valid` clear: a lane beyond the chunk, which only keeps the wave together
__device__ __forceinline__ void take1(float g, float p, float m, float v, bool valid, const UCoef &c, TAcc &a,
                                      unsigned *__restrict__ wave_bins) {
    const unsigned ga = __float_as_uint(g) & 0x7fffffffu, pa = __float_as_uint(p) & 0x7fffffffu;
    const bool gfin = ga < 0x7f800000u, pfin = pa < 0x7f800000u;
    if (valid) {
        if (gfin) {
            a.sumsq[0] += (double)g * (double)g;
            a.maxbits[0] = max(a.maxbits[0], ga);
            a.count[1] += ga == 0u;
        } else {
            ++a.count[0];
        }
        if (pfin) {
            a.sumsq[1] += (double)p * (double)p;
            a.maxbits[1] = max(a.maxbits[1], pa);
        } else {
            ++a.count[2];
        }
        const float u = c.stepped ? c.step_size * (m / (sqrtf(v) * c.inv + c.eps)) : 0.0f;        // adam1's term, rounded as adam1 rounds it
        const unsigned ua = __float_as_uint(u) & 0x7fffffffu;
        if (ua < 0x7f800000u) {
            a.sumsq[2] += (double)u * (double)u;
            a.maxbits[2] = max(a.maxbits[2], ua);
        }
    }
    hist_add(wave_bins, bin_of(ga), valid && gfin);
}

__device__ __forceinline__ void take_scalar(const float *__restrict__ g, const float *__restrict__ p, const float *__restrict__ m,
                                            const float *__restrict__ v, int i, bool valid, const UCoef &c, TAcc &a,
                                            unsigned *__restrict__ wave_bins) {
    float gi = 0.0f, pi = 0.0f, mi = 0.0f, vi = 0.0f;
    if (valid) { gi = g[i]; pi = p[i]; mi = m[i]; vi = v[i]; }
    take1(gi, pi, mi, vi, valid, c, a, wave_bins);
}

// The chunks of the table, then the chunks of the watched buffers.  Loads only: g, p, m, v and the words are const here.
__global__ __launch_bounds__(THREADS) void k_tensor_stats(const lav_optim_tensor *__restrict__ table, int ntensors, int total_chunks,
                                                          const lav_optim_watch *__restrict__ watch, int nwatch,
                                                          const lav_optim_state *__restrict__ state, TensorPart *__restrict__ part,
                                                          WatchPart *__restrict__ wpart) {
    __shared__ unsigned s_bins[WAVES][BINS];
    __shared__ double s_sum[3][WAVES];
    __shared__ int s_count[3][WAVES];
    __shared__ unsigned s_max[3][WAVES];
    const int tid = threadIdx.x, chunk = blockIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    if (chunk >= total_chunks) {        // a watched buffer: the count and the maximum alone
        const lav_optim_watch &row = watch[find_row(watch, nwatch, chunk - total_chunks)];
        const long long first = (long long)(chunk - total_chunks - row.chunk0) * OPTIM_CHUNK, left = row.numel - first;
        const int n = left <= 0 ? 0 : (int)(left < OPTIM_CHUNK ? left : OPTIM_CHUNK);
        const float *__restrict__ src = row.data + first;
        int bad = 0;
        unsigned mx = 0;
        auto take = [&](float x) {
            const unsigned xa = __float_as_uint(x) & 0x7fffffffu;
            if (xa < 0x7f800000u) mx = max(mx, xa); else ++bad;
        };
        const int head = head_of(src, n), nv = (n - head) >> 2, tail = head + 4 * nv;
        if (tid < head) take(src[tid]);
        const float4 *s4 = reinterpret_cast<const float4 *>(src + head);
        for (int k = tid; k < nv; k += THREADS) {
            const float4 x = s4[k];
            take(x.x); take(x.y); take(x.z); take(x.w);
        }
        if (tail + tid < n) take(src[tail + tid]);
#pragma unroll
        for (int o = WAVE / 2; o >= 1; o >>= 1) {
            bad += __shfl_down(bad, o, WAVE);
            mx = max(mx, (unsigned)__shfl_down((int)mx, o, WAVE));
        }
        if (lane == 0) { s_count[0][wave] = bad; s_max[0][wave] = mx; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < WAVES; ++w) { bad += s_count[0][w]; mx = max(mx, s_max[0][w]); }
            wpart[chunk - total_chunks].bad = bad;
            wpart[chunk - total_chunks].maxbits = mx;
        }
        return;
    }
    for (int i = tid; i < WAVES * BINS; i += THREADS) (&s_bins[0][0])[i] = 0u;
    __syncthreads();
    const lav_optim_tensor &row = table[find_row(table, ntensors, chunk)];
    const long long first = (long long)(chunk - row.chunk0) * OPTIM_CHUNK, left = row.numel - first;
    const int n = left <= 0 ? 0 : (int)(left < OPTIM_CHUNK ? left : OPTIM_CHUNK);
    const lav_optim_state &st = state[row.state];
    UCoef c;
    c.step_size = st.step_size; c.inv = st.inv_sqrt_bc2; c.eps = (float)row.eps; c.stepped = st.step > 0;
    const float *__restrict__ g = row.g + first;
    const float *__restrict__ p = row.p + first, *__restrict__ m = row.m + first, *__restrict__ v = row.v + first;
    TAcc a = {{0.0, 0.0, 0.0}, {0, 0, 0}, {0u, 0u, 0u}};
    unsigned *wave_bins = s_bins[wave];
    const uintptr_t ap = reinterpret_cast<uintptr_t>(p) & 15;
    const bool same = ap == (reinterpret_cast<uintptr_t>(m) & 15) && ap == (reinterpret_cast<uintptr_t>(v) & 15);
    // every loop below has the same trip count on all lanes (the bounds are the workgroup's)
    if (!same) {
        for (int i0 = 0; i0 < n; i0 += THREADS) take_scalar(g, p, m, v, i0 + tid, i0 + tid < n, c, a, wave_bins);
    } else {
        const bool g16 = (reinterpret_cast<uintptr_t>(g) & 15) == ap;
        const int head = head_of(p, n), nv = (n - head) >> 2, tail = head + 4 * nv;
        if (head > 0) take_scalar(g, p, m, v, tid, tid < head, c, a, wave_bins);
        const float4 *p4 = reinterpret_cast<const float4 *>(p + head), *m4 = reinterpret_cast<const float4 *>(m + head);
        const float4 *v4 = reinterpret_cast<const float4 *>(v + head);
        for (int k0 = 0; k0 < nv; k0 += THREADS) {
            const int k = k0 + tid;
            const bool valid = k < nv;
            float4 gg = {0.0f, 0.0f, 0.0f, 0.0f}, pp = gg, mm = gg, vv = gg;
            if (valid) {
                if (g16) {
                    gg = reinterpret_cast<const float4 *>(g + head)[k];
                } else {
                    const float *gs = g + head + 4 * k;
                    gg.x = gs[0]; gg.y = gs[1]; gg.z = gs[2]; gg.w = gs[3];
                }
                pp = p4[k]; mm = m4[k]; vv = v4[k];
            }
            take1(gg.x, pp.x, mm.x, vv.x, valid, c, a, wave_bins);
            take1(gg.y, pp.y, mm.y, vv.y, valid, c, a, wave_bins);
            take1(gg.z, pp.z, mm.z, vv.z, valid, c, a, wave_bins);
            take1(gg.w, pp.w, mm.w, vv.w, valid, c, a, wave_bins);
        }
        if (tail < n) take_scalar(g, p, m, v, tail + tid, tail + tid < n, c, a, wave_bins);
    }
#pragma unroll
    for (int o = WAVE / 2; o >= 1; o >>= 1) {        // lane l takes lane l + o: a fixed tree
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            a.sumsq[f] += __shfl_down(a.sumsq[f], o, WAVE);
            a.count[f] += __shfl_down(a.count[f], o, WAVE);
            a.maxbits[f] = max(a.maxbits[f], (unsigned)__shfl_down((int)a.maxbits[f], o, WAVE));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            s_sum[f][wave] = a.sumsq[f]; lds_store_fence();       // (no ds_write2_b64: common.hpp)
            s_count[f][wave] = a.count[f];
            s_max[f][wave] = a.maxbits[f];
        }
    }
    __syncthreads();
    TensorPart &out = part[chunk];
    if (tid < 3) {      // the waves in their order
        double s = s_sum[tid][0];
        int n_ = s_count[tid][0];
        unsigned mx = s_max[tid][0];
        for (int w = 1; w < WAVES; ++w) { s += s_sum[tid][w]; n_ += s_count[tid][w]; mx = max(mx, s_max[tid][w]); }
        out.sumsq[tid] = s; out.count[tid] = n_; out.maxbits[tid] = mx;
    }
    if (tid < BINS) {
        unsigned h = 0;
        for (int w = 0; w < WAVES; ++w) h += s_bins[w][tid];
        out.hist[tid] = (unsigned short)h;
    }
}

// One wave per tensor, then one per watched buffer: its chunks' partials in chunk order.  The integers are free of any order: lane b
// sums bin b, eight chunks' loads in flight at a time, and the counts and maxima are taken 64 chunks at a time, a chunk per lane.  The
// sums of squares are staged in LDS 64 chunks at a time and added by lanes 0 .. 2 one after the other, in chunk order.
__global__ __launch_bounds__(WAVE) void k_tensor_reduce(const lav_optim_tensor *__restrict__ table, int ntensors,
                                                        const lav_optim_watch *__restrict__ watch, const TensorPart *__restrict__ part,
                                                        const WatchPart *__restrict__ wpart, lav_optim_tensor_row *__restrict__ rows_out,
                                                        lav_optim_watch_row *__restrict__ watch_out) {
    __shared__ double s_sum[3][WAVE];
    const int lane = threadIdx.x, r = blockIdx.x;
    if (r >= ntensors) {
        const lav_optim_watch &row = watch[r - ntensors];
        const int chunks = (int)((row.numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK);
        long long bad = 0;
        unsigned mx = 0;
        for (int c = lane; c < chunks; c += WAVE) { bad += wpart[row.chunk0 + c].bad; mx = max(mx, wpart[row.chunk0 + c].maxbits); }
#pragma unroll
        for (int o = WAVE / 2; o >= 1; o >>= 1) {
            bad += __shfl_down(bad, o, WAVE);
            mx = max(mx, (unsigned)__shfl_down((int)mx, o, WAVE));
        }
        if (lane == 0) {
            lav_optim_watch_row &out = watch_out[r - ntensors];
            out.nonfinite = bad;
            out.maxabs = __uint_as_float(mx);
            out.reserved = 0;
        }
        return;
    }
    const lav_optim_tensor &row = table[r];
    const int chunks = (int)((row.numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK);
    const TensorPart *__restrict__ q = part + row.chunk0;
    long long h = 0;
    int c = 0;
    for (; c + 8 <= chunks; c += 8) {
        unsigned v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = q[c + j].hist[lane];
#pragma unroll
        for (int j = 0; j < 8; ++j) h += v[j];
    }
    for (; c < chunks; ++c) h += q[c].hist[lane];
    long long n[3] = {0, 0, 0};
    unsigned mx[3] = {0u, 0u, 0u};
    double s = 0.0;
    for (int c0 = 0; c0 < chunks; c0 += WAVE) {
        const int mine = c0 + lane, here = min(WAVE, chunks - c0);
        if (mine < chunks) {
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                s_sum[f][lane] = q[mine].sumsq[f]; lds_store_fence();       // (no ds_write2_b64: common.hpp)
                n[f] += q[mine].count[f];
                mx[f] = max(mx[f], q[mine].maxbits[f]);
            }
        }
        __syncthreads();
        if (lane < 3)
            for (int i = 0; i < here; ++i) s += s_sum[lane][i];
        __syncthreads();
    }
#pragma unroll
    for (int o = WAVE / 2; o >= 1; o >>= 1) {
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            n[f] += __shfl_down(n[f], o, WAVE);
            mx[f] = max(mx[f], (unsigned)__shfl_down((int)mx[f], o, WAVE));
        }
    }
    lav_optim_tensor_row &out = rows_out[r];
    out.hist[lane] = h;
    if (lane == 0) {
        out.g_sumsq = s;
        out.g_nonfinite = n[0]; out.g_zeros = n[1]; out.p_nonfinite = n[2];
        out.g_maxabs = __uint_as_float(mx[0]); out.p_maxabs = __uint_as_float(mx[1]); out.u_maxabs = __uint_as_float(mx[2]);
        out.reserved = 0;
    } else if (lane == 1) {
        out.p_sumsq = s;
    } else if (lane == 2) {
        out.u_sumsq = s;
    }
}

// ---- who caused a skipped step (lav_optim_blame) ---------------------------------------------------------------------------------
// One workgroup.  A round gives every thread one row, whose chunks' counts it adds up; thread 0 then walks the round's rows in table
// order and appends records until it has LAV_OPTIM_BLAME_PER_STEP of them: the ring is a function of the steps alone.
template <class Row>
__device__ __forceinline__ void blame_rows(const Row *__restrict__ rows, int n, const int *__restrict__ part_bad, bool tensors, long long step,
                                           lav_optim_blame_block *__restrict__ blame, long long *s_count, int *s_found) {
    const int tid = threadIdx.x, k = tensors ? 0 : 1;
    if (tid == 0) *s_found = 0;
    __syncthreads();
    for (int r0 = 0; r0 < n; r0 += THREADS) {
        const int r = r0 + tid;
        long long bad = 0;
        if (r < n) {
            const int chunks = (int)((rows[r].numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK);
            for (int c = 0; c < chunks; ++c) bad += part_bad[rows[r].chunk0 + c];
        }
        s_count[tid] = bad;
        __syncthreads();
        if (tid == 0) {
            int found = *s_found;
            long long written = blame->written[k];
            for (int i = 0; i < THREADS && r0 + i < n && found < LAV_OPTIM_BLAME_PER_STEP; ++i) {
                if (s_count[i] == 0) continue;
                lav_optim_blame_record &rec = blame->ring[k][written % LAV_OPTIM_BLAME_RING];
                rec.step = step;
                rec.nonfinite = s_count[i];
                if constexpr (sizeof(Row) == sizeof(lav_optim_tensor)) rec.index = rows[r0 + i].state; else rec.index = r0 + i;
                rec.reserved = 0;
                ++written; ++found;
            }
            blame->written[k] = written;
            *s_found = found;
        }
        __syncthreads();
        if (*s_found >= LAV_OPTIM_BLAME_PER_STEP) break;       // (uniform: thread 0 writes it again only behind the next barrier)
    }
}

__global__ __launch_bounds__(THREADS) void k_optim_blame(const lav_optim_tensor *__restrict__ table, int ntensors, int total_chunks,
                                                         const lav_optim_watch *__restrict__ watch, int nwatch,
                                                         const int *__restrict__ part_bad, const lav_optim_global *__restrict__ global,
                                                         lav_optim_blame_block *__restrict__ blame) {
    __shared__ long long s_count[THREADS];
    __shared__ int s_found;
    if (global->apply) return;
    const long long step = global->applied + global->skipped;
    blame_rows(table, ntensors, part_bad, true, step, blame, s_count, &s_found);
    __syncthreads();
    blame_rows(watch, nwatch, part_bad + total_chunks, false, step, blame, s_count, &s_found);
}

int check_tables(const void *table, int ntensors, int total_chunks, const void *watch, int nwatch, int watch_chunks, bool words,
                 const void *workspace, size_t workspace_bytes, size_t (*needs)(long long, long long)) {
    LAV_REQUIRE(ntensors >= 0 && total_chunks >= 0 && nwatch >= 0 && watch_chunks >= 0, "lav_optim: negative counts");
    LAV_REQUIRE((ntensors == 0) == (total_chunks == 0) && (nwatch == 0) == (watch_chunks == 0), "lav_optim: a table without chunks, or chunks without a table");
    LAV_REQUIRE(total_chunks >= ntensors && watch_chunks >= nwatch, "lav_optim: fewer chunks than rows (a row has at least one element)");
    LAV_REQUIRE((long long)total_chunks + watch_chunks <= 0x7fffffffLL, "lav_optim: %lld chunks", (long long)total_chunks + watch_chunks);
    LAV_REQUIRE((ntensors == 0 || table) && (nwatch == 0 || watch) && words, "lav_optim: null table or words");
    LAV_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "lav_optim: workspace must be 256-byte aligned");
    LAV_REQUIRE(workspace_bytes >= needs(total_chunks, watch_chunks), "lav_optim: workspace of %zu bytes, needs %zu", workspace_bytes,
                needs(total_chunks, watch_chunks));
    return LAV_OK;
}

int check_args(const void *table, int ntensors, int total_chunks, const void *watch, int nwatch, int watch_chunks, const void *global,
               const void *workspace, size_t workspace_bytes) {
    return check_tables(table, ntensors, total_chunks, watch, nwatch, watch_chunks, global != nullptr, workspace, workspace_bytes,
                        lav_optim_workspace_bytes);
}

// the step's per-chunk counts of elements that are not finite, behind its partial sums (run)
const int *part_bad_of(const void *workspace, int chunks) {
    return reinterpret_cast<const int *>(static_cast<const char *>(workspace) + align_up((size_t)std::max(chunks, 1) * sizeof(double), 256));
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

extern "C" size_t lav_optim_tensor_stats_workspace_bytes(long long total_chunks, long long watch_chunks) {
    if (total_chunks < 0 || watch_chunks < 0 || total_chunks + watch_chunks > 0x7fffffffLL) return 0;
    return lav::align_up((size_t)std::max(total_chunks, 1LL) * sizeof(TensorPart), 256) +
           lav::align_up((size_t)std::max(watch_chunks, 1LL) * sizeof(WatchPart), 256);
}

extern "C" int lav_optim_tensor_stats(const lav_optim_tensor *table, int ntensors, int total_chunks, const lav_optim_watch *watch, int nwatch,
                                      int watch_chunks, const lav_optim_state *state, lav_optim_tensor_row *rows_out,
                                      lav_optim_watch_row *watch_out, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_tables(table, ntensors, total_chunks, watch, nwatch, watch_chunks, (ntensors == 0 || (state && rows_out)) && (nwatch == 0 || watch_out),
                              workspace, workspace_bytes, lav_optim_tensor_stats_workspace_bytes))
        return rc;
    LAV_REQUIRE(((reinterpret_cast<uintptr_t>(rows_out) | reinterpret_cast<uintptr_t>(watch_out)) & 7) == 0, "lav_optim_tensor_stats: rows must be 8-byte aligned");
    static_assert(BINS == WAVE, "k_tensor_reduce: a lane per bin");
    if (total_chunks + watch_chunks == 0) return LAV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    TensorPart *part = static_cast<TensorPart *>(workspace);
    WatchPart *wpart = reinterpret_cast<WatchPart *>(static_cast<char *>(workspace) + align_up((size_t)std::max(total_chunks, 1) * sizeof(TensorPart), 256));
    const int tok = timer_begin("optim_tensor_stats", st);          // (lav_profile_read: the pass over the chunks, and the reduction, apart)
    hipLaunchKernelGGL(k_tensor_stats, dim3(total_chunks + watch_chunks), dim3(THREADS), 0, st, table, ntensors, total_chunks, watch, nwatch, state, part, wpart);
    timer_end(tok, st);
    const int tok_reduce = timer_begin("optim_tensor_reduce", st);
    hipLaunchKernelGGL(k_tensor_reduce, dim3(ntensors + nwatch), dim3(WAVE), 0, st, table, ntensors, watch, part, wpart, rows_out, watch_out);
    timer_end(tok_reduce, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}

extern "C" int lav_optim_blame(const lav_optim_tensor *table, int ntensors, int total_chunks, const lav_optim_watch *watch, int nwatch,
                               int watch_chunks, const lav_optim_global *global, lav_optim_blame_block *blame, const void *workspace,
                               size_t workspace_bytes, void *stream) {
    if (int rc = check_tables(table, ntensors, total_chunks, watch, nwatch, watch_chunks, global && blame, workspace, workspace_bytes, lav_optim_workspace_bytes))
        return rc;
    LAV_REQUIRE((reinterpret_cast<uintptr_t>(blame) & 7) == 0, "lav_optim_blame: the block must be 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("optim_blame", st);
    hipLaunchKernelGGL(k_optim_blame, dim3(1), dim3(THREADS), 0, st, table, ntensors, total_chunks, watch, nwatch,
                       part_bad_of(workspace, total_chunks + watch_chunks), global, blame);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
