// Single-query multi-head attention pooling of the brake net (lav/models/attention.py:21-38, called from
// team_code_v2/models/rgb.py:69-70).  gfx950 only.
//
// The module has ONE learned query per head, so both projections fold around it:
//   dots[h][n] = scale * q_h . (W_k,h x_n + b_k,h + PE[n])  =  u_h . x_n + bias[h][n]
//                u_h = scale * W_k,h^T q_h  (heads x C),   bias[h][n] = scale * q_h . (b_k,h + PE[n])
//   out_h      = sum_n softmax(dots[h])[n] (W_v,h x_n + b_v,h)  =  W_v,h (sum_n p[h][n] x_n) + b_v,h
// i.e. two reductions over the map and one 64 x 512 matrix-vector product per head instead of the (N x C) x (C x 2C)
// key/value GEMM: 2 MMAC instead of 113 at the wide view's 216 tokens.  u and bias depend on the weights only and are
// prepared once on the host (lav_amd/rgb.py).  HBM-light (the 442 KB map is read twice from L2, W_v once); one
// 1024-thread workgroup per (head, image): (a) dots (waves split channels x tokens); (b) soft-max over the tokens through LDS;
// (c) the pooled map, two threads per channel; (d) the head's 64 outputs, sixteen lanes per output row of W_v.
//
// Train mode (lav_attn_train_forward / _backward, the brake-net trainer): the same folding, with u and the bias prepared on the
// device from the LIVE q, linear_kv and a device-resident PE table (k_attn_prep), and the forward saving p and the pooled maps.
// The backward, per (image, head), with g = W_v,h^T dout_h, dp_n = g . x_n, dd_n = p_n (dp_n - sum_m p_m dp_m):
//   dx_n = sum_h (p_hn g_h + dd_hn u_h)                          (k_attn_bwd_head, k_attn_bwd_dx: a rank-2H update per image)
//   dW_v,h = sum_b dout_h (x) xbar_h,  db_v = sum_b dout        (k_attn_bwd_batch)
//   dW_k,h = scale q_h (x) R_h,  R_h = sum_b sum_n dd_hn x_n     (k_attn_bwd_key)
//   dq_h = scale (W_k,h R_h + sum_b sum_n dd_hn (b_k,h + PE[n])),  db_k,h = scale q_h sum_b sum_n dd_hn
// Every sum runs in an order fixed by the shape (images in order, fixed wave trees), no atomics: bit-reproducible.
#include "common.hpp"

namespace {
using namespace lav;

constexpr int ATT_THREADS = 1024;      // 16 waves: every phase is a latency chain of L2 loads, so it is cut 16 ways
constexpr int ATT_MAX_TOKENS = 4096;   // tokens of one map (LDS: probabilities)
constexpr int ATT_MAX_C = 1024;        // channels (LDS: pooled map of one head)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

// One workgroup per (head, image).  TRAIN (lav_attn_train_forward): also writes the normalised probabilities p [batch][heads][N]
// and the pooled maps xbar [batch][heads][C] for the backward, and (d) reads W_v with scalar loads (any C that the heads divide).
template <bool TRAIN>
__global__ __launch_bounds__(ATT_THREADS) void k_attn_pool(const float *__restrict__ x, int C, int N, int heads,
                                                           const float *__restrict__ u, const float *__restrict__ bias,
                                                           const float *__restrict__ w_v, const float *__restrict__ b_v,
                                                           float *__restrict__ out, float *__restrict__ p_out, float *__restrict__ xbar_out) {
    __shared__ float prob[ATT_MAX_TOKENS];
    __shared__ float part[4][ATT_MAX_TOKENS];   // (a): partial dots of the four channel quarters
    __shared__ float xbar[ATT_MAX_C];
    __shared__ float red[32];
    const int h = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float *xb = x + (long)b * C * N;
    const float *uh = u + (long)h * C;
    // (a) dots.  Wave (cq, tq): channel quarter cq = wid & 3, tokens tq*64 + lane + 256 i.  Consecutive lanes read
    // consecutive tokens of one channel plane; u_h[c] is wave-uniform (scalar loads); 16 loads in flight per lane.
    {
        const int cq = wid & 3, tq = wid >> 2;
        const int cpq = (C + 3) / 4, c_lo = cq * cpq, c_hi = min(C, c_lo + cpq);
        for (int n = tq * 64 + lane; n < N; n += 256) {
            float acc = 0.f;
#pragma unroll 16
            for (int c = c_lo; c < c_hi; ++c) acc = fmaf(uh[c], xb[(long)c * N + n], acc);
            part[cq][n] = acc;
        }
    }
    __syncthreads();
    // (b) soft-max over the tokens
    float mx = -INFINITY;
    for (int n = tid; n < N; n += ATT_THREADS) {
        const float d = ((part[0][n] + part[1][n]) + (part[2][n] + part[3][n])) + bias[(long)h * N + n];
        prob[n] = d;
        mx = fmaxf(mx, d);
    }
    mx = wave_max(mx);
    if (lane == 0) red[wid] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int w = 1; w < ATT_THREADS / 64; ++w) mx = fmaxf(mx, red[w]);
    float sum = 0.f;
    for (int n = tid; n < N; n += ATT_THREADS) {
        const float e = expf(prob[n] - mx);
        prob[n] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    __syncthreads();
    if (lane == 0) red[16 + wid] = sum;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < ATT_THREADS / 64; ++w) tot += red[16 + w];
    const float inv = 1.f / tot;
    if (TRAIN) {
        float *pb = p_out + ((long)b * heads + h) * N;
        for (int n = tid; n < N; n += ATT_THREADS) pb[n] = prob[n] * inv;
    }
    // (c) pooled map of this head: xbar[c] = sum_n p[n] x[c][n]; two threads per channel walk its token row (L1 lines are
    // consumed whole over the iterations), p[n] is an LDS broadcast
    for (int c0 = 0; c0 < C; c0 += ATT_THREADS / 2) {
        const int c = c0 + (tid >> 1), halfn = tid & 1;
        float acc = 0.f;
        if (c < C) {
            const float *xr = xb + (long)c * N;
            const int n_mid = (N / 2) & ~3, n_lo = halfn ? n_mid : 0, n_hi = halfn ? N : n_mid;
            int n = n_lo;
            if ((reinterpret_cast<uintptr_t>(xr) & 15) == 0) {
#pragma unroll 8
                for (; n + 4 <= n_hi; n += 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(xr + n);
                    acc = fmaf(prob[n], v.x, acc);
                    acc = fmaf(prob[n + 1], v.y, acc);
                    acc = fmaf(prob[n + 2], v.z, acc);
                    acc = fmaf(prob[n + 3], v.w, acc);
                }
            }
            for (; n < n_hi; ++n) acc = fmaf(prob[n], xr[n], acc);
        }
        acc += __shfl_xor(acc, 1, 64);
        if (c < C && halfn == 0) {
            xbar[c] = acc * inv;
            if (TRAIN) xbar_out[((long)b * heads + h) * C + c] = acc * inv;
        }
    }
    __syncthreads();
    // (d) the head's outputs: row h*dh + d of W_v against xbar, sixteen lanes per row (each a contiguous 1/16 of the row)
    const int dh = C / heads;
    for (int d0 = 0; d0 < dh; d0 += ATT_THREADS / 16) {
        const int d = d0 + (tid >> 4), seg = tid & 15;
        float acc = 0.f;
        if (d < dh && TRAIN) {
            const float *wr = w_v + (long)(h * dh + d) * C;
            for (int c = seg; c < C; c += 16) acc = fmaf(wr[c], xbar[c], acc);
        } else if (d < dh) {
            const float *wr = w_v + (long)(h * dh + d) * C;
            for (int c = seg * 4; c < C; c += 64) {
                const float4 w4 = *reinterpret_cast<const float4 *>(wr + c);
                acc = fmaf(w4.x, xbar[c], acc);
                acc = fmaf(w4.y, xbar[c + 1], acc);
                acc = fmaf(w4.z, xbar[c + 2], acc);
                acc = fmaf(w4.w, xbar[c + 3], acc);
            }
        }
#pragma unroll
        for (int sft = 1; sft < 16; sft <<= 1) acc += __shfl_xor(acc, sft, 64);
        if (d < dh && seg == 0) out[(long)b * C + h * dh + d] = acc + b_v[h * dh + d];
    }
}

// ------------------------------------------------------------------------------------------ train mode (lav_attn_train_*)
constexpr int AT_THREADS = 256;

__device__ __forceinline__ float block4_sum(float v, float *red) {   // 4 waves; every thread gets the sum, in a fixed order
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// u [heads][C] = scale W_k,h^T q_h and bias [heads][N] = scale q_h . (b_k,h + pe[n]) from the live parameters (one thread per value)
__global__ __launch_bounds__(AT_THREADS) void k_attn_prep(const float *__restrict__ q, const float *__restrict__ w_kv,
                                                          const float *__restrict__ b_kv, const float *__restrict__ pe, int C, int N,
                                                          int heads, float scale, float *__restrict__ u, float *__restrict__ bias) {
    const int dh = C / heads;
    const long i = (long)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i < (long)heads * C) {
        const int h = (int)(i / C), c = (int)(i - (long)h * C);
        float acc = 0.f;
        for (int d = 0; d < dh; ++d) acc = fmaf(q[h * dh + d], w_kv[(long)(h * dh + d) * C + c], acc);   // coalesced along c
        u[i] = scale * acc;
        return;
    }
    const long j = i - (long)heads * C;
    if (j >= (long)heads * N) return;
    const int h = (int)(j / N), n = (int)(j - (long)h * N);
    float acc = 0.f;
    for (int d = 0; d < dh; ++d) acc = fmaf(q[h * dh + d], b_kv[h * dh + d] + pe[(long)n * dh + d], acc);
    bias[j] = scale * acc;
}

// Per (head, image): g = W_v,h^T dout_h, dp_n = g . x_n, dd_n = p_n (dp_n - sum_m p_m dp_m), r = sum_n dd_n x_n.
// Writes g [batch][heads][C], dd [batch][heads][N], r [batch][heads][C].
__global__ __launch_bounds__(AT_THREADS) void k_attn_bwd_head(const float *__restrict__ x, int C, int N, int heads,
                                                              const float *__restrict__ w_v, const float *__restrict__ dout,
                                                              const float *__restrict__ p, float *__restrict__ g_out,
                                                              float *__restrict__ dd_out, float *__restrict__ r_out) {
    __shared__ float gs[ATT_MAX_C];
    __shared__ float dd[ATT_MAX_TOKENS];
    __shared__ float red[4];
    const int h = blockIdx.x, b = blockIdx.y, dh = C / heads;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long bh = (long)b * heads + h;
    const float *xb = x + (long)b * C * N, *pb = p + bh * N, *db = dout + (long)b * C + h * dh;
    for (int c = tid; c < C; c += AT_THREADS) {
        float acc = 0.f;
        for (int d = 0; d < dh; ++d) acc = fmaf(w_v[(long)(h * dh + d) * C + c], db[d], acc);
        gs[c] = acc;
        g_out[bh * C + c] = acc;
    }
    __syncthreads();
    float sp = 0.f;
    for (int n = tid; n < N; n += AT_THREADS) {          // consecutive lanes read consecutive tokens of one channel plane
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = fmaf(gs[c], xb[(long)c * N + n], acc);
        dd[n] = acc;
        sp = fmaf(pb[n], acc, sp);
    }
    const float s = block4_sum(sp, red);
    for (int n = tid; n < N; n += AT_THREADS) {          // (the same thread wrote dd[n] above)
        const float v = pb[n] * (dd[n] - s);
        dd[n] = v;
        dd_out[bh * N + n] = v;
    }
    __syncthreads();
    for (int c = wid; c < C; c += AT_THREADS / 64) {     // one wave per channel, lanes along its token row
        const float *xr = xb + (long)c * N;
        float acc = 0.f;
        for (int n = lane; n < N; n += 64) acc = fmaf(dd[n], xr[n], acc);
        acc = wave_sum(acc);
        if (lane == 0) r_out[bh * C + c] = acc;
    }
}

// dx[b][c][n] = sum_h (p[b][h][n] g[b][h][c] + dd[b][h][n] u[h][c]), heads in order
__global__ __launch_bounds__(AT_THREADS) void k_attn_bwd_dx(int batch, int C, int N, int heads, const float *__restrict__ p,
                                                            const float *__restrict__ g, const float *__restrict__ dd,
                                                            const float *__restrict__ u, float *__restrict__ dx) {
    const long total = (long)batch * C * N, plane = (long)C * N;
    for (long i = (long)blockIdx.x * AT_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * AT_THREADS) {
        const long b = i / plane, rem = i - b * plane;
        const int c = (int)(rem / N), n = (int)(rem - (long)c * N);
        float acc = 0.f;
        for (int h = 0; h < heads; ++h) {
            const long bh = b * heads + h;
            acc = fmaf(p[bh * N + n], g[bh * C + c], acc);
            acc = fmaf(dd[bh * N + n], u[(long)h * C + c], acc);
        }
        dx[i] = acc;
    }
}

// Sums over the batch, images in order: dW_v, db_v (into the value half of dw_kv / db_kv), R [heads][C] = sum_b r, D [heads][N] = sum_b dd
__global__ __launch_bounds__(AT_THREADS) void k_attn_bwd_batch(int batch, int C, int N, int heads, const float *__restrict__ dout,
                                                               const float *__restrict__ xbar, const float *__restrict__ r,
                                                               const float *__restrict__ dd, float *__restrict__ dw_kv,
                                                               float *__restrict__ db_kv, float *__restrict__ R, float *__restrict__ D) {
    const int dh = C / heads;
    const long nw = (long)C * C, nb = C, nr = (long)heads * C, nd = (long)heads * N;
    long i = (long)blockIdx.x * AT_THREADS + threadIdx.x;
    float acc = 0.f;
    if (i < nw) {
        const int o = (int)(i / C), c = (int)(i - (long)o * C), h = o / dh;
        for (int b = 0; b < batch; ++b) acc = fmaf(dout[(long)b * C + o], xbar[((long)b * heads + h) * C + c], acc);
        dw_kv[nw + i] = acc;
        return;
    }
    i -= nw;
    if (i < nb) {
        for (int b = 0; b < batch; ++b) acc += dout[(long)b * C + i];
        db_kv[C + i] = acc;
        return;
    }
    i -= nb;
    if (i < nr) {
        const int h = (int)(i / C), c = (int)(i - (long)h * C);
        for (int b = 0; b < batch; ++b) acc += r[((long)b * heads + h) * C + c];
        R[i] = acc;
        return;
    }
    i -= nr;
    if (i < nd) {
        const int h = (int)(i / N), n = (int)(i - (long)h * N);
        for (int b = 0; b < batch; ++b) acc += dd[((long)b * heads + h) * N + n];
        D[i] = acc;
    }
}

// The key half and the query: one wave per key row o = h*dh + d.
//   dW_k[o][c] = scale q[o] R[h][c],   db_k[o] = scale q[o] S_h,   dq[o] = scale (W_k[o] . R[h] + b_k[o] S_h + sum_n D[h][n] pe[n][d])
// with S_h = sum_n D[h][n]
__global__ __launch_bounds__(AT_THREADS) void k_attn_bwd_key(int C, int N, int heads, float scale, const float *__restrict__ q,
                                                             const float *__restrict__ w_kv, const float *__restrict__ b_kv,
                                                             const float *__restrict__ pe, const float *__restrict__ R,
                                                             const float *__restrict__ D, float *__restrict__ dq,
                                                             float *__restrict__ dw_kv, float *__restrict__ db_kv) {
    const int lane = threadIdx.x & 63, o = blockIdx.x * (AT_THREADS / 64) + (threadIdx.x >> 6);
    if (o >= C) return;                                  // (wave-uniform)
    const int dh = C / heads, h = o / dh, d = o - h * dh;
    const float qo = q[o];
    const float *Rh = R + (long)h * C, *Dh = D + (long)h * N, *wk = w_kv + (long)o * C;
    float aw = 0.f, as = 0.f, ap = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float rv = Rh[c];
        dw_kv[(long)o * C + c] = scale * qo * rv;
        aw = fmaf(wk[c], rv, aw);
    }
    for (int n = lane; n < N; n += 64) {
        const float dv = Dh[n];
        as += dv;
        ap = fmaf(dv, pe[(long)n * dh + d], ap);
    }
    aw = wave_sum(aw);
    as = wave_sum(as);
    ap = wave_sum(ap);
    if (lane == 0) {
        dq[o] = scale * (aw + fmaf(b_kv[o], as, ap));
        db_kv[o] = scale * qo * as;
    }
}

int attn_train_check(int batch, int C, int N, int heads, const char *who) {
    LAV_REQUIRE(batch >= 1 && batch <= 65535 && heads >= 1 && heads <= 65535, "%s: batch %d, heads %d", who, batch, heads);
    LAV_REQUIRE(C >= heads && C % heads == 0 && (C / heads) % 2 == 0 && C <= ATT_MAX_C,
                "%s: channels %d unsupported (an even multiple of the %d heads, <= %d)", who, C, heads, ATT_MAX_C);
    LAV_REQUIRE(N >= 1 && N <= ATT_MAX_TOKENS, "%s: %d tokens unsupported (<= %d)", who, N, ATT_MAX_TOKENS);
    LAV_REQUIRE((long)batch * C * N < (1L << 40), "%s: map too large", who);
    return LAV_OK;
}

unsigned grid_of(long n) { return (unsigned)std::max<long>(1, std::min<long>((n + AT_THREADS - 1) / AT_THREADS, 1L << 20)); }
}  // namespace

extern "C" int lav_attn_pool(const float *x, int batch, int C, int N, int heads, const float *u, const float *dots_bias,
                             const float *w_v, const float *b_v, float *out, void *stream) {
    LAV_REQUIRE(x && u && dots_bias && w_v && b_v && out, "lav_attn_pool: null argument");
    LAV_REQUIRE(batch >= 1 && batch <= 65535 && heads >= 1 && heads <= 65535, "lav_attn_pool: bad batch / heads");
    LAV_REQUIRE(C >= heads && C % heads == 0 && C % 16 == 0 && C <= ATT_MAX_C, "lav_attn_pool: channels %d unsupported (multiple of 16 and of the heads, <= %d)", C, ATT_MAX_C);
    LAV_REQUIRE(N >= 1 && N <= ATT_MAX_TOKENS, "lav_attn_pool: %d tokens unsupported (<= %d)", N, ATT_MAX_TOKENS);
    hipLaunchKernelGGL(k_attn_pool<false>, dim3(heads, batch), dim3(ATT_THREADS), 0, static_cast<hipStream_t>(stream), x, C, N, heads, u,
                       dots_bias, w_v, b_v, out, nullptr, nullptr);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}

extern "C" size_t lav_attn_train_workspace_bytes(int batch, int C, int N, int heads) {
    if (batch < 1 || C < 1 || N < 1 || heads < 1) return 0;
    const size_t bh = (size_t)batch * heads;
    return (bh * (2 * (size_t)C + N) + (size_t)heads * (C + N)) * sizeof(float);    // g, r, dd | R, D
}

extern "C" int lav_attn_train_forward(const float *x, int batch, int C, int N, int heads, const float *q, const float *w_kv,
                                      const float *b_kv, const float *pe, float scale, float *u, float *dots_bias, float *out,
                                      float *p, float *xbar, void *stream) {
    LAV_REQUIRE(x && q && w_kv && b_kv && pe && u && dots_bias && out && p && xbar, "lav_attn_train_forward: null argument");
    if (int rc = attn_train_check(batch, C, N, heads, "lav_attn_train_forward")) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("attn_train_fwd", st);
    hipLaunchKernelGGL(k_attn_prep, dim3(grid_of((long)heads * (C + N))), dim3(AT_THREADS), 0, st, q, w_kv, b_kv, pe, C, N, heads, scale,
                       u, dots_bias);
    hipLaunchKernelGGL(k_attn_pool<true>, dim3(heads, batch), dim3(ATT_THREADS), 0, st, x, C, N, heads, u, dots_bias, w_kv + (long)C * C,
                       b_kv + C, out, p, xbar);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}

extern "C" int lav_attn_train_backward(const float *x, int batch, int C, int N, int heads, const float *q, const float *w_kv,
                                       const float *b_kv, const float *pe, float scale, const float *u, const float *p, const float *xbar,
                                       const float *dout, float *dx, float *dq, float *dw_kv, float *db_kv, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    LAV_REQUIRE(x && q && w_kv && b_kv && pe && u && p && xbar && dout && dx && dq && dw_kv && db_kv && workspace,
                "lav_attn_train_backward: null argument");
    if (int rc = attn_train_check(batch, C, N, heads, "lav_attn_train_backward")) return rc;
    LAV_REQUIRE(workspace_bytes >= lav_attn_train_workspace_bytes(batch, C, N, heads),
                "lav_attn_train_backward: workspace smaller than lav_attn_train_workspace_bytes");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long bh = (long)batch * heads;
    float *g = static_cast<float *>(workspace), *r = g + bh * C, *dd = r + bh * C, *R = dd + bh * N, *D = R + (long)heads * C;
    const int tok = timer_begin("attn_train_bwd", st);
    hipLaunchKernelGGL(k_attn_bwd_head, dim3(heads, batch), dim3(AT_THREADS), 0, st, x, C, N, heads, w_kv + (long)C * C, dout, p, g, dd, r);
    hipLaunchKernelGGL(k_attn_bwd_dx, dim3(grid_of((long)batch * C * N)), dim3(AT_THREADS), 0, st, batch, C, N, heads, p, g, dd, u, dx);
    hipLaunchKernelGGL(k_attn_bwd_batch, dim3(grid_of((long)C * C + C + (long)heads * (C + N))), dim3(AT_THREADS), 0, st, batch, C, N,
                       heads, dout, xbar, r, dd, dw_kv, db_kv, R, D);
    hipLaunchKernelGGL(k_attn_bwd_key, dim3((unsigned)((C + AT_THREADS / 64 - 1) / (AT_THREADS / 64))), dim3(AT_THREADS), 0, st, C, N,
                       heads, scale, q, w_kv, b_kv, pe, R, D, dq, dw_kv, db_kv);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
