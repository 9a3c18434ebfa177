// Train mode of ERFNet's factorised convolution pairs (non_bottleneck_1d, lav/models/erfnet.py) and the segmenter's loss.
// gfx950 only.  NCHW float32, every product and sum in fp32 FMA (no operand splitting: the results are within the
// 2e-6 * sum|a||b| bar of the fp16-piece kernels without needing a bound per tensor).
//
// One pair is  t = relu(conv3x1_d(x) + ba),  z = conv1x3_d(t) + bb  with dilation d (1 for the first pair of a block) and
// weights Wa = conv3x1.weight [C][C][3][1], Wb = conv1x3.weight [C][C][1][3] read in PyTorch's layout (no repack).
//
//   lav_pair_train_forward   k_pair_fwd      one workgroup per image row (b, h): t's row from three rows of x (global,
//                                            coalesced along w), kept in LDS, then z's row from it.  Writes t and z.
//   lav_pair_train_backward  k_pair_dt       per row: dt = [t > 0] * conv1x3_d^T(dz)           (dz's row in LDS)
//                            k_pair_dx       per row: dx = conv3x1_d^T(dt)                      (three rows of dt)
//                            k_pair_wgrad x2 dWb, dbb from (dz, t) and dWa, dba from (dt, x): each workgroup sums a fixed
//                                            group of rows for a tile of 8 output channels into its own partial slot
//                            k_pair_reduce   partial slots summed in slot order
//   lav_seg_xent_forward     k_xent          per pixel softmax cross-entropy (classes <= 8, labels in [0, classes)), dlogits = (softmax - onehot) / N,
//                                            per-workgroup float64 partial sums of the loss
//                            k_xent_final    partials summed in order by one workgroup
//   lav_seg_xent_up_forward  k_xent_up       the same loss on the nearest s x-upsampled logits (the brake net's seg head), one thread per
//                                            low-resolution cell from the label histogram of its s x s block; k_xent_final as above
//
// No float atomics anywhere: every sum is taken in an order fixed by the shape, so the results are bit-reproducible.
// Shapes: (channels, width) in {(16, 128), (64, 64), (128, 32)} (ERFNet's stages on 256-pixel-wide images), any batch and
// any number of rows.
#include "common.hpp"

namespace {
using namespace lav;

constexpr int PT_THREADS = 256;
constexpr int WG_TILE = 8;          // output channels per weight-gradient workgroup
constexpr int WG_MAX_GROUPS = 128;  // row groups of the weight gradients (partial slots)
constexpr int XENT_MAX_C = 8;
constexpr int XENT_GROUPS = 1024;

struct PairGeom {
    int B, H, d;
};

__device__ __forceinline__ size_t at(int b, int c, int h, int w, int C, int H, int W) {
    return (((size_t)b * C + c) * H + h) * W + w;
}

// t and z of row (b, h).  Thread tid owns column w = tid % W and channels c0 + j * CS (CS = 256 / W): every value it reads
// from x or t serves all of its NC outputs.
template <int C, int W>
__global__ __launch_bounds__(PT_THREADS) void k_pair_fwd(PairGeom g, const float *__restrict__ x, const float *__restrict__ wa,
                                                         const float *__restrict__ ba, const float *__restrict__ wb,
                                                         const float *__restrict__ bb, float *__restrict__ t, float *__restrict__ z) {
    constexpr int CS = PT_THREADS / W, NC = C * W / PT_THREADS;
    static_assert(PT_THREADS % W == 0 && (C * W) % PT_THREADS == 0, "shape");
    __shared__ float ts[C * W];
    const int row = blockIdx.x, b = row / g.H, h = row - b * g.H;
    const int w = threadIdx.x % W, c0 = threadIdx.x / W;
    float acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = ba[c0 + j * CS];
    for (int k = 0; k < 3; ++k) {
        const int hh = h + (k - 1) * g.d;
        if (hh < 0 || hh >= g.H) continue;
        for (int ci = 0; ci < C; ++ci) {
            const float xv = x[at(b, ci, hh, w, C, g.H, W)];
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[j] = fmaf(wa[((c0 + j * CS) * C + ci) * 3 + k], xv, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = c0 + j * CS;
        const float v = relu_nan(acc[j]);
        ts[c * W + w] = v;
        t[at(b, c, h, w, C, g.H, W)] = v;
        acc[j] = bb[c];
    }
    __syncthreads();
    for (int k = 0; k < 3; ++k) {
        const int ww = w + (k - 1) * g.d;
        if (ww < 0 || ww >= W) continue;
        for (int ci = 0; ci < C; ++ci) {
            const float tv = ts[ci * W + ww];
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[j] = fmaf(wb[((c0 + j * CS) * C + ci) * 3 + k], tv, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) z[at(b, c0 + j * CS, h, w, C, g.H, W)] = acc[j];
}

// dt[ci][w] = [t > 0] * sum_{c, k} Wb[c][ci][k] dz[c][w - (k - 1) d]
template <int C, int W>
__global__ __launch_bounds__(PT_THREADS) void k_pair_dt(PairGeom g, const float *__restrict__ dz, const float *__restrict__ t,
                                                        const float *__restrict__ wb, float *__restrict__ dt) {
    constexpr int CS = PT_THREADS / W, NC = C * W / PT_THREADS;
    __shared__ float zs[C * W];
    const int row = blockIdx.x, b = row / g.H, h = row - b * g.H;
    const int w = threadIdx.x % W, c0 = threadIdx.x / W;
#pragma unroll
    for (int j = 0; j < NC; ++j) zs[(c0 + j * CS) * W + w] = dz[at(b, c0 + j * CS, h, w, C, g.H, W)];
    __syncthreads();
    float acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0.f;
    for (int k = 0; k < 3; ++k) {
        const int ww = w - (k - 1) * g.d;
        if (ww < 0 || ww >= W) continue;
        for (int c = 0; c < C; ++c) {
            const float gv = zs[c * W + ww];
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[j] = fmaf(wb[(c * C + c0 + j * CS) * 3 + k], gv, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const size_t i = at(b, c0 + j * CS, h, w, C, g.H, W);
        dt[i] = t[i] > 0.f ? acc[j] : 0.f;
    }
}

// dx[ci][h][w] = sum_{c, k} Wa[c][ci][k] dt[c][h - (k - 1) d][w]
template <int C, int W>
__global__ __launch_bounds__(PT_THREADS) void k_pair_dx(PairGeom g, const float *__restrict__ dt, const float *__restrict__ wa,
                                                        float *__restrict__ dx) {
    constexpr int CS = PT_THREADS / W, NC = C * W / PT_THREADS;
    const int row = blockIdx.x, b = row / g.H, h = row - b * g.H;
    const int w = threadIdx.x % W, c0 = threadIdx.x / W;
    float acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0.f;
    for (int k = 0; k < 3; ++k) {
        const int hh = h - (k - 1) * g.d;
        if (hh < 0 || hh >= g.H) continue;
        for (int c = 0; c < C; ++c) {
            const float gv = dt[at(b, c, hh, w, C, g.H, W)];
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[j] = fmaf(wa[(c * C + c0 + j * CS) * 3 + k], gv, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) dx[at(b, c0 + j * CS, h, w, C, g.H, W)] = acc[j];
}

// Weight and bias gradient partials of one conv of the pair: workgroup (group, tile) sums rows [group * per, (group + 1) * per)
// of   dW[co][ci][k] += sum_w A[co][h][w] * S[ci][h'][w']   db[co] += sum_w A[co][h][w]
// VERT (conv3x1): h' = h + (k - 1) d, w' = w;  else (conv1x3): h' = h, w' = w + (k - 1) d;  S = 0 outside the map.
// partial[group][C * C * 3 + C]: the weight entries, then the biases.
template <int C, int W, bool VERT>
__global__ __launch_bounds__(PT_THREADS) void k_pair_wgrad(PairGeom g, const float *__restrict__ A, const float *__restrict__ S, int per,
                                                           float *__restrict__ partial) {
    constexpr int NE = WG_TILE * C * 3, NA = (NE + PT_THREADS - 1) / PT_THREADS, NS = VERT ? 3 : 1;
    __shared__ float as[WG_TILE * W];
    constexpr int SP = W + 1;           // row pitch of the S tile: lanes of a wave read different (k, ci) rows at one w - an odd pitch
                                        // spreads them over the 64 banks (a pitch of W put them all on one or two)
    __shared__ float ss[NS * C * SP];
    const int group = blockIdx.x, tile = blockIdx.y, rows = g.B * g.H;
    const int r0 = group * per, r1 = min(r0 + per, rows);
    float acc[NA];
    int e_co[NA], e_ci[NA], e_k[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int e = threadIdx.x + j * PT_THREADS, ee = e < NE ? e : 0;
        acc[j] = 0.f;
        e_co[j] = ee / (C * 3);
        e_ci[j] = (ee / 3) % C;
        e_k[j] = ee % 3;
    }
    float bacc = 0.f;
    for (int r = r0; r < r1; ++r) {
        const int b = r / g.H, h = r - b * g.H;
        __syncthreads();                 // (the previous row's reads of the LDS tiles are done)
        for (int i = threadIdx.x; i < WG_TILE * W; i += PT_THREADS) {
            const int co = i / W, w = i - co * W;
            as[i] = A[at(b, tile * WG_TILE + co, h, w, C, g.H, W)];
        }
        for (int i = threadIdx.x; i < NS * C * W; i += PT_THREADS) {
            const int s = i / (C * W), rem = i - s * C * W, ci = rem / W, w = rem - ci * W;
            const int hh = VERT ? h + (s - 1) * g.d : h;
            ss[(s * C + ci) * SP + w] = (hh >= 0 && hh < g.H) ? S[at(b, ci, hh, w, C, g.H, W)] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            if (threadIdx.x + j * PT_THREADS >= NE) continue;
            const float *a = as + e_co[j] * W;
            float v = acc[j];
            if (VERT) {
                const float *s = ss + (e_k[j] * C + e_ci[j]) * SP;
                for (int w = 0; w < W; ++w) v = fmaf(a[w], s[w], v);
            } else {
                const int sh = (e_k[j] - 1) * g.d, lo = max(0, -sh), hi = min(W, W - sh);
                const float *s = ss + e_ci[j] * SP + sh;
                for (int w = lo; w < hi; ++w) v = fmaf(a[w], s[w], v);
            }
            acc[j] = v;
        }
        if (threadIdx.x < WG_TILE) {
            const float *a = as + threadIdx.x * W;
            for (int w = 0; w < W; ++w) bacc += a[w];
        }
    }
    float *out = partial + (size_t)group * (C * C * 3 + C);
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        if (threadIdx.x + j * PT_THREADS >= NE) continue;
        out[((tile * WG_TILE + e_co[j]) * C + e_ci[j]) * 3 + e_k[j]] = acc[j];
    }
    if (threadIdx.x < WG_TILE) out[C * C * 3 + tile * WG_TILE + threadIdx.x] = bacc;
}

// out_w[i] / out_b[i - nw] = sum over slots, in slot order
__global__ __launch_bounds__(PT_THREADS) void k_pair_reduce(const float *__restrict__ partial, int groups, int nw, int nb,
                                                            float *__restrict__ out_w, float *__restrict__ out_b) {
    const int i = blockIdx.x * PT_THREADS + threadIdx.x, n = nw + nb;
    if (i >= n) return;
    float s = 0.f;
    for (int gi = 0; gi < groups; ++gi) s += partial[(size_t)gi * n + i];
    if (i < nw) out_w[i] = s;
    else out_b[i - nw] = s;
}

// sum over the workgroup's 256 threads in a fixed tree order; result in thread 0
__device__ __forceinline__ double block_sum(double v, double *lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = PT_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    return lds[0];
}

__global__ __launch_bounds__(PT_THREADS) void k_xent(const float *__restrict__ logits, const long long *__restrict__ labels, int B, int NC,
                                                     long plane, float inv_n, float *__restrict__ dlogits, double *__restrict__ partial) {
    __shared__ double lds[PT_THREADS];
    const long n = (long)B * plane;
    double sum = 0.0;
    for (long p = (long)blockIdx.x * PT_THREADS + threadIdx.x; p < n; p += (long)gridDim.x * PT_THREADS) {
        const long b = p / plane, s = p - b * plane;
        const float *lg = logits + b * NC * plane + s;
        float v[XENT_MAX_C];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < XENT_MAX_C; ++c) {
            v[c] = c < NC ? lg[c * plane] : -INFINITY;
            m = fmaxf(m, v[c]);
        }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < XENT_MAX_C; ++c) {
            v[c] = c < NC ? expf(v[c] - m) : 0.f;
            se += v[c];
        }
        const long long lab = labels[p];
        const bool ok = lab >= 0 && lab < NC;        // (memory safety only: the caller guarantees labels in [0, classes), lav_amd.h)
        const int li = ok ? (int)lab : 0;
        const float lse = m + logf(se), rse = 1.f / se;
        float xl = 0.f;
        float *dl = dlogits + b * NC * plane + s;
#pragma unroll
        for (int c = 0; c < XENT_MAX_C; ++c) {
            if (c < NC) {
                if (c == li) xl = lg[c * plane];
                dl[c * plane] = (v[c] * rse - (ok && c == li ? 1.f : 0.f)) * inv_n;
            }
        }
        if (ok) sum += (double)lse - (double)xl;
    }
    const double tot = block_sum(sum, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(PT_THREADS) void k_xent_final(const double *__restrict__ partial, int groups, double inv_n, float *__restrict__ loss) {
    __shared__ double lds[PT_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < groups; i += PT_THREADS) s += partial[i];
    const double tot = block_sum(s, lds);
    if (threadIdx.x == 0) loss[0] = (float)(tot * inv_n);
}

// F.cross_entropy(F.interpolate(logits, scale_factor=s), labels) without the upsampled map: inside one s x s block the logits are
// constant, so one thread per low-resolution cell takes the block's label histogram cnt and adds s^2 lse - sum_k cnt_k logit_k to
// the loss; dlogits = (s^2 softmax - cnt) / N (N = batch * s^2 * plane)
template <typename L>
__global__ __launch_bounds__(PT_THREADS) void k_xent_up(const float *__restrict__ logits, const L *__restrict__ labels, int B, int NC, int h,
                                                        int w, int s, float inv_n, float *__restrict__ dlogits, double *__restrict__ partial) {
    __shared__ double lds[PT_THREADS];
    const long plane = (long)h * w, n = (long)B * plane, Wf = (long)w * s, Pf = plane * s * s;
    const float s2 = (float)(s * s);
    double sum = 0.0;
    for (long p = (long)blockIdx.x * PT_THREADS + threadIdx.x; p < n; p += (long)gridDim.x * PT_THREADS) {
        const long b = p / plane, cell = p - b * plane, i = cell / w, j = cell - i * w;
        const float *lg = logits + b * NC * plane + cell;
        float v[XENT_MAX_C], e[XENT_MAX_C], cnt[XENT_MAX_C];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < XENT_MAX_C; ++c) {
            v[c] = c < NC ? lg[c * plane] : -INFINITY;
            m = fmaxf(m, v[c]);
            cnt[c] = 0.f;
        }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < XENT_MAX_C; ++c) {
            e[c] = c < NC ? expf(v[c] - m) : 0.f;
            se += e[c];
        }
        const L *lb = labels + b * Pf + i * s * Wf + j * s;
        for (int di = 0; di < s; ++di)
            for (int dj = 0; dj < s; ++dj) {
                const long long lab = (long long)lb[di * Wf + dj];      // (a label outside [0, classes) counts nowhere: memory safety only)
#pragma unroll
                for (int c = 0; c < XENT_MAX_C; ++c) cnt[c] += lab == c ? 1.f : 0.f;
            }
        const float lse = m + logf(se), rse = 1.f / se;
        double cl = (double)s2 * (double)lse;
        float *dl = dlogits + b * NC * plane + cell;
#pragma unroll
        for (int c = 0; c < XENT_MAX_C; ++c) {
            if (c < NC) {
                cl -= (double)cnt[c] * (double)v[c];
                dl[c * plane] = (s2 * (e[c] * rse) - cnt[c]) * inv_n;
            }
        }
        sum += cl;
    }
    const double tot = block_sum(sum, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

int wgrad_groups(int rows) { return std::max(1, std::min(rows, WG_MAX_GROUPS)); }

template <int C, int W>
int launch_fwd(PairGeom g, const float *x, const float *wa, const float *ba, const float *wb, const float *bb, float *t, float *z,
               hipStream_t st) {
    hipLaunchKernelGGL((k_pair_fwd<C, W>), dim3((unsigned)(g.B * g.H)), dim3(PT_THREADS), 0, st, g, x, wa, ba, wb, bb, t, z);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}

template <int C, int W>
int launch_bwd(PairGeom g, const float *x, const float *t, const float *dz, const float *wa, const float *wb, float *dt, float *dx,
               float *dwa, float *dba, float *dwb, float *dbb, float *partial, hipStream_t st) {
    const int rows = g.B * g.H, groups = wgrad_groups(rows), per = (rows + groups - 1) / groups;
    const int n = C * C * 3 + C;
    float *pb = partial, *pa = partial + (size_t)groups * n;
    const dim3 rgrid((unsigned)rows), wgrid((unsigned)groups, (unsigned)(C / WG_TILE)), ngrid((unsigned)((n + PT_THREADS - 1) / PT_THREADS));
    hipLaunchKernelGGL((k_pair_dt<C, W>), rgrid, dim3(PT_THREADS), 0, st, g, dz, t, wb, dt);
    hipLaunchKernelGGL((k_pair_wgrad<C, W, false>), wgrid, dim3(PT_THREADS), 0, st, g, dz, t, per, pb);
    hipLaunchKernelGGL((k_pair_dx<C, W>), rgrid, dim3(PT_THREADS), 0, st, g, dt, wa, dx);
    hipLaunchKernelGGL((k_pair_wgrad<C, W, true>), wgrid, dim3(PT_THREADS), 0, st, g, dt, x, per, pa);
    hipLaunchKernelGGL(k_pair_reduce, ngrid, dim3(PT_THREADS), 0, st, pb, groups, C * C * 3, C, dwb, dbb);
    hipLaunchKernelGGL(k_pair_reduce, ngrid, dim3(PT_THREADS), 0, st, pa, groups, C * C * 3, C, dwa, dba);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}

int check_geom(int batch, int channels, int h, int w, int dil, const char *who) {
    LAV_REQUIRE(lav_pair_train_supported(channels, w), "%s: (channels %d, width %d) is not one of (16, 128), (64, 64), (128, 32)", who, channels, w);
    LAV_REQUIRE(batch >= 1 && h >= 1 && dil >= 1, "%s: batch %d, rows %d, dilation %d", who, batch, h, dil);
    LAV_REQUIRE((long)batch * h <= (1L << 30) && (long)batch * channels * h * w < (1L << 31), "%s: tensor too large", who);
    return LAV_OK;
}

}  // namespace

extern "C" int lav_pair_train_supported(int channels, int width) {
    return (channels == 16 && width == 128) || (channels == 64 && width == 64) || (channels == 128 && width == 32);
}

extern "C" size_t lav_pair_train_workspace_bytes(int batch, int channels, int h) {
    if (batch < 1 || channels < 1 || h < 1) return 0;
    return 2 * (size_t)wgrad_groups(batch * h) * ((size_t)channels * channels * 3 + channels) * sizeof(float);
}

extern "C" int lav_pair_train_forward(const float *x, const float *wa, const float *ba, const float *wb, const float *bb, int batch, int channels,
                                      int h, int w, int dil, float *t, float *z, void *stream) {
    LAV_REQUIRE(x && wa && ba && wb && bb && t && z, "lav_pair_train_forward: null pointer");
    if (int rc = check_geom(batch, channels, h, w, dil, "lav_pair_train_forward")) return rc;
    const PairGeom g{batch, h, dil};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("pair_train_fwd", st);
    int rc = channels == 16 ? launch_fwd<16, 128>(g, x, wa, ba, wb, bb, t, z, st)
             : channels == 64 ? launch_fwd<64, 64>(g, x, wa, ba, wb, bb, t, z, st)
                              : launch_fwd<128, 32>(g, x, wa, ba, wb, bb, t, z, st);
    timer_end(tok, st);
    return rc;
}

extern "C" int lav_pair_train_backward(const float *x, const float *t, const float *dz, const float *wa, const float *wb, int batch, int channels,
                                       int h, int w, int dil, float *dt, float *dx, float *dwa, float *dba, float *dwb, float *dbb, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    LAV_REQUIRE(x && t && dz && wa && wb && dt && dx && dwa && dba && dwb && dbb && workspace, "lav_pair_train_backward: null pointer");
    if (int rc = check_geom(batch, channels, h, w, dil, "lav_pair_train_backward")) return rc;
    LAV_REQUIRE(workspace_bytes >= lav_pair_train_workspace_bytes(batch, channels, h), "lav_pair_train_backward: workspace smaller than lav_pair_train_workspace_bytes");
    const PairGeom g{batch, h, dil};
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *p = static_cast<float *>(workspace);
    const int tok = timer_begin("pair_train_bwd", st);
    int rc = channels == 16 ? launch_bwd<16, 128>(g, x, t, dz, wa, wb, dt, dx, dwa, dba, dwb, dbb, p, st)
             : channels == 64 ? launch_bwd<64, 64>(g, x, t, dz, wa, wb, dt, dx, dwa, dba, dwb, dbb, p, st)
                              : launch_bwd<128, 32>(g, x, t, dz, wa, wb, dt, dx, dwa, dba, dwb, dbb, p, st);
    timer_end(tok, st);
    return rc;
}

extern "C" size_t lav_seg_xent_workspace_bytes(void) { return XENT_GROUPS * sizeof(double); }

extern "C" int lav_seg_xent_forward(const float *logits, const long long *labels, int batch, int classes, long plane, float *loss, float *dlogits,
                                    void *workspace, size_t workspace_bytes, void *stream) {
    LAV_REQUIRE(logits && labels && loss && dlogits && workspace, "lav_seg_xent_forward: null pointer");
    LAV_REQUIRE(classes >= 1 && classes <= XENT_MAX_C, "lav_seg_xent_forward: %d classes (1..%d)", classes, XENT_MAX_C);
    LAV_REQUIRE(batch >= 1 && plane >= 1 && (long)batch * plane * classes < (1L << 40), "lav_seg_xent_forward: batch %d, plane %ld", batch, plane);
    LAV_REQUIRE(workspace_bytes >= lav_seg_xent_workspace_bytes(), "lav_seg_xent_forward: workspace smaller than lav_seg_xent_workspace_bytes");
    const long n = (long)batch * plane;
    const int groups = (int)std::min<long>((n + PT_THREADS - 1) / PT_THREADS, XENT_GROUPS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    const int tok = timer_begin("seg_xent", st);
    hipLaunchKernelGGL(k_xent, dim3((unsigned)groups), dim3(PT_THREADS), 0, st, logits, labels, batch, classes, plane, (float)(1.0 / (double)n),
                       dlogits, partial);
    hipLaunchKernelGGL(k_xent_final, dim3(1), dim3(PT_THREADS), 0, st, partial, groups, 1.0 / (double)n, loss);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}

extern "C" int lav_seg_xent_up_forward(const float *logits, const void *labels, int label_bytes, int batch, int classes, int h, int w, int scale,
                                       float *loss, float *dlogits, void *workspace, size_t workspace_bytes, void *stream) {
    LAV_REQUIRE(logits && labels && loss && dlogits && workspace, "lav_seg_xent_up_forward: null pointer");
    LAV_REQUIRE(label_bytes == 1 || label_bytes == 8, "lav_seg_xent_up_forward: labels of %d bytes (1: uint8, 8: int64)", label_bytes);
    LAV_REQUIRE(classes >= 1 && classes <= XENT_MAX_C, "lav_seg_xent_up_forward: %d classes (1..%d)", classes, XENT_MAX_C);
    LAV_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && scale >= 1 && scale <= 64, "lav_seg_xent_up_forward: batch %d, %d x %d, scale %d", batch, h, w, scale);
    LAV_REQUIRE((long)batch * h * w * scale * scale * std::max(classes, 8) < (1L << 40), "lav_seg_xent_up_forward: too large");
    LAV_REQUIRE(workspace_bytes >= lav_seg_xent_workspace_bytes(), "lav_seg_xent_up_forward: workspace smaller than lav_seg_xent_workspace_bytes");
    const long n = (long)batch * h * w;
    const double inv_n = 1.0 / ((double)n * scale * scale);
    const int groups = (int)std::min<long>((n + PT_THREADS - 1) / PT_THREADS, XENT_GROUPS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    const int tok = timer_begin("seg_xent_up", st);
    if (label_bytes == 1)
        hipLaunchKernelGGL(k_xent_up<unsigned char>, dim3((unsigned)groups), dim3(PT_THREADS), 0, st, logits,
                           static_cast<const unsigned char *>(labels), batch, classes, h, w, scale, (float)inv_n, dlogits, partial);
    else
        hipLaunchKernelGGL(k_xent_up<long long>, dim3((unsigned)groups), dim3(PT_THREADS), 0, st, logits,
                           static_cast<const long long *>(labels), batch, classes, h, w, scale, (float)inv_n, dlogits, partial);
    hipLaunchKernelGGL(k_xent_final, dim3(1), dim3(PT_THREADS), 0, st, partial, groups, inv_n, loss);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
