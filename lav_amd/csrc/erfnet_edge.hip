// ERFNet's two entry DownsamplerBlocks (3 -> 16 -> 64 channels, H x W -> H/4 x W/4) as ONE launch (lav_erfnet_entry).
//
// A DownsamplerBlock is relu(bn(cat(conv3x3/s2(x), maxpool2x2(x)))).  As separate launches the two blocks at the network's entry are
// four dependent kernels (k_conv_smallcin, k_pool_affine, k_conv_split, k_pool_affine: 31.5 us of the frame's lidar graph) for
// 0.6 GFLOP and 10 MB: launch latency, not work.  Both branches of a block read the same input tile and block 2 needs a one-pixel
// halo of block 1's output, so one workgroup can own an 8 x 8 tile of block 2's output from the raw image to the store:
//   LDS         the 35 x 35 x 3 input patch of the tile (out-of-image positions hold pad_value, the pre-image of the reference's zero
//               padding under the folded input affine), both blocks' weights and epilogue vectors, and block 1's 16 channels on the
//               17 x 17 region block 2 reads (positions outside block 1's image are block 2's zero padding);
//   block 1     wave g computes channels 4g .. 4g+3 of the region, a position per lane: 27 fp32 FMAs per convolution channel in
//               ascending (ci, ky, kx) order as k_conv_smallcin does them; the three pooled channels (max, fmaf, ReLU as k_pool_affine)
//               ride in wave 3 beside convolution channel 12.  Pool windows are 2 x 2 at stride 2 on even sizes: none crosses the edge;
//   block 2     wave g owns two rows of the tile (16 pixels) x 48 convolution channels: K = 144 as 36 steps of three
//               v_mfma_f32_16x16x4_f32 (exact fp32 products, an fp32 FMA chain per output: right in every precision mode).  The weights
//               are the A operand, so the pixels sit on the lanes and a store instruction writes whole 32-byte row segments.
//               The 16 pooled channels are four outputs per thread.
// No workgroup reads another's data: no flags, no counters, an ordinary grid of ceil(W/32) x ceil(H/32) x batch workgroups.
#include <cstdint>

#include "common.hpp"

namespace {
using namespace lav;
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int EN_T = 8;                       // output tile of block 2: EN_T x EN_T pixels
constexpr int EN_RN = 2 * EN_T + 1;           // block 1 region of the tile: 17 x 17
constexpr int EN_PN = 4 * EN_T + 3;           // input patch: 35 x 35
constexpr int EN_IS = 37;                     // input patch row stride (odd: the stride-2 reads of a wave spread over the banks)
constexpr int EN_RS = 24;                     // region row stride: two region rows (a pixel row of block 2) are 16 banks apart
constexpr int EN_CS = EN_RN * EN_RS + 1;      // region channel stride (odd: the two k of a half wave sit on odd / even banks)
constexpr int EN_WS = 49;                     // block 2 weight row stride [k][48 + 1]
constexpr int EN_C1 = 16, EN_C1C = 13, EN_C2 = 64, EN_C2C = 48, EN_K1 = 27, EN_K2 = 144;
constexpr int EN_IN = (3 * EN_PN * EN_IS + 3) / 4 * 4, EN_B1 = EN_C1 * EN_CS, EN_W2 = EN_K2 * EN_WS, EN_W1 = EN_K1 * EN_C1;
constexpr int EN_EP = 3 * EN_C1 + EN_C2C + 2 * EN_C2;
constexpr size_t EN_LDS = (size_t)(EN_IN + EN_B1 + EN_W2 + EN_W1 + EN_EP) * sizeof(float);

struct EntryArgs {
    const float *__restrict__ x, *__restrict__ w1, *__restrict__ b1, *__restrict__ s1, *__restrict__ t1;
    const float *__restrict__ w2, *__restrict__ b2, *__restrict__ s2, *__restrict__ t2;
    float *__restrict__ y;
    int H, W;
    float pad;
};

__global__ __launch_bounds__(256) void k_erfnet_entry(EntryArgs a) {
    extern __shared__ __attribute__((aligned(16))) float en_smem[];
    float *s_in = en_smem;                 // [3][EN_PN][EN_IS]
    float *s_b1 = s_in + EN_IN;            // [16][EN_CS] as rows of EN_RS
    float *s_w2 = s_b1 + EN_B1;            // [tap * 16 + ci][EN_WS]
    float *s_w1 = s_w2 + EN_W2;            // [ci * 9 + tap][16] (channels 13..15: zeros)
    float *s_ep = s_w1 + EN_W1;            // bias1[16], scale1[16], shift1[16], bias2[48], scale2[64], shift2[64]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.z, oy0 = blockIdx.y * EN_T, ox0 = blockIdx.x * EN_T;
    const int H = a.H, W = a.W, H1 = H >> 1, W1 = W >> 1, OH = H >> 2, OW = W >> 2;

    // ---- staging: every load of a thread is issued before the first is stored
    {
        const int iy0 = 4 * oy0 - 3, ix0 = 4 * ox0 - 3;
        const float *xn = a.x + (long)n * 3 * H * W;
        constexpr int NPT = 3 * EN_PN * EN_PN, NIT = (NPT + 255) / 256;
        float v[NIT];
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int e = min(tid + 256 * i, NPT - 1);
            const int px = e % EN_PN, r = e / EN_PN, py = r % EN_PN, ci = r / EN_PN;
            const int iy = iy0 + py, ix = ix0 + px;
            const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
            const float t = xn[((long)ci * H + min(max(iy, 0), H - 1)) * W + min(max(ix, 0), W - 1)];
            v[i] = ok ? t : a.pad;
        }
        // block 2's weights [48][16][9] -> [tap * 16 + ci][co]: read as 16-byte pieces in source order
        constexpr int NW4 = EN_C2C * EN_K2 / 4, NWI = (NW4 + 255) / 256;
        float4 wv[NWI];
#pragma unroll
        for (int i = 0; i < NWI; ++i) wv[i] = reinterpret_cast<const float4 *>(a.w2)[min(tid + 256 * i, NW4 - 1)];
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int e = tid + 256 * i;
            if (e < NPT) s_in[(e / EN_PN) * EN_IS + e % EN_PN] = v[i];
        }
#pragma unroll
        for (int i = 0; i < NWI; ++i) {
            const int q = tid + 256 * i;
            if (q < NW4) {
                const float w4[4] = {wv[i].x, wv[i].y, wv[i].z, wv[i].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = 4 * q + j, tap = e % 9, r = e / 9, ci = r % 16, co = r / 16;
                    s_w2[(tap * 16 + ci) * EN_WS + co] = w4[j];
                }
            }
        }
        for (int d = tid; d < EN_W1; d += 256) {
            const int co = d % EN_C1, k = d / EN_C1;
            s_w1[d] = co < EN_C1C ? a.w1[co * EN_K1 + k] : 0.f;
        }
        if (tid < EN_C1) {
            s_ep[tid] = tid < EN_C1C ? a.b1[tid] : 0.f;
            s_ep[EN_C1 + tid] = a.s1[tid];
            s_ep[2 * EN_C1 + tid] = a.t1[tid];
        }
        if (tid < EN_C2C) s_ep[3 * EN_C1 + tid] = a.b2[tid];
        if (tid < EN_C2) {
            s_ep[3 * EN_C1 + EN_C2C + tid] = a.s2[tid];
            s_ep[3 * EN_C1 + EN_C2C + EN_C2 + tid] = a.t2[tid];
        }
    }
    __syncthreads();

    // ---- block 1 on the 17 x 17 region: wave g -> channels 4g .. 4g+3
    {
        const int c0 = 4 * wave;
        const float4 b4 = *reinterpret_cast<const float4 *>(s_ep + c0), sc4 = *reinterpret_cast<const float4 *>(s_ep + EN_C1 + c0),
                     sh4 = *reinterpret_cast<const float4 *>(s_ep + 2 * EN_C1 + c0);
        const float bb[4] = {b4.x, b4.y, b4.z, b4.w}, ss[4] = {sc4.x, sc4.y, sc4.z, sc4.w}, hh[4] = {sh4.x, sh4.y, sh4.z, sh4.w};
        for (int p = lane; p < EN_RN * EN_RN; p += 64) {
            const int ry = p / EN_RN, rx = p - ry * EN_RN;
            const int y1 = 2 * oy0 - 1 + ry, x1 = 2 * ox0 - 1 + rx;
            const bool inside = y1 >= 0 && y1 < H1 && x1 >= 0 && x1 < W1;
            const float *in0 = s_in + (2 * ry) * EN_IS + 2 * rx;     // tap (0, 0) of the position, channel 0
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ci = 0; ci < 3; ++ci)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const float xv = in0[(ci * EN_PN + ky) * EN_IS + kx];
                        const float4 w4 = *reinterpret_cast<const float4 *>(s_w1 + (ci * 9 + ky * 3 + kx) * EN_C1 + c0);   // broadcast
                        acc[0] = fmaf(xv, w4.x, acc[0]);
                        acc[1] = fmaf(xv, w4.y, acc[1]);
                        acc[2] = fmaf(xv, w4.z, acc[2]);
                        acc[3] = fmaf(xv, w4.w, acc[3]);
                    }
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = acc[j] + bb[j];
            if (wave == 3) {   // channels 13..15: the pooled branch of input channels 0..2 (the window: input rows 2 y1, 2 y1 + 1)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float *q = in0 + (c * EN_PN + 1) * EN_IS + 1;
                    v[c + 1] = max_nan4(q[0], q[1], q[EN_IS], q[EN_IS + 1]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t = fmaf(v[j], ss[j], hh[j]);
                t = relu_nan(t);
                s_b1[(c0 + j) * EN_CS + ry * EN_RS + rx] = inside ? t : 0.f;
            }
        }
    }
    __syncthreads();

    // ---- block 2, convolution branch: wave g -> tile rows 2g, 2g+1; D[channel][pixel] = sum_k W[channel][k] * X[k][pixel]
    const long plane = (long)OH * OW;
    float *yn = a.y + (long)n * EN_C2 * plane;
    {
        const int pr = lane & 15, kq = lane >> 4;
        const int py = 2 * wave + (pr >> 3), px = pr & 7;
        const float *xb = s_b1 + kq * EN_CS + (2 * py) * EN_RS + 2 * px;     // B[k = kq][pixel pr] of step (tap 0, chunk 0)
        const float *wb = s_w2 + kq * EN_WS + pr;                            // A[channel pr][k = kq]
        f32x4 acc[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                const float xv = xb[4 * kc * EN_CS + (tap / 3) * EN_RS + tap % 3];
                const float *wr = wb + (tap * 16 + 4 * kc) * EN_WS;
#pragma unroll
                for (int nt = 0; nt < 3; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[16 * nt], xv, acc[nt], 0, 0, 0);
            }
        const int oy = oy0 + py, ox = ox0 + px;
        if (oy < OH && ox < OW) {
            const float *e_b = s_ep + 3 * EN_C1, *e_s = e_b + EN_C2C, *e_t = e_s + EN_C2;
#pragma unroll
            for (int nt = 0; nt < 3; ++nt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int co = 16 * nt + 4 * kq + j;      // D row = 4 (lane >> 4) + register
                    float v = acc[nt][j] + e_b[co];
                    v = fmaf(v, e_s[co], e_t[co]);
                    yn[co * plane + (long)oy * OW + ox] = relu_nan(v);
                }
        }
    }
    // ---- block 2, pooled branch: 16 channels x 64 pixels
    {
        const float *e_s = s_ep + 3 * EN_C1 + EN_C2C + EN_C2C, *e_t = e_s + EN_C2;   // channels 48..63
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int it = tid + 256 * i, px = it & 7, py = (it >> 3) & 7, c = it >> 6;
            const float *q = s_b1 + c * EN_CS + (2 * py + 1) * EN_RS + 2 * px + 1;
            float v = max_nan4(q[0], q[1], q[EN_RS], q[EN_RS + 1]);
            v = fmaf(v, e_s[c], e_t[c]);
            const int oy = oy0 + py, ox = ox0 + px;
            if (oy < OH && ox < OW) yn[(EN_C2C + c) * plane + (long)oy * OW + ox] = relu_nan(v);
        }
    }
}
}  // namespace

extern "C" int lav_erfnet_entry(const float *x, int batch, int h, int w, const float *w1, const float *b1, float pad_value, const float *scale1,
                                const float *shift1, const float *w2, const float *b2, const float *scale2, const float *shift2, float *y,
                                void *stream) {
    LAV_REQUIRE(batch >= 1 && batch <= 65535 && h >= 4 && w >= 4 && h % 4 == 0 && w % 4 == 0, "lav_erfnet_entry: h, w multiples of 4 and 1 <= batch <= 65535 expected");
    LAV_REQUIRE((long)batch * 64 * (h / 4) * (w / 4) < (1L << 31) && (long)batch * 3 * h * w < (1L << 31), "lav_erfnet_entry: tensor too large");
    LAV_REQUIRE(x && w1 && b1 && scale1 && shift1 && w2 && b2 && scale2 && shift2 && y, "lav_erfnet_entry: bad argument");
    LAV_REQUIRE(reinterpret_cast<uintptr_t>(w2) % 16 == 0, "lav_erfnet_entry: w2 must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    EntryArgs a{x, w1, b1, scale1, shift1, w2, b2, scale2, shift2, y, h, w, pad_value};
    const dim3 grid((unsigned)((w / 4 + EN_T - 1) / EN_T), (unsigned)((h / 4 + EN_T - 1) / EN_T), (unsigned)batch);
    LAV_REQUIRE(grid.y <= 65535, "lav_erfnet_entry: image too tall");
    const int tok = timer_begin("erfnet_entry", st);
    const int rc = launch_lds<k_erfnet_entry>(grid, dim3(256), EN_LDS, st, (int)EN_LDS, a);
    timer_end(tok, st);
    return rc;
}
