// A run of L <= 3 identical 3x3 layers (stride 1, pad 1, no bias) -> ReLU -> BatchNorm affine at C = 64 channels over one H x W map,
// batch 1, as ONE launch WITHOUT any hand-off between workgroups (lav_conv3x3_tile_f16): stage s1 of the BEV backbone behind its
// stride-2 layer (lav_amd/lidar.py ConvBackbone).  Arithmetic per output value as k_conv_split_f16 and k_conv3x3_run_f16: two fp16
// pieces per operand, three v_mfma_f32_32x32x16_f16 products (split_arith.hpp's F16X3 order), fp32 accumulate, f16_out_scales, the
// layers' own packed fp16 weights; the K loop's sums are grouped as k_conv3x3_run_f16's (one chain per 16-channel chunk).
//
// Workgroup (512 threads) = one TH x TW output tile for all L layers.  It stages the input tile with a halo of L pixels once and
// recomputes the halo of the intermediate layers: layer l (0-based) computes the tile grown by e = L - 1 - l pixels on every side.
//   buffers    two LDS maps [piece][8 channels][pixel of the region] x 16 B.  A holds the input region, B layer 0's output, A again
//              layer 1's.  A position outside the MAP holds 0 in every buffer: the zero padding of the next layer applies to the map,
//              not to the tile (what the convolution would give there is not zero: ReLU and BatchNorm leave `shift`).
//   waves      eight = 2 cout blocks of 32 x 4 groups.  Any 32 pixels of a region form a matrix block (a lane addresses its own pixel
//              in LDS); group g multiplies blocks g and g + 4: at most two accumulators per wave, every wave runs the whole K loop.
//   weights    straight from L2 into a nine-tap register ring per wave, as conv_run.hip: a tap's slot is refilled as soon as it is used,
//              with the next chunk's tap or the next layer's first chunk.
//   scales     layer 0: the power of two of the producer's amax parts.  Later layers: of the largest finite |value| of the region the
//              workgroup just computed (positions inside the map only), one LDS reduction at the barrier between two layers.
//   output     the last layer stores its tile (plain stores, a lane's neighbours write consecutive x) and leaves one maximum per
//              workgroup in amax_out - the layout lav_conv2d_amax's readers take.
// No loop waits on another workgroup and there is no workspace.  Maps that are no multiple of the tile: loads are clamped, stores
// masked; the LDS addresses depend on the tile alone.
#include <cstdlib>
#include <cstring>

#include "common.hpp"
#include "persistent.hpp"
#include "split_arith.hpp"

namespace {
using namespace lav;

constexpr int TILE_C = 64, TILE_MAX_L = 3, TILE_MAX_WG = 16384;
constexpr size_t TILE_W_BYTES = (size_t)9 * (TILE_C / 32) * (TILE_C / 16) * 2 * 1024;   // fp16 section of a layer: [cout block][tap][chunk][piece][lane] x 16 B

struct TileArgs {
    const float *x;
    float *out;
    const unsigned char *w[TILE_MAX_L];
    const float *wscale[TILE_MAX_L], *scale[TILE_MAX_L], *shift[TILE_MAX_L];
    const float *amax_in;
    float *amax_out;
    int amax_in_count, H, W, tiles_x;
};

__device__ __forceinline__ void tile_load_w(const unsigned char *p, int t, u32x4 (&dst)[2]) {
    // p: the lane's 16 bytes of tap 0 of a chunk; a tap further on is 4 chunks x 2 KB away
    dst[0] = *reinterpret_cast<const u32x4 *>(p + t * (TILE_C / 16) * 2048);
    dst[1] = *reinterpret_cast<const u32x4 *>(p + t * (TILE_C / 16) * 2048 + 1024);
}

// chunk x tap loop of one layer over NA pixel blocks of the wave.  in: the layer's input region (RWI pixels wide, NPI pixels),
// base[j]: byte offset of the lane's pixel of block j (its tap (0, 0)) inside a channel group.
template <int NA, int RWI, int NPI>
__device__ __forceinline__ void tile_mma(const unsigned char *in, const int (&base)[2], int half, u32x4 (&wr)[9][2], const unsigned char *w_this,
                                         const unsigned char *w_next, f32x16 (&tot)[2]) {
    constexpr int PIECE = 8 * NPI * 16;
#pragma nounroll
    for (int ch = 0; ch < TILE_C / 16; ++ch) {
        // one accumulation chain per chunk (27 products), the chunks' sums added in order - the chain length of conv_run.hip's K parts: a
        // single chain of 108 products is 1.7x as far from float64 (the matrix pipe truncates every accumulation)
        f32x16 acc[NA];
#pragma unroll
        for (int j = 0; j < NA; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        const unsigned char *w_refill = ch + 1 < TILE_C / 16 ? w_this + (ch + 1) * 2048 : w_next;
        const unsigned char *bin = in + (ch * 2 + half) * NPI * 16;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int toff = ((t / 3) * RWI + (t % 3)) * 16;
            u32x4 b[NA][2];
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                b[j][0] = *reinterpret_cast<const u32x4 *>(bin + toff + base[j]);
                b[j][1] = *reinterpret_cast<const u32x4 *>(bin + PIECE + toff + base[j]);
            }
            // split_arith.hpp's F16X3_A / _B order, smallest terms first: w1 b0, w0 b1, w0 b0; consecutive products go round the accumulators
#pragma unroll
            for (int j = 0; j < NA; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wr[t][1]), __builtin_bit_cast(f16x8, b[j][0]), acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NA; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wr[t][0]), __builtin_bit_cast(f16x8, b[j][1]), acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NA; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wr[t][0]), __builtin_bit_cast(f16x8, b[j][0]), acc[j], 0, 0, 0);
            tile_load_w(w_refill, t, wr[t]);
        }
#pragma unroll
        for (int j = 0; j < NA; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[j][r] += acc[j][r];
    }
}

// One layer: the OH x OW region whose first pixel is (oy0, ox0) of the map, from `in` (the region grown by one pixel) into `outb`
// (pieces of the next layer's input, scaled by what the region holds) or, LAST, into the map a.out.  Returns the next layer's
// activation scale.  s_epi: this layer's [scale 64][shift 64].
template <int OH, int OW, bool LAST>
__device__ __forceinline__ float tile_layer(const TileArgs &a, const unsigned char *in, unsigned char *outb, int oy0, int ox0, float sx, float sw,
                                            const float *s_epi, float *s_wmax, u32x4 (&wr)[9][2], const unsigned char *w_this,
                                            const unsigned char *w_next) {
    constexpr int NP = OH * OW, NB = (NP + 31) / 32, RWI = OW + 2, NPI = (OH + 2) * (OW + 2);
    static_assert(NB <= 8, "two pixel blocks per wave group at the most");
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cbw = wid & 1, grp = wid >> 1;
    const int H = a.H, W = a.W;
    const long plane = (long)H * W;

    int qu[2], base[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        qu[j] = (grp + 4 * j) * 32 + l31;                    // the lane's pixel of block j; past the region: multiplies a copy of the last pixel, never stored
        const int q = min(qu[j], NP - 1);
        base[j] = ((q / OW) * RWI + (q % OW)) * 16;
    }
    const int nact = grp + 4 < NB ? 2 : grp < NB ? 1 : 0;     // (wave-uniform)
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    if (nact == 2) tile_mma<2, RWI, NPI>(in, base, half, wr, w_this, w_next, acc);
    else tile_mma<1, RWI, NPI>(in, base, half, wr, w_this, w_next, acc);   // (a wave without a block multiplies block 0's copy: the ring moves on all the same)

    float out_sx, out_sw;
    f16_out_scales(sx, sw, out_sx, out_sw);
    float lm = 0.f;
    bool inmap[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = min(qu[j], NP - 1);
        const int gy = oy0 + q / OW, gx = ox0 + q % OW;
        inmap[j] = j < nact && qu[j] < NP && gy >= 0 && gy < H && gx >= 0 && gx < W;
        float *yo = a.out + (long)gy * W + gx;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = cbw * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            float vv = acc[j][r] * out_sx * out_sw;
            vv = relu_nan(vv);
            vv = fmaf(vv, s_epi[co], s_epi[64 + co]);
            vv = inmap[j] ? vv : 0.f;
            if (LAST) {
                if (inmap[j]) yo[co * plane] = vv;
            } else {
                acc[j][r] = vv;
            }
            lm = fmaxf(lm, finite_abs(vv));
        }
    }
    lm = wave_finite_absmax(lm);
    if (lane == 0) s_wmax[wid] = lm;
    __syncthreads();   // everybody is through with `in`, and the waves' maxima are there
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) m = fmaxf(m, s_wmax[i]);
    if (LAST) {
        if (tid == 0 && a.amax_out) a.amax_out[blockIdx.x] = m;
        return 0.f;
    }
    const float sn = f16_scale_of(m), inv = 1.f / sn;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j < nact && qu[j] < NP) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {   // the lane's four channels (r & 3) + 4 * half of channel group cbw * 4 + g
                unsigned p00, p01, p10, p11;
                split2h_pair(acc[j][4 * g] * inv, acc[j][4 * g + 1] * inv, p00, p10);
                split2h_pair(acc[j][4 * g + 2] * inv, acc[j][4 * g + 3] * inv, p01, p11);
                unsigned char *d = outb + ((cbw * 4 + g) * NP + qu[j]) * 16 + half * 8;
                *reinterpret_cast<u32x2 *>(d) = u32x2{p00, p01};
                lds_store_fence();
                *reinterpret_cast<u32x2 *>(d + 8 * NP * 16) = u32x2{p10, p11};
                lds_store_fence();
            }
        }
    }
    __syncthreads();   // the next layer's input is complete (and s_wmax may be written again)
    return sn;
}

template <int TH, int TW, int L>
__global__ __launch_bounds__(512) void k_conv3x3_tile_f16(TileArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int RH = TH + 2 * L, RW = TW + 2 * L, NPA = RH * RW;
    constexpr int NPB = L > 1 ? (TH + 2 * (L - 1)) * (TW + 2 * (L - 1)) : 0;
    constexpr int BUF_A = 2 * 8 * NPA * 16, BUF_B = 2 * 8 * NPB * 16;
    unsigned char *bufA = smem, *bufB = smem + BUF_A;
    float *s_epi = reinterpret_cast<float *>(smem + BUF_A + BUF_B);   // [L][scale 64 | shift 64]
    float *s_wmax = s_epi + L * 128;                                  // [8]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = a.H, W = a.W;
    const long plane = (long)H * W;
    const int ty0 = (blockIdx.x / a.tiles_x) * TH, tx0 = (blockIdx.x % a.tiles_x) * TW;

    u32x4 wr[9][2];
    const long wlane = (long)(wid & 1) * 9 * (TILE_C / 16) * 2048 + lane * 16;   // the wave's cout block, first chunk
#pragma unroll
    for (int t = 0; t < 9; ++t) tile_load_w(a.w[0] + wlane, t, wr[t]);
    if (tid < L * 128) {
        const int l = tid >> 7, c = tid & 63;
        s_epi[tid] = (tid & 64) ? a.shift[l][c] : a.scale[l][c];
    }
    const float m_in = parts_absmax(a.amax_in, a.amax_in_count, lane);   // the producer's maxima (every wave for itself)
    float sx = f16_scale_of(m_in);

    // ---- the input region: 8 channels of one pixel per task; all loads in flight, then conversion
    {
        constexpr int NTASK = NPA * 8, NTK = (NTASK + 511) / 512;
        const float inv = 1.f / sx;
        float v[NTK][8];
        bool ok[NTK];
#pragma unroll
        for (int u = 0; u < NTK; ++u) {
            const int task = min(tid + u * 512, NTASK - 1);
            const int g = task / NPA, p = task - g * NPA;
            const int gy = ty0 - L + p / RW, gx = tx0 - L + p % RW;
            ok[u] = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const float *sp = a.x + (long)g * 8 * plane + (long)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
#pragma unroll
            for (int c = 0; c < 8; ++c) v[u][c] = sp[c * plane];
        }
#pragma unroll
        for (int u = 0; u < NTK; ++u) {
            const int task = tid + u * 512;
            if (task < NTASK) {
                u32x4 q0, q1;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    unsigned p0, p1;
                    split2h_pair(ok[u] ? v[u][2 * e] * inv : 0.f, ok[u] ? v[u][2 * e + 1] * inv : 0.f, p0, p1);
                    q0[e] = p0; q1[e] = p1;
                }
                *reinterpret_cast<u32x4 *>(bufA + task * 16) = q0;            // task = group * NPA + pixel
                *reinterpret_cast<u32x4 *>(bufA + BUF_A / 2 + task * 16) = q1;
            }
        }
    }
    __syncthreads();

    if constexpr (L == 1) {
        tile_layer<TH, TW, true>(a, bufA, nullptr, ty0, tx0, sx, *a.wscale[0], s_epi, s_wmax, wr, a.w[0] + wlane, a.w[0] + wlane);
    } else if constexpr (L == 2) {
        sx = tile_layer<TH + 2, TW + 2, false>(a, bufA, bufB, ty0 - 1, tx0 - 1, sx, *a.wscale[0], s_epi, s_wmax, wr, a.w[0] + wlane, a.w[1] + wlane);
        tile_layer<TH, TW, true>(a, bufB, nullptr, ty0, tx0, sx, *a.wscale[1], s_epi + 128, s_wmax, wr, a.w[1] + wlane, a.w[1] + wlane);
    } else {
        sx = tile_layer<TH + 4, TW + 4, false>(a, bufA, bufB, ty0 - 2, tx0 - 2, sx, *a.wscale[0], s_epi, s_wmax, wr, a.w[0] + wlane, a.w[1] + wlane);
        sx = tile_layer<TH + 2, TW + 2, false>(a, bufB, bufA, ty0 - 1, tx0 - 1, sx, *a.wscale[1], s_epi + 128, s_wmax, wr, a.w[1] + wlane, a.w[2] + wlane);
        tile_layer<TH, TW, true>(a, bufA, nullptr, ty0, tx0, sx, *a.wscale[2], s_epi + 256, s_wmax, wr, a.w[2] + wlane, a.w[2] + wlane);
    }
}

struct TileConfig { int th, tw, tiles_x, tiles; size_t lds; };

// how a run of this geometry is cut, or false: not served (the caller keeps one launch per layer)
bool tile_config(int channels, int h, int w, int nlayers, TileConfig &c) {
    if (channels != TILE_C || nlayers < 1 || nlayers > TILE_MAX_L || h < 1 || w < 1 || h > 32768 || w > 32768) return false;
    c.th = 8; c.tw = 16;
    c.tiles_x = (w + c.tw - 1) / c.tw;
    const long tiles = (long)c.tiles_x * ((h + c.th - 1) / c.th);
    if (tiles > TILE_MAX_WG) return false;
    c.tiles = (int)tiles;
    const int L = nlayers;
    const size_t npa = (size_t)(c.th + 2 * L) * (c.tw + 2 * L), npb = L > 1 ? (size_t)(c.th + 2 * (L - 1)) * (c.tw + 2 * (L - 1)) : 0;
    c.lds = (npa + npb) * 2 * 8 * 16 + (size_t)L * 128 * 4 + 8 * 4;
    return c.lds <= 160 * 1024;
}

template <int TH, int TW, int L>
int tile_launch(const TileArgs &a, const TileConfig &c, hipStream_t st) {
    return launch_lds<k_conv3x3_tile_f16<TH, TW, L>>(dim3(c.tiles), dim3(512), c.lds, st, 160 * 1024, a);
}
}  // namespace

extern "C" size_t lav_conv3x3_tile_f16_lds_bytes(int channels, int h, int w, int nlayers) {
    TileConfig c;
    return tile_config(channels, h, w, nlayers, c) ? c.lds : 0;
}

extern "C" int lav_conv3x3_tile_f16_amax_count(int channels, int h, int w, int nlayers) {
    TileConfig c;
    return tile_config(channels, h, w, nlayers, c) ? c.tiles : 0;
}

extern "C" int lav_conv3x3_tile_f16(int channels, int h, int w, int nlayers, const float *x, const void *const *w_f16, const float *const *scale,
                                    const float *const *shift, float *out, const float *amax_in, int amax_in_count, float *amax_out, void *stream) {
    TileConfig c;
    LAV_REQUIRE(tile_config(channels, h, w, nlayers, c), "lav_conv3x3_tile_f16: %d layers of %d channels on %d x %d are not served (lav_conv3x3_tile_f16_lds_bytes returns 0)",
                nlayers, channels, h, w);
    LAV_REQUIRE(x && w_f16 && scale && shift && out && amax_in && amax_in_count >= 1, "lav_conv3x3_tile_f16: null argument (the first layer's scale comes from amax_in)");
    TileArgs a;
    for (int i = 0; i < TILE_MAX_L; ++i) {
        const int j = layer_of(i, nlayers);
        LAV_REQUIRE(w_f16[j] && scale[j] && shift[j], "lav_conv3x3_tile_f16: null argument of layer %d", j);
        a.w[i] = static_cast<const unsigned char *>(w_f16[j]);
        a.wscale[i] = reinterpret_cast<const float *>(a.w[i] + TILE_W_BYTES);   // (the packing's tail: conv_split.hpp)
        a.scale[i] = scale[j]; a.shift[i] = shift[j];
    }
    a.x = x; a.out = out; a.amax_in = amax_in; a.amax_in_count = amax_in_count; a.amax_out = amax_out;
    a.H = h; a.W = w; a.tiles_x = c.tiles_x;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("conv3x3_tile", st);
    const int rc = nlayers == 1 ? tile_launch<8, 16, 1>(a, c, st) : nlayers == 2 ? tile_launch<8, 16, 2>(a, c, st) : tile_launch<8, 16, 3>(a, c, st);
    timer_end(tok, st);   // (also when the launch failed: the slot that timer_begin opened is closed on every path)
    return rc;
}
