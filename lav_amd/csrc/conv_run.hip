// A run of L identical 3x3 layers (stride 1, pad 1, no bias) -> ReLU -> BatchNorm affine at C = 64 / 128 channels over one H x W
// map, batch 1, as ONE persistent launch (lav_conv3x3_run_f16): the BEV backbone's stages after their stride-2 layer
// (lav_amd/lidar.py ConvBackbone).  Arithmetic per output value as k_conv_split_f16 (conv_split_kernel.hpp): two fp16 pieces per
// operand, three v_mfma_f32_32x32x16_f16 products (lo x lo dropped), fp32 accumulate, the split kernel's own packed fp16 weights.
//
// Workgroup (512 threads) = one output row y x one slice s of NCBW cout blocks of 32, for all L layers.  Its eight waves are
// NCBW cout blocks x KS parts of the K loop (16-channel chunks); every wave multiplies all NPB pixel blocks of the row.  Per layer:
//   weights    straight from L2 into a nine-tap register ring (one chunk of the wave's cout block).  A tap's slot is refilled as soon
//              as it is used - with the next chunk's tap, or with the NEXT LAYER's first chunk: those requests are in flight while the
//              rows are awaited.  The BatchNorm vectors go to LDS before the wait, too.
//   hand-off   wave 0 polls the 64-bit words {layers done | largest finite |y| written} of rows y-1, y, y+1 (all slices: a row's
//              channels come from every slice) - one lane per word, the protocol of k_conv1d_pair_chain_f16 (conv_pair.hip).  The
//              layer's activation scale is the power of two of the maxima it just read (per workgroup and layer; the first layer
//              takes the producer's amax parts).  Waits are bounded (LAV_CHAIN_SPIN_LIMIT): a workgroup that gives up raises the
//              sticky counter and the launch's abort word, writes NaN over its part of the result and leaves; the others follow.
//   rows       the three input rows, all channels, write-through loads -> two fp16 pieces -> LDS [piece][8 channels][row][W + 2]
//              x 16 B (a zero column either side: the taps need no bounds)
//   matrix     chunk x tap loop, B fragments from LDS; the K parts' partial tiles are summed through LDS in a fixed order (the
//              epilogue of pixel block b is done by K part b % KS: every wave stores something)
//   publish    rows go out write-through into one of two ping-pong maps (the last layer: plain stores into the result), every wave
//              drains its stores, barrier, one lane stores the row's word.  The last layer leaves the workgroup's maximum in amax_out
//              (one float per workgroup, the layout lav_conv2d_amax's readers take).
// Two maps suffice: a workgroup overwrites row y of layer l-1 only after rows y-1 .. y+1 of layer l are out, i.e. after everyone
// who reads that row has staged it.
#include <cstdlib>
#include <cstring>

#include "common.hpp"
#include "persistent.hpp"
#include "split_arith.hpp"

namespace {
using namespace lav;

constexpr int RUN_MAX = 8;            // layers per run
constexpr int RUN_MAX_WG = 256;       // workgroups per run: all resident at once, one per CU
constexpr size_t RUN_ZERO_CAP = 16 + (size_t)RUN_MAX * RUN_MAX_WG * 8;   // abort word (16 B) + the words; zeroed per launch as needed
constexpr size_t RUN_STICKY_OFF = RUN_ZERO_CAP;                           // {time-outs, launches}
constexpr size_t RUN_MAPS_OFF = (RUN_STICKY_OFF + 16 + 255) / 256 * 256;
constexpr int RUN_TAIL_LDS = 2 * 128 * 4 + 64;                            // BatchNorm vectors, per-wave maxima, scale, abort flag

struct RunArgs {
    const float *x;
    float *out, *map[2];
    const unsigned char *w[RUN_MAX];                    // fp16 section of each layer's packed weights: [cout block][tap][chunk][piece][lane] x 16 B
    const float *wscale[RUN_MAX], *scale[RUN_MAX], *shift[RUN_MAX];
    const float *amax_in;
    float *amax_out;
    unsigned long long *words;                          // [layer][row * NS + slice]
    int *abort_word, *sticky;
    long long spin_limit;
    int amax_in_count, C, H, W, L, NS, data_bytes;
};

template <int NPB, int NCBW, int KS, int NTK>
__global__ __launch_bounds__(512) void k_conv3x3_run_f16(RunArgs a) {
    static_assert(NCBW * KS == 8, "eight waves");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cbw = wid % NCBW, kp = wid / NCBW;
    const int C = a.C, H = a.H, W = a.W, L = a.L, NS = a.NS;
    const int y = blockIdx.x / NS, s = blockIdx.x - y * NS;
    const int nchunk = C >> 4, G8 = C >> 3, WP = W + 2, nper = nchunk / KS;
    const int cb = s * NCBW + cbw;                    // the wave's cout block
    const long plane = (long)H * W;
    const int piece = G8 * 3 * WP * 16;               // bytes of one fp16 piece of the staged rows
    float *s_red = reinterpret_cast<float *>(smem);   // (overlays the staged rows once the matrix loop is through)
    float *s_epi = reinterpret_cast<float *>(smem + a.data_bytes);   // [2][128]
    float *s_wmax = s_epi + 256;                      // [8]
    float *s_m = s_wmax + 8;
    int *s_abort = reinterpret_cast<int *>(s_m + 4);
    if (tid == 0) *s_abort = 0;
    if (blockIdx.x == 0 && tid == 0) atomicAdd(a.sticky + 1, 1);

    u32x4 wr[9][2];
    // p: the lane's 16 bytes of tap 0 of a chunk; a tap further on is nchunk * 2 KB away
    auto load_w = [&](const unsigned char *p, int t, u32x4 (&dst)[2]) {
        dst[0] = *reinterpret_cast<const u32x4 *>(p + (long)t * nchunk * 2048);
        dst[1] = *reinterpret_cast<const u32x4 *>(p + (long)t * nchunk * 2048 + 1024);
    };
    const long wlane = ((long)cb * 9 * nchunk + kp * nper) * 2048 + lane * 16;   // the wave's first chunk of a layer
#pragma unroll
    for (int t = 0; t < 9; ++t) load_w(a.w[0] + wlane, t, wr[t]);
    float m_in = parts_absmax(a.amax_in, a.amax_in_count, lane);   // first layer: the producer's maxima (every wave for itself)

    int pxb[NPB];   // this lane's pixel of each pixel block (clamped: a block's tail multiplies a copy of the last pixel, never stored)
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) pxb[pb] = min(pb * 32 + l31, W - 1);

    for (int l = 0; l < L; ++l) {
        const bool last = l + 1 == L;
        const float *src = l == 0 ? a.x : a.map[(l - 1) & 1];
        float *dst = last ? a.out : a.map[l & 1];
        if (tid >= 64 && tid < 64 + C) {
            s_epi[tid - 64] = a.scale[l][tid - 64];
            s_epi[128 + tid - 64] = a.shift[l][tid - 64];
        }
        if (l > 0) {
            // ---- rows y-1 .. y+1 of layer l-1: wait for their words (every slice of each), take their maxima
            if (wid == 0) {
                const int rr = y - 1 + lane / NS, ss = lane % NS;
                const bool need = lane < 3 * NS && rr >= 0 && rr < H;
                const unsigned long long *wp = a.words + (long)(l - 1) * H * NS + (need ? rr * NS + ss : 0);
                unsigned long long wv = (unsigned long long)l << 32;   // rows outside the image: done, maximum 0
                long long spins = 0;
                bool ok = false;
                while (true) {
                    if (need) wv = __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ok = __all((int)(wv >> 32) == l);
                    if (ok) break;
                    ++spins;
                    const bool timed_out = spins > a.spin_limit;
                    const bool peer_gone = !timed_out && (spins & 63) == 0 && __hip_atomic_load(a.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                    if (timed_out || peer_gone) {
                        if (lane == 0) {
                            *s_abort = 1;
                            if (timed_out) { atomicAdd(a.sticky, 1); __hip_atomic_store(a.abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
                        }
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (ok) {
                    const float m = wave_finite_absmax(need ? finite_abs(__uint_as_float((unsigned)wv)) : 0.f);
                    if (lane == 0) s_m[0] = m;
                }
            }
            __syncthreads();
            if (*(volatile int *)s_abort) {
                // (uniform after the barrier.)  This workgroup stops here and voids its part of the run's result
                const int nco = NCBW * 32;
                for (int i = tid; i < nco * W; i += 512) a.out[(long)(s * nco + i / W) * plane + (long)y * W + (i % W)] = __uint_as_float(0x7fc00000u);
                if (tid == 0 && a.amax_out) a.amax_out[blockIdx.x] = 0.f;
                return;
            }
            m_in = s_m[0];
        }
        // the zero column either side of every staged row (every layer: the partial tiles overlay them)
        for (int i = tid; i < 2 * G8 * 3 * 2; i += 512) {
            const int side = i & 1, q = i >> 1;            // q = (piece * G8 + group) * 3 + row
            *reinterpret_cast<u32x4 *>(smem + ((long)q * WP + (side ? WP - 1 : 0)) * 16) = u32x4{0u, 0u, 0u, 0u};
        }
        // ---- the three input rows: 16 channels of one (chunk, row, pixel) per task; all loads in flight, then conversion
        const float sx = f16_scale_of(m_in), inv = 1.f / sx;
        {
            float v[NTK][16];
            bool okr[NTK];
            const int ntask = nchunk * 3 * W;
#pragma unroll
            for (int u = 0; u < NTK; ++u) {
                const int task = tid + u * 512;
                const int tk = min(task, ntask - 1);
                const int q = tk / W, px = tk - q * W, c = q / 3, t = q - 3 * c;
                const int yy = y + t - 1;
                okr[u] = task < ntask && yy >= 0 && yy < H;
                const float *sp = src + ((long)c * 16 * H + (okr[u] ? yy : y)) * W + px;
#pragma unroll
                for (int ch = 0; ch < 16; ++ch) v[u][ch] = __hip_atomic_load(sp + ch * plane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int u = 0; u < NTK; ++u) {
                const int task = tid + u * 512;
                if (task < ntask) {
                    const int q = task / W, px = task - q * W, c = q / 3, t = q - 3 * c;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        u32x4 q2[2];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            unsigned p0, p1;
                            const float x0 = okr[u] ? v[u][8 * h + 2 * e] : 0.f, x1 = okr[u] ? v[u][8 * h + 2 * e + 1] : 0.f;
                            split2h_pair(x0 * inv, x1 * inv, p0, p1);
                            q2[0][e] = p0; q2[1][e] = p1;
                        }
                        const int entry = ((c * 2 + h) * 3 + t) * WP + px + 1;
                        *reinterpret_cast<u32x4 *>(smem + entry * 16) = q2[0];
                        *reinterpret_cast<u32x4 *>(smem + piece + entry * 16) = q2[1];
                    }
                }
            }
        }
        __syncthreads();
        // the epilogue's two powers of two: the halves of sx * sw's exponent (neither product over- or underflows before y does)
        float out_sx, out_sw;
        f16_out_scales(sx, *a.wscale[l], out_sx, out_sw);

        // ---- matrix phase
        f32x16 acc[NPB];
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[pb][r] = 0.f;
        const unsigned char *w_this = a.w[l] + wlane, *w_next = a.w[last ? l : l + 1] + wlane;
        for (int ci = 0; ci < nper; ++ci) {
            const int ch = kp * nper + ci;
            const unsigned char *w_refill = ci + 1 < nper ? w_this + (ci + 1) * 2048 : w_next;
            const unsigned char *bin = smem + ((ch * 2 + half) * 3 * WP) * 16;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int toff = ((t / 3) * WP + (t % 3)) * 16;
                // pixel blocks in groups of three: fragments of one group in registers at a time; within a group the three products go
                // round the accumulators (split_arith.hpp's F16X3_A / _B order, smallest terms first: w1 b0, w0 b1, w0 b0)
#pragma unroll
                for (int g0 = 0; g0 < NPB; g0 += 3) {
                    constexpr int GMAX = 3;
                    u32x4 b[GMAX][2];
#pragma unroll
                    for (int j = 0; j < GMAX; ++j)
                        if (g0 + j < NPB) {
                            b[j][0] = *reinterpret_cast<const u32x4 *>(bin + toff + pxb[g0 + j] * 16);
                            b[j][1] = *reinterpret_cast<const u32x4 *>(bin + piece + toff + pxb[g0 + j] * 16);
                        }
#pragma unroll
                    for (int j = 0; j < GMAX; ++j)
                        if (g0 + j < NPB)
                            acc[g0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wr[t][1]), __builtin_bit_cast(f16x8, b[j][0]), acc[g0 + j], 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < GMAX; ++j)
                        if (g0 + j < NPB)
                            acc[g0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wr[t][0]), __builtin_bit_cast(f16x8, b[j][1]), acc[g0 + j], 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < GMAX; ++j)
                        if (g0 + j < NPB)
                            acc[g0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wr[t][0]), __builtin_bit_cast(f16x8, b[j][0]), acc[g0 + j], 0, 0, 0);
                }
                // the slot's next tenant: the next chunk's tap, or the next layer's first chunk (in flight across the hand-off)
                load_w(w_refill, t, wr[t]);
            }
        }
        __syncthreads();   // everybody is through with the staged rows: the partial tiles may overlay them
        // ---- the K parts' partial tiles: pixel block pb is finished by part pb % KS, the others hand theirs over
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb) {
            const int o = pb % KS;
            if (kp != o) {
                const int idx = kp < o ? kp : kp - 1;
                float *d = s_red + ((long)((idx * NCBW + cbw) * NPB + pb) * 16) * 64 + lane;
#pragma unroll
                for (int r = 0; r < 16; ++r) d[r * 64] = acc[pb][r];
            }
        }
        __syncthreads();
        float lm = 0.f;
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb) {
            const int o = pb % KS;
            if (kp == o) {
                f32x16 tot;
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[r] = 0.f;
#pragma nounroll
                for (int k = 0; k < KS; ++k) {   // fixed order, whoever finishes the block (not unrolled: KS - 1 partial tiles in registers at once spill)
                    if (k == o) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) tot[r] += acc[pb][r];
                    } else {
                        const int idx = k < o ? k : k - 1;
                        const float *d = s_red + ((long)((idx * NCBW + cbw) * NPB + pb) * 16) * 64 + lane;
#pragma unroll
                        for (int r = 0; r < 16; ++r) tot[r] += d[r * 64];
                    }
                }
                const int px = pb * 32 + l31;
                float *yo = dst + (long)y * W + px;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    float vv = tot[r] * out_sx * out_sw;
                    vv = relu_nan(vv);
                    vv = fmaf(vv, s_epi[co], s_epi[128 + co]);
                    if (px < W) {
                        if (last) yo[co * plane] = vv;
                        else __hip_atomic_store(yo + co * plane, vv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        lm = fmaxf(lm, finite_abs(vv));
                    }
                }
            }
        }
        lm = wave_finite_absmax(lm);
        if (lane == 0) s_wmax[wid] = lm;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's row stores have left (write-through): the word may follow
        __syncthreads();
        if (tid == 0) {
            float m = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) m = fmaxf(m, s_wmax[i]);
            if (last) {
                if (a.amax_out) a.amax_out[blockIdx.x] = m;
            } else {
                __hip_atomic_store(a.words + (long)l * H * NS + blockIdx.x, ((unsigned long long)(l + 1) << 32) | __float_as_uint(m), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

struct RunConfig { int NS, NCBW, KS, NPB, NTK; size_t data_bytes, map_bytes; };

// how a run of this geometry is cut, or false: not served (the caller keeps one launch per layer)
bool run_config(int channels, int h, int w, RunConfig &c) {
    if ((channels != 64 && channels != 128) || h < 1 || w < 1 || w > 160) return false;
    if (channels == 64) c.NS = 1;
    else c.NS = h * 4 <= RUN_MAX_WG ? 4 : 2;
    if (h * c.NS > RUN_MAX_WG) return false;
    c.NCBW = channels / 32 / c.NS; c.KS = 8 / c.NCBW;
    if (c.NCBW * c.KS != 8 || (channels / 16) % c.KS) return false;
    c.NPB = w <= 64 ? 2 : w <= 96 ? 3 : 5;
    const int ntask = channels / 16 * 3 * w;
    c.NTK = ntask <= 1024 ? 2 : ntask <= 2048 ? 4 : 0;
    if (!c.NTK) return false;
    const size_t rows = (size_t)2 * (channels / 8) * 3 * (w + 2) * 16, red = (size_t)(c.KS - 1) * c.NCBW * c.NPB * 4096;
    c.data_bytes = (std::max(rows, red) + 255) / 256 * 256;
    if (c.data_bytes + RUN_TAIL_LDS > 160 * 1024) return false;
    c.map_bytes = ((size_t)channels * h * w * sizeof(float) + 255) / 256 * 256;
    return true;
}

// the instantiations that are built: the cuts run_config makes of the geometries the BEV backbone has
struct RunBuild { int NPB, NCBW, KS, NTK; int (*launch)(dim3, dim3, size_t, hipStream_t, int, const RunArgs &); };
template <int NPB, int NCBW, int KS, int NTK>
constexpr RunBuild run_build() { return {NPB, NCBW, KS, NTK, &launch_lds<k_conv3x3_run_f16<NPB, NCBW, KS, NTK>, RunArgs>}; }
constexpr RunBuild RUN_BUILDS[] = {run_build<5, 2, 4, 4>(), run_build<3, 2, 4, 4>(), run_build<3, 2, 4, 2>(), run_build<2, 2, 4, 4>(),
                                   run_build<2, 2, 4, 2>(), run_build<2, 1, 8, 4>(), run_build<2, 1, 8, 2>(), run_build<3, 1, 8, 4>()};
}  // namespace

extern "C" size_t lav_conv3x3_run_f16_workspace_bytes(int channels, int h, int w, int nlayers) {
    RunConfig c;
    if (nlayers < 1 || nlayers > RUN_MAX || !run_config(channels, h, w, c)) return 0;
    return RUN_MAPS_OFF + 2 * c.map_bytes;
}

extern "C" size_t lav_conv3x3_run_f16_lds_bytes(int channels, int h, int w) {
    RunConfig c;
    if (!run_config(channels, h, w, c)) return 0;
    return c.data_bytes + RUN_TAIL_LDS;
}

extern "C" int lav_conv3x3_run_f16_amax_count(int channels, int h, int w) {
    RunConfig c;
    return run_config(channels, h, w, c) ? h * c.NS : 0;
}

extern "C" size_t lav_conv3x3_run_f16_weight_bytes(int channels) {
    if (channels < 32 || channels % 32) return 0;
    return (size_t)9 * (channels / 32) * (channels / 16) * 2 * 1024;
}

extern "C" int lav_conv3x3_run_f16(int channels, int h, int w, int nlayers, const float *x, const void *const *w_f16, const float *const *scale,
                                   const float *const *shift, float *out, const float *amax_in, int amax_in_count, float *amax_out, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    RunConfig c;
    LAV_REQUIRE(nlayers >= 1 && nlayers <= RUN_MAX, "lav_conv3x3_run_f16: 1..%d layers", RUN_MAX);
    LAV_REQUIRE(run_config(channels, h, w, c), "lav_conv3x3_run_f16: %d channels on %d x %d is not served (lav_conv3x3_run_f16_workspace_bytes returns 0)", channels, h, w);
    LAV_REQUIRE(x && w_f16 && scale && shift && out && amax_in && amax_in_count >= 1, "lav_conv3x3_run_f16: null argument (the first layer's scale comes from amax_in)");
    LAV_REQUIRE(workspace && workspace_bytes >= RUN_MAPS_OFF + 2 * c.map_bytes, "lav_conv3x3_run_f16: workspace too small");
    const RunBuild *build = nullptr;
    for (const RunBuild &b : RUN_BUILDS)
        if (c.NPB == b.NPB && c.NCBW == b.NCBW && c.KS == b.KS && c.NTK == b.NTK) build = &b;
    LAV_REQUIRE(build, "lav_conv3x3_run_f16: tile %d x %d / %d / %d not built", c.NPB, c.NCBW, c.KS, c.NTK);
    RunArgs a;
    char *ws = static_cast<char *>(workspace);
    const size_t wbytes = lav_conv3x3_run_f16_weight_bytes(channels);
    for (int i = 0; i < RUN_MAX; ++i) {
        const int j = layer_of(i, nlayers);
        LAV_REQUIRE(w_f16[j] && scale[j] && shift[j], "lav_conv3x3_run_f16: null argument of layer %d", j);
        a.w[i] = static_cast<const unsigned char *>(w_f16[j]);
        a.wscale[i] = reinterpret_cast<const float *>(a.w[i] + wbytes);   // (the packing's tail: conv_split.hpp)
        a.scale[i] = scale[j]; a.shift[i] = shift[j];
    }
    a.x = x; a.out = out;
    a.map[0] = reinterpret_cast<float *>(ws + RUN_MAPS_OFF); a.map[1] = reinterpret_cast<float *>(ws + RUN_MAPS_OFF + c.map_bytes);
    a.amax_in = amax_in; a.amax_in_count = amax_in_count; a.amax_out = amax_out;
    a.abort_word = reinterpret_cast<int *>(ws); a.words = reinterpret_cast<unsigned long long *>(ws + 16);
    a.sticky = reinterpret_cast<int *>(ws + RUN_STICKY_OFF);
    a.spin_limit = chain_spin_limit();
    a.C = channels; a.H = h; a.W = w; a.L = nlayers; a.NS = c.NS; a.data_bytes = (int)c.data_bytes;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nwg = h * c.NS;
    // the words this launch polls and its abort word, at zero (a memset node under capture, replayed first)
    LAV_HIP(hipMemsetAsync(ws, 0, (16 + (size_t)(nlayers - 1) * nwg * 8 + 15) / 16 * 16, st));
    const size_t lds = c.data_bytes + RUN_TAIL_LDS;
    const int tok = timer_begin("conv3x3_run", st);
    const int rc = build->launch(dim3(nwg), dim3(512), lds, st, 160 * 1024, a);
    timer_end(tok, st);
    return rc;
}

extern "C" int lav_conv3x3_run_f16_status(const void *workspace, int *h_timeouts_launches2, void *stream) {
    LAV_REQUIRE(workspace && h_timeouts_launches2, "lav_conv3x3_run_f16_status: bad argument");
    return read_status(workspace, RUN_STICKY_OFF, h_timeouts_launches2, static_cast<hipStream_t>(stream));
}
