// Image augmentation for the camera trainers (train_seg / train_bra_v2 --augment): the reference's augment(0.5)
// (lav/utils/augmenter.py - seven imgaug operations in random order, each with probability 0.5) as ONE launch per batch.
// The semantics are this library's own restatement (include/lav_amd.h, lav_amd/data/augment.py): parity with imgaug is UNPINNED,
// there is no imgaug and there are no recorded outputs to compare with.  What is pinned: this kernel against
// lav_amd.data.augment.augment_numpy - bit for bit for every op but noise (logf / cosf differ from NumPy's by an ulp, which can
// move a value across a .5 boundary: at most one grey level on at most 1e-4 of the pixel-channels).
//
// A workgroup owns a TW x TH output tile of one image.  It loads the tile with the halo its chain needs (blur consumes 2, elastic 6:
// |displacement| <= 3.5 plus the cubic footprint; each occurs at most once, so 8 covers every order) into LDS, one dword per pixel
// (R | G << 8 | B << 16: consecutive lanes on consecutive banks), and runs the image's active ops in the image's order between two
// LDS buffers; intermediate images never reach HBM.  The rectangle an op must produce is the tile grown by the radii of the
// neighbourhood ops still to come, clipped to the image: border rules refer to the image edge, never to the tile edge.  Pointwise
// ops are pure functions of (value, global pixel, parameters) - their random words come from Philox4x32-10 with the counter
// (x, y, sample, tag | op << 8 | draw) - so they are recomputed in the halo, and a run of consecutive pointwise ops stays in registers.
// The elastic warp's raw displacement field is such a function too; it is staged in LDS once instead of 25 Philox calls per pixel.
// The op list is uniform per workgroup: every branch on it is scalar.
#include "common.hpp"
#include "philox.hpp"

#pragma clang fp contract(off)

namespace {
using namespace lav;
constexpr int TW = 64, TH = 32, HALO = 8;
constexpr int RW = TW + 2 * HALO, RH = TH + 2 * HALO;       // the LDS region: 80 x 48 pixels
constexpr int FW = TW + 8, FH = TH + 8;                      // the raw field: elastic's output (at most the tile + 2) + 2 for its smoothing
constexpr int THREADS = 256;

struct Rect {
    int x0, y0, x1, y1;
    __device__ __forceinline__ int width() const { return x1 - x0; }
    __device__ __forceinline__ int count() const { return (x1 - x0) * (y1 - y0); }
};

__device__ __forceinline__ float uniform24(unsigned word) { return (float)(word >> 8) * 5.9604644775390625e-8f; }          // [0, 1)
__device__ __forceinline__ float uniform24_open(unsigned word) { return (float)((word >> 8) + 1u) * 5.9604644775390625e-8f; }  // (0, 1]
__device__ __forceinline__ float gauss(unsigned a, unsigned b) {
    return sqrtf(-2.f * logf(uniform24_open(a))) * cosf(6.2831854820251465f * uniform24(b));
}
__device__ __forceinline__ float round_clip(float v) { return fminf(fmaxf(rintf(v), 0.f), 255.f); }
// multiply and contrast: a float32 parameter times an 8-bit value is exact in float64, so this is the correctly rounded result (a
// float32 product rounds ONTO a tie for m = 1/1.2 at every twelfth grey level: 9 m = 7.49999982 -> 7.5 -> 8)
__device__ __forceinline__ float round_clip(double v) { return (float)fmin(fmax(rint(v), 0.0), 255.0); }
// reflect-101 of an index at most 2 outside [0, n)
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n >= 3) {
        i = i < 0 ? -i : i;
        return i >= n ? 2 * (n - 1) - i : i;
    }
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    i = i < 0 ? i + p : i;
    return i < n ? i : p - i;
}
// Keys' cubic convolution weights, a = -0.75, of the taps at -1, 0, 1, 2 around floor(position); [0, 1, 0, 0] exactly at t = 0
__device__ __forceinline__ void cubic(float t, float (&wt)[4]) {
    const float t1 = t + 1.f, t2 = 1.f - t;
    wt[0] = ((-0.75f * t1 + 3.75f) * t1 - 6.f) * t1 + 3.f;
    wt[1] = ((1.25f * t - 2.25f) * t) * t + 1.f;
    wt[2] = ((1.25f * t2 - 2.25f) * t2) * t2 + 1.f;
    wt[3] = ((1.f - wt[0]) - wt[1]) - wt[2];
}
__device__ __forceinline__ bool is_pointwise(int op) { return op >= LAV_AUG_NOISE && op <= LAV_AUG_GRAYSCALE; }

__device__ __forceinline__ void pointwise(int op, const lav_augment_params &P, int x, int y, unsigned k0, unsigned k1, float &r, float &g, float &b) {
    const unsigned tag = P.tag | ((unsigned)op << 8);
    if (op == LAV_AUG_NOISE) {
        unsigned q[4];
        philox4x32((unsigned)x, (unsigned)y, P.sample, tag, k0, k1, q);
        const float z0 = gauss(q[0], q[1]);
        float z1 = z0, z2 = z0;
        if ((P.per_channel >> LAV_AUG_NOISE) & 1) {
            z1 = gauss(q[2], q[3]);
            philox4x32((unsigned)x, (unsigned)y, P.sample, tag | 1u, k0, k1, q);
            z2 = gauss(q[0], q[1]);
        }
        r = round_clip(r + P.noise_scale * z0);
        g = round_clip(g + P.noise_scale * z1);
        b = round_clip(b + P.noise_scale * z2);
    } else if (op == LAV_AUG_DROPOUT) {
        unsigned q[4];
        philox4x32((unsigned)x, (unsigned)y, P.sample, tag, k0, k1, q);
        const bool pc = (P.per_channel >> LAV_AUG_DROPOUT) & 1;
        const float u0 = uniform24(q[0]), u1 = pc ? uniform24(q[1]) : u0, u2 = pc ? uniform24(q[2]) : u0;
        r = u0 < P.dropout_p ? 0.f : r;
        g = u1 < P.dropout_p ? 0.f : g;
        b = u2 < P.dropout_p ? 0.f : b;
    } else if (op == LAV_AUG_MULTIPLY) {
        r = round_clip((double)r * (double)P.multiply[0]);
        g = round_clip((double)g * (double)P.multiply[1]);
        b = round_clip((double)b * (double)P.multiply[2]);
    } else if (op == LAV_AUG_CONTRAST) {
        r = round_clip(128.0 + (double)P.contrast[0] * ((double)r - 128.0));
        g = round_clip(128.0 + (double)P.contrast[1] * ((double)g - 128.0));
        b = round_clip(128.0 + (double)P.contrast[2] * ((double)b - 128.0));
    } else {   // LAV_AUG_GRAYSCALE
        const float gr = (float)((4899 * (int)r + 9617 * (int)g + 1868 * (int)b + 8192) >> 14);
        r = round_clip(r + P.gray_alpha * (gr - r));
        g = round_clip(g + P.gray_alpha * (gr - g));
        b = round_clip(b + P.gray_alpha * (gr - b));
    }
}

__global__ __launch_bounds__(THREADS) void k_augment(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, int h, int w,
                                                     const lav_augment_params *__restrict__ params, unsigned k0, unsigned k1) {
    __shared__ unsigned s_img[2][RW * RH];
    __shared__ float2 s_field[FW * FH];
    const lav_augment_params &P = params[blockIdx.z];   // uniform: scalar loads
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, ox = tx0 - HALO, oy = ty0 - HALO;
    const size_t base = (size_t)blockIdx.z * h * w * 3;

    // the ops that run, four bits each, in order; every op at most once, whatever the record holds
    unsigned list = 0, used = 0;
    int nops = 0, margin = 0;
#pragma unroll
    for (int k = 0; k < LAV_AUG_OPS; ++k) {
        const int op = P.order[k];
        if (op >= 0 && op < LAV_AUG_OPS && ((P.active >> op) & 1) && !((used >> op) & 1)) {
            used |= 1u << op;
            list |= (unsigned)op << (4 * nops++);
            margin += op == LAV_AUG_BLUR ? 2 : op == LAV_AUG_ELASTIC ? 6 : 0;
        }
    }
    // the tile grown by m, inside the image (m <= HALO: inside the LDS region too)
    auto grown = [&](int m) { return Rect{max(tx0 - m, 0), max(ty0 - m, 0), min(tx0 + TW + m, w), min(ty0 + TH + m, h)}; };
    auto at = [&](int x, int y) { return (y - oy) * RW + (x - ox); };

    {
        const Rect R = grown(margin);
        const int rw = R.width(), cnt = R.count();
        for (int i = threadIdx.x; i < cnt; i += THREADS) {
            const int y = R.y0 + i / rw, x = R.x0 + i % rw;
            const unsigned char *p = in + base + ((size_t)y * w + x) * 3;
            s_img[0][at(x, y)] = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
        }
    }
    __syncthreads();

    int cur = 0, k = 0;
    while (k < nops) {
        const int op = (list >> (4 * k)) & 15;
        if (is_pointwise(op)) {
            int k2 = k + 1;
            while (k2 < nops && is_pointwise((list >> (4 * k2)) & 15)) ++k2;
            const Rect R = grown(margin);
            const int rw = R.width(), cnt = R.count();
            for (int i = threadIdx.x; i < cnt; i += THREADS) {
                const int y = R.y0 + i / rw, x = R.x0 + i % rw;
                const unsigned v = s_img[cur][at(x, y)];
                float r = (float)(v & 255u), g = (float)((v >> 8) & 255u), b = (float)((v >> 16) & 255u);
                for (int j = k; j < k2; ++j) pointwise((list >> (4 * j)) & 15, P, x, y, k0, k1, r, g, b);
                s_img[cur][at(x, y)] = (unsigned)r | (unsigned)g << 8 | (unsigned)b << 16;   // in place: a thread's own pixel
            }
            k = k2;
        } else if (op == LAV_AUG_BLUR) {
            margin -= 2;
            const Rect R = grown(margin);
            const int rw = R.width(), cnt = R.count();
            for (int i = threadIdx.x; i < cnt; i += THREADS) {
                const int y = R.y0 + i / rw, x = R.x0 + i % rw;
                int xs[5];
#pragma unroll
                for (int t = 0; t < 5; ++t) xs[t] = reflect101(x + t - 2, w) - ox;
                float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const unsigned *row = s_img[cur] + (reflect101(y + j - 2, h) - oy) * RW;
                    float hs[3] = {0.f, 0.f, 0.f};
#pragma unroll
                    for (int t = 0; t < 5; ++t) {
                        const unsigned v = row[xs[t]];
                        const float c[3] = {(float)(v & 255u), (float)((v >> 8) & 255u), (float)((v >> 16) & 255u)};
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) hs[ch] = t == 0 ? P.blur_w[0] * c[ch] : hs[ch] + P.blur_w[t] * c[ch];
                    }
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) acc[ch] = j == 0 ? P.blur_w[0] * hs[ch] : acc[ch] + P.blur_w[j] * hs[ch];
                }
                s_img[cur ^ 1][at(x, y)] = (unsigned)round_clip(acc[0]) | (unsigned)round_clip(acc[1]) << 8 | (unsigned)round_clip(acc[2]) << 16;
            }
            cur ^= 1;
            ++k;
        } else {   // LAV_AUG_ELASTIC
            margin -= 6;
            const Rect R = grown(margin);
            const Rect F{max(R.x0 - 2, 0), max(R.y0 - 2, 0), min(R.x1 + 2, w), min(R.y1 + 2, h)};
            const int fw = F.width(), fcnt = min(F.count(), FW * FH);
            const unsigned tag = P.tag | ((unsigned)LAV_AUG_ELASTIC << 8);
            for (int i = threadIdx.x; i < fcnt; i += THREADS) {
                unsigned q[4];
                philox4x32((unsigned)(F.x0 + i % fw), (unsigned)(F.y0 + i / fw), P.sample, tag, k0, k1, q);
                s_field[i] = make_float2(2.f * uniform24(q[0]) - 1.f, 2.f * uniform24(q[1]) - 1.f);
            }
            __syncthreads();
            const int rw = R.width(), cnt = R.count();
            for (int i = threadIdx.x; i < cnt; i += THREADS) {
                const int y = R.y0 + i / rw, x = R.x0 + i % rw;
                int xs[5];
#pragma unroll
                for (int t = 0; t < 5; ++t) xs[t] = reflect101(x + t - 2, w) - F.x0;
                float dx = 0.f, dy = 0.f;
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const int rowoff = (reflect101(y + j - 2, h) - F.y0) * fw;
                    float hx = 0.f, hy = 0.f;
#pragma unroll
                    for (int t = 0; t < 5; ++t) {
                        const int fi = min(max(rowoff + xs[t], 0), FW * FH - 1);   // (in range for every record; clamped for a broken one)
                        const float2 f = s_field[fi];
                        hx = t == 0 ? P.field_w[0] * f.x : hx + P.field_w[t] * f.x;
                        hy = t == 0 ? P.field_w[0] * f.y : hy + P.field_w[t] * f.y;
                    }
                    dx = j == 0 ? P.field_w[0] * hx : dx + P.field_w[j] * hx;
                    dy = j == 0 ? P.field_w[0] * hy : dy + P.field_w[j] * hy;
                }
                dx = dx * P.elastic_alpha;
                dy = dy * P.elastic_alpha;
                const float sx = (float)x - dx, sy = (float)y - dy;
                const float fx = floorf(sx), fy = floorf(sy);
                float wx[4], wy[4];
                cubic(sx - fx, wx);
                cubic(sy - fy, wy);
                // (a displacement beyond the specified 3.5 - a broken record - reads zeros, not another tile's LDS)
                const int ix = (int)fminf(fmaxf(fx, -1e6f), 1e6f) - 1, iy = (int)fminf(fmaxf(fy, -1e6f), 1e6f) - 1;
                float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int yy = iy + j;
                    float rowv[3] = {0.f, 0.f, 0.f};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int xx = ix + t;
                        const bool inside = xx >= 0 && xx < w && yy >= 0 && yy < h && xx >= ox && xx < ox + RW && yy >= oy && yy < oy + RH;
                        const unsigned v = inside ? s_img[cur][at(xx, yy)] : 0u;
                        const float c[3] = {(float)(v & 255u), (float)((v >> 8) & 255u), (float)((v >> 16) & 255u)};
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) rowv[ch] = t == 0 ? wx[0] * c[ch] : rowv[ch] + wx[t] * c[ch];
                    }
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) acc[ch] = j == 0 ? wy[0] * rowv[ch] : acc[ch] + wy[j] * rowv[ch];
                }
                s_img[cur ^ 1][at(x, y)] = (unsigned)round_clip(acc[0]) | (unsigned)round_clip(acc[1]) << 8 | (unsigned)round_clip(acc[2]) << 16;
            }
            cur ^= 1;
            ++k;
        }
        __syncthreads();
    }

    const Rect R = grown(0);
    const int rw = R.width(), cnt = R.count();
    for (int i = threadIdx.x; i < cnt; i += THREADS) {
        const int y = R.y0 + i / rw, x = R.x0 + i % rw;
        const unsigned v = s_img[cur][at(x, y)];
        unsigned char *p = out + base + ((size_t)y * w + x) * 3;
        p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16);
    }
}
}  // namespace

extern "C" int lav_augment_u8(const unsigned char *in, unsigned char *out, int n, int h, int w, const lav_augment_params *params,
                              unsigned long long seed, void *stream) {
    static_assert(sizeof(lav_augment_params) == 128, "lav_augment_params is 32 words");
    LAV_REQUIRE(n >= 0 && h >= 1 && w >= 1 && ((in && out && params) || n == 0), "lav_augment_u8: bad argument");
    if (n == 0) return LAV_OK;
    LAV_REQUIRE(n <= 65535, "lav_augment_u8: %d images in one launch (at most 65535)", n);
    const size_t bytes = (size_t)n * h * w * 3;
    LAV_REQUIRE(in + bytes <= out || out + bytes <= in, "lav_augment_u8: in and out overlap (halos are read from in)");
    LAV_REQUIRE((h + TH - 1) / TH <= 65535 && (long)w + TW < (long)INT32_MAX, "lav_augment_u8: image %d x %d too large", h, w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((w + TW - 1) / TW, (h + TH - 1) / TH, n);
    const int tok = timer_begin("augment_u8", st);
    hipLaunchKernelGGL(k_augment, grid, dim3(THREADS), 0, st, in, out, h, w, params, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32));
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
