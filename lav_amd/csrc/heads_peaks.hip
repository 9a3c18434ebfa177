// lav_heads_at_peaks: the box / orientation heads (conv3x3 -> ReLU -> eval BatchNorm -> ConvTranspose2d k 3, stride 2, padding 1,
// output_padding 1; lidar.py Head) evaluated at the peak rows of lav_extract_peaks only, instead of on the whole 2H x 2W map of
// which the frame reads 2 x 15 pixels.
//
// One output pixel (x, y) of the transposed convolution depends on the hidden pixels (y >> 1 [+ 1 if y is odd], x >> 1 [+ 1 if x is
// odd]) - 1, 2 or 4 of them - through the taps ky = 1 (y even) or ky = 2, 0 (y odd: hidden rows (y - 1) / 2 and (y + 1) / 2), likewise
// kx; hidden pixels at index H resp. W do not exist.  Each hidden pixel is a 3 x 3 x cin window of the zero-padded feature map.
//
// One workgroup of 1024 threads per (row, head), no hand-off, no workspace.  All four hidden pixels of the 2 x 2 block are always
// computed (the weight stream is the cost, not the FMAs); the tail selects the ones the parity asks for.  The channels are walked in
// chunks of 384 (one pass for the frame's map): the chunk's 4 x 4 feature patches are staged in LDS, then lane (k8, c8) of wave v owns k = 128 i + 8 v + k8
// and the hidden channels 8 c8 .. 8 c8 + 7: four LDS reads and two 16-byte weight loads (a wave reads 2 KB of the packed
// [k][64 channels] weights contiguously) feed 32 fmaf.  The 128 K slices (chains of 9 cin / 128 products: short chains are what keeps
// the fp32 sum as accurate as the dense kernels' matrix accumulators) are combined in a fixed order: the lanes k8 ^ 4, then k8 ^ 2
// of a wave through lane swaps, the remaining 32 slices through LDS.  That last sum and the tail's sum over the hidden channels carry
// their rounding errors along (two-sum) - 32 + 64 terms, free beside the stream.  Every sum's order depends on (cin, hidden) alone: results
// do not depend on the other rows, on the launch, or on anything measured at run time.
//
// Rows: a row is live when score > -1e4 (lav_extract_peaks writes -1e5 for "no candidate") and 0 <= x < 2W, 0 <= y < 2H (NaN fails
// every comparison).  The coordinates are converted and clamped BEFORE anything is addressed with them and the row's verdict only
// selects between the computed values and zeros at the store: a bad row cannot form an address.
#include "common.hpp"

namespace {
using namespace lav;

constexpr int HP_THREADS = 1024, HP_HID = 64, HP_CC = 384, HP_MAX_HEADS = 4, HP_MAX_OUTS = 4;
constexpr int HP_SLICE = 256 + 8;   // floats between two slices in LDS: the two lane groups that store land in different banks

// s + x with the rounding error of the sum added to c (Knuth's two-sum: exact for any two floats short of overflow)
__device__ __forceinline__ void add_carry(float &s, float &c, float x) {
    const float t = s + x, bb = t - s;
    c += (s - (t - bb)) + (x - bb);
    s = t;
}

// the value of lane ^ 32 resp. lane ^ 16, on the VALU ((x, x) swapped: one result is the own value, the other the partner's)
__device__ __forceinline__ float lane_xor32(float v) {
    const unsigned u = __float_as_uint(v);
    const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(a[0] ^ a[1] ^ u);
}
__device__ __forceinline__ float lane_xor16(float v) {
    const unsigned u = __float_as_uint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return __uint_as_float(a[0] ^ a[1] ^ u);
}

struct HeadsPeaksArgs {
    const float *feat, *rows;
    float *out;
    int cin, H, W, nrows, ncol, nheads;
    const float *w1[HP_MAX_HEADS];     // packed [kpad][64]: k = ci * 9 + ky * 3 + kx, zeros beyond 9 cin and beyond the hidden width
    const float *scale[HP_MAX_HEADS], *shift[HP_MAX_HEADS];
    const float *wt[HP_MAX_HEADS];     // ConvTranspose2d layout [hidden][outs][3][3]
    const float *bias[HP_MAX_HEADS];   // or null
    int hidden[HP_MAX_HEADS], outs[HP_MAX_HEADS], col[HP_MAX_HEADS];
};

__global__ __launch_bounds__(HP_THREADS) void k_heads_at_peaks(HeadsPeaksArgs a) {
    __shared__ float s_patch[HP_CC * 16];
    __shared__ float s_part[32 * HP_SLICE];
    __shared__ float s_hid[HP_HID * 4];
    __shared__ float s_tail[HP_MAX_OUTS * HP_HID];
    const int tid = threadIdx.x, row = blockIdx.x, g = blockIdx.y;
    const float *r = a.rows + (long)row * 3;
    const float score = r[0], fx = r[1], fy = r[2];
    const bool live = score > -1e4f && fx >= 0.f && fx < (float)(2 * a.W) && fy >= 0.f && fy < (float)(2 * a.H);
    const int x = min(max(live ? (int)fx : 0, 0), 2 * a.W - 1), y = min(max(live ? (int)fy : 0, 0), 2 * a.H - 1);
    const int hx0 = x >> 1, hy0 = y >> 1;
    const int K = 9 * a.cin, kpad = (K + 127) / 128 * 128;
    const float *w1 = a.w1[g];
    const int lane = tid & 63, wv = tid >> 6, k8 = lane >> 3, c8 = lane & 7;

    float acc[8][4];
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[c][p] = 0.f;

    for (int c0 = 0; c0 < a.cin; c0 += HP_CC) {   // (one pass at cin <= 384)
        const int cn = min(HP_CC, a.cin - c0);
        // the chunk's 4 x 4 feature patch per channel: s_patch[ci][r][q] = feature (c0 + ci, hy0 - 1 + r, hx0 - 1 + q), 0 outside the map
        for (int e = tid; e < cn * 16; e += HP_THREADS) {
            const int ci = c0 + (e >> 4), yy = hy0 - 1 + ((e >> 2) & 3), xx = hx0 - 1 + (e & 3);
            const bool in = yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
            const long at = in ? ((long)ci * a.H + yy) * a.W + xx : 0;
            const float v = a.feat[at];
            s_patch[e] = in ? v : 0.f;
        }
        __syncthreads();
        // k = ci * 9 + ky * 3 + kx runs over the chunk's 9 cn products, rounded up to the packed rows (zero weights; the patch index is clamped)
        const int kb = 9 * c0, kn = min(9 * cn, kpad - kb), kr = (kn + 127) / 128 * 128;
        const float4 *wp = reinterpret_cast<const float4 *>(w1 + (long)(kb + 8 * wv + k8) * HP_HID + 8 * c8);
#pragma unroll 3
        for (int kk = 8 * wv + k8; kk < kr; kk += 128, wp += 128 * HP_HID / 4) {
            const float4 w0 = wp[0], w4 = wp[1];
            const int kc = min(kk, kn - 1), ci = kc / 9, t = kc - ci * 9, ky = t / 3, kx = t - ky * 3;
            const float *f = s_patch + ci * 16 + ky * 4 + kx;
            const float f0 = kk < kn ? f[0] : 0.f, f1 = kk < kn ? f[1] : 0.f, f2 = kk < kn ? f[4] : 0.f, f3 = kk < kn ? f[5] : 0.f;
            const float wc[8] = {w0.x, w0.y, w0.z, w0.w, w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                acc[c][0] = fmaf(wc[c], f0, acc[c][0]);
                acc[c][1] = fmaf(wc[c], f1, acc[c][1]);
                acc[c][2] = fmaf(wc[c], f2, acc[c][2]);
                acc[c][3] = fmaf(wc[c], f3, acc[c][3]);
            }
        }
        __syncthreads();
    }
    // the eight K slices of a wave: (k8, k8 ^ 4), then (k8, k8 ^ 2) - a + b is the same float in both lanes; lanes k8 < 2 store
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float v = acc[c][p];
            v = v + lane_xor32(v);
            v = v + lane_xor16(v);
            if (k8 < 2) s_part[(wv * 2 + k8) * HP_SLICE + (c * 4 + p) * 8 + c8] = v;
        }
    __syncthreads();
    const int hid = a.hidden[g], outs = a.outs[g];
    if (tid < 256) {   // element j * 8 + c8 of a slice: hidden channel 8 c8 + (j >> 2), pixel j & 3
        float v = s_part[tid], carry = 0.f;
        for (int s = 1; s < 32; ++s) add_carry(v, carry, s_part[s * HP_SLICE + tid]);
        v += carry;
        const int j = tid >> 3, ch = 8 * (tid & 7) + (j >> 2), p = j & 3;
        const bool have = ch < hid;
        const float sc = a.scale[g][have ? ch : 0], sh = a.shift[g][have ? ch : 0];
        s_hid[ch * 4 + p] = have ? fmaf(relu_nan(v), sc, sh) : 0.f;   // ConvLayer's relu_pre order: ReLU, then the folded BatchNorm
    }
    __syncthreads();
    // the transposed convolution's taps at this pixel: hidden pixel (py, px) of the 2 x 2 block through (ky, kx)
    if (tid < outs * HP_HID) {
        const int o = tid >> 6, ch = tid & 63;
        float t = 0.f;
        if (ch < hid) {
            const float *w = a.wt[g] + ((long)ch * outs + o) * 9;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int py = p >> 1, px = p & 1;
                const bool use = (py == 0 || ((y & 1) && hy0 + 1 < a.H)) && (px == 0 || ((x & 1) && hx0 + 1 < a.W));
                const int ky = (y & 1) ? (py ? 0 : 2) : 1, kx = (x & 1) ? (px ? 0 : 2) : 1;
                const float wv_ = w[ky * 3 + kx];
                t = use ? fmaf(s_hid[ch * 4 + p], wv_, t) : t;
            }
        }
        s_tail[tid] = t;
    }
    __syncthreads();
    float *orow = a.out + (long)row * a.ncol;
    if (tid < outs) {
        float v = s_tail[tid * HP_HID], carry = 0.f;
        for (int ch = 1; ch < HP_HID; ++ch) add_carry(v, carry, s_tail[tid * HP_HID + ch]);
        if (a.bias[g]) add_carry(v, carry, a.bias[g][tid]);
        orow[a.col[g] + tid] = live ? v + carry : 0.f;
    }
    if (g == 0 && tid >= 64 && tid < 67) orow[tid - 64] = r[tid - 64];   // (score, x, y) as they came
}
}  // namespace

extern "C" size_t lav_heads_at_peaks_packed_floats(int cin, int hidden) {
    if (cin < 1 || hidden < 1 || hidden > HP_HID) return 0;
    return (size_t)((9l * cin + 127) / 128 * 128) * HP_HID;
}

extern "C" int lav_heads_at_peaks(const float *feat, int cin, int h, int w, const float *rows, int ncls, int max_det, int nheads,
                                  const float *const *w1_packed, const float *const *scale, const float *const *shift,
                                  const float *const *wt, const float *const *bias, const int *hidden, const int *outs, float *out,
                                  void *stream) {
    LAV_REQUIRE(feat && rows && out && w1_packed && scale && shift && wt && bias && hidden && outs, "lav_heads_at_peaks: null argument");
    LAV_REQUIRE(cin >= 1 && h >= 1 && w >= 1 && (long)cin * h * w < (1l << 31) && h < (1 << 29) && w < (1 << 29), "lav_heads_at_peaks: bad map size");
    LAV_REQUIRE(ncls >= 1 && max_det >= 1 && (long)ncls * max_det <= 65535, "lav_heads_at_peaks: bad row count");
    LAV_REQUIRE(nheads >= 1 && nheads <= HP_MAX_HEADS, "lav_heads_at_peaks: 1 .. %d heads", HP_MAX_HEADS);
    HeadsPeaksArgs a;
    a.feat = feat; a.rows = rows; a.out = out;
    a.cin = cin; a.H = h; a.W = w; a.nrows = ncls * max_det; a.nheads = nheads;
    int col = 3;
    for (int g = 0; g < HP_MAX_HEADS; ++g) {
        const bool on = g < nheads;
        if (on) {
            LAV_REQUIRE(hidden[g] >= 1 && hidden[g] <= HP_HID && outs[g] >= 1 && outs[g] <= HP_MAX_OUTS,
                        "lav_heads_at_peaks: head %d: hidden width in 1 .. %d and 1 .. %d outputs expected", g, HP_HID, HP_MAX_OUTS);
            LAV_REQUIRE(w1_packed[g] && scale[g] && shift[g] && wt[g], "lav_heads_at_peaks: head %d: null weights", g);
        }
        a.w1[g] = on ? w1_packed[g] : nullptr; a.scale[g] = on ? scale[g] : nullptr; a.shift[g] = on ? shift[g] : nullptr;
        a.wt[g] = on ? wt[g] : nullptr; a.bias[g] = on ? bias[g] : nullptr;
        a.hidden[g] = on ? hidden[g] : 0; a.outs[g] = on ? outs[g] : 0; a.col[g] = col;
        col += a.outs[g];
    }
    a.ncol = col;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("heads_at_peaks", st);
    hipLaunchKernelGGL(k_heads_at_peaks, dim3(a.nrows, nheads), dim3(HP_THREADS), 0, st, a);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
