// The trainers' visual logs (lav/utils/logger.py: log_bev_info, log_lidar_info, log_seg_info, log_bra_info), composed from tensors that
// a logged step left in HBM.  One frame format for the four of them, described by three host-built tables: panels (a destination
// rectangle and a source: image, label map, logits, planes, colour), primitives (dots, segments, filled convex polygons, each clipped
// to the panel it names, later over earlier) and rows of text.  The specification is lav_amd.train.log_view.log_view_numpy and the two
// agree bit for bit (tests/test_gpu_log_view.py).  What is pinned against the reference and what cannot be (matplotlib's rasterisation
// and figure scaling, its font, imshow's normalisation) is said there.
//
// One C call, up to three stream operations: the PLANES panels' minimum / maximum words are zeroed, k_log_minmax finds them (ordered
// integer keys of the float64 means under atomicMax: the result does not depend on the order of arrival), k_log_compose writes the
// frame.  A workgroup of k_log_compose owns a 32 x 8 tile of the frame, one pixel per lane: the pixel takes its panel's colour, then the
// last primitive that covers it, then the text.  The primitives are scanned in drawing order, 256 at a time, those whose clipped box
// touches the tile are copied to an LDS list, and the list is drawn and emptied whenever the next scan could overflow it and at the end:
// a tile touched by more primitives than the list holds draws all of them, in order.
//
// Floating point is left to the device in two places, both in float64 with contraction off (lav_amd/build.py): the PLANES mean (the
// sum in channel order, divided by the channel count) and its grey level floor((m - lo) * 255 / (hi - lo)).
#include "common.hpp"
#include "view_cover.hpp"

#pragma clang fp contract(off)

namespace {
using namespace lav;
constexpr int TW = 32, TH = 8, THREADS = 256;
constexpr int LIST = 512;              // culled records a tile keeps in LDS; a scan adds at most THREADS
constexpr int REC = 16;                // ints per primitive: kind, x0, y0, x1, y1, radius, colour, panel, x2, y2, x3, y3, vertices, 3 unused
constexpr int PREC = 16;               // ints per panel: kind, x, y, w, h, channels, colour, palette offset, palette entries, label bytes, source (lo, hi), 4 unused
constexpr int MAX_PANELS = 8;
constexpr int GLYPH_W = 5, GLYPH_H = 7, GLYPH_STEP = 6;
enum { IMAGE_U8 = 0, LABELS = 1, LOGITS = 2, PLANES = 3, SOLID = 4 };
enum { DOT = 0, SEGMENT = 1, CONVEX = 2 };
static_assert(LIST >= 2 * THREADS && TW * TH == THREADS, "one pixel per lane; a scan never overflows the list");

__device__ __forceinline__ const void *source_of(const int *p) {
    return reinterpret_cast<const void *>((unsigned long long)(unsigned)p[10] | (unsigned long long)(unsigned)p[11] << 32);
}

// float64 mean of pixel i over the C planes: the sum in channel order, divided by C
__device__ __forceinline__ double plane_mean(const float *src, int C, size_t plane, size_t i) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s = s + (double)src[(size_t)c * plane + i];
    return s / (double)C;
}
__device__ __forceinline__ bool finite64(double v) { return (__double_as_longlong(v) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll; }
// an unsigned key that orders like the finite double it stands for; never 0
__device__ __forceinline__ unsigned long long key_of(double v) {
    const long long b = __double_as_longlong(v);
    return b < 0 ? ~(unsigned long long)b : (unsigned long long)b | 0x8000000000000000ull;
}
__device__ __forceinline__ double value_of(unsigned long long k) {
    return __longlong_as_double((long long)(k & 0x8000000000000000ull ? k & 0x7fffffffffffffffull : ~k));
}

// mm[2 p] = largest key of panel p's finite means, mm[2 p + 1] = largest inverted key (the smallest mean); 0 where none is finite
__global__ __launch_bounds__(THREADS) void k_log_minmax(const int *__restrict__ panels, unsigned long long *__restrict__ mm) {
    const int *p = panels + blockIdx.y * PREC;
    if (p[0] != PLANES) return;
    const float *src = static_cast<const float *>(source_of(p));
    const size_t plane = (size_t)p[3] * p[4];
    unsigned long long hi = 0, lo = 0;
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < plane; i += (size_t)gridDim.x * THREADS) {
        const double m = plane_mean(src, p[5], plane, i);
        if (finite64(m)) {
            const unsigned long long k = key_of(m);
            hi = k > hi ? k : hi;
            lo = ~k > lo ? ~k : lo;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long h2 = __shfl_xor(hi, d), l2 = __shfl_xor(lo, d);
        hi = h2 > hi ? h2 : hi;
        lo = l2 > lo ? l2 : lo;
    }
    if ((threadIdx.x & 63) == 0 && hi != 0) {
        atomicMax(mm + 2 * blockIdx.y, hi);
        atomicMax(mm + 2 * blockIdx.y + 1, lo);
    }
}

__device__ __forceinline__ int palette_colour(long long label, const int *p, const unsigned char *__restrict__ pal, int npal) {
    // label i + 1 -> palette[i]; everything else black (visualize_semantic_processed)
    if (label < 1 || label > p[8]) return 0;
    const long long at = (long long)p[7] + label - 1;
    if (at < 0 || at >= npal) return 0;
    return pal[at * 3] | pal[at * 3 + 1] << 8 | pal[at * 3 + 2] << 16;
}

// the colour of panel p at its own pixel (x, y)
__device__ __forceinline__ int panel_pixel(const int *p, int slot, int x, int y, const unsigned char *__restrict__ pal, int npal,
                                           const unsigned long long *__restrict__ mm) {
    const int w = p[3], h = p[4], C = p[5];
    const size_t plane = (size_t)w * h, at = (size_t)y * w + x;
    const void *src = source_of(p);
    switch (p[0]) {
    case IMAGE_U8: {
        const unsigned char *s = static_cast<const unsigned char *>(src) + at * 3;
        return s[0] | s[1] << 8 | s[2] << 16;
    }
    case LABELS: {
        const long long v = p[9] == 1 ? (long long)static_cast<const unsigned char *>(src)[at]
                          : p[9] == 4 ? (long long)static_cast<const int *>(src)[at] : static_cast<const long long *>(src)[at];
        return palette_colour(v, p, pal, npal);
    }
    case LOGITS: {
        // np.argmax: the first maximum, and a NaN counts as one
        const float *s = static_cast<const float *>(src) + at;
        float bv = s[0];
        int best = 0;
        for (int c = 1; c < C && bv == bv; ++c) {
            const float v = s[(size_t)c * plane];
            if (v > bv || v != v) { bv = v; best = c; }
        }
        return palette_colour(best, p, pal, npal);
    }
    case PLANES: {
        const unsigned long long khi = mm[2 * slot], klo = ~mm[2 * slot + 1];
        const double m = plane_mean(static_cast<const float *>(src), C, plane, at);
        int g = 0;
        if (khi != 0 && finite64(m)) {
            const double hi = value_of(khi), lo = value_of(klo);
            if (hi != lo) {
                const double v = floor(((m - lo) * 255.0) / (hi - lo));
                g = v >= 0.0 ? (v <= 255.0 ? (int)v : 255) : 0;
            }
        }
        return g | g << 8 | g << 16;
    }
    case SOLID: return p[6] & 0xffffff;
    default: return 0;
    }
}

// the record's box in its panel's coordinates
__device__ __forceinline__ void box_of(const int *r, int &x0, int &y0, int &x1, int &y1) {
    if (r[0] == CONVEX) {
        x0 = min(min(r[1], r[3]), min(r[8], r[10])); x1 = max(max(r[1], r[3]), max(r[8], r[10]));
        y0 = min(min(r[2], r[4]), min(r[9], r[11])); y1 = max(max(r[2], r[4]), max(r[9], r[11]));
    } else {
        x0 = min(r[1], r[3]) - r[5]; x1 = max(r[1], r[3]) + r[5];
        y0 = min(r[2], r[4]) - r[5]; y1 = max(r[2], r[4]) + r[5];
    }
}

// a filled convex polygon of four vertices (a triangle repeats its last): inside its box, every edge function >= 0 or every one <= 0
__device__ __forceinline__ bool covers_convex(const int *r, int x, int y) {
    const int vx[4] = {r[1], r[3], r[8], r[10]}, vy[4] = {r[2], r[4], r[9], r[11]};
    bool pos = true, neg = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = (k + 1) & 3;
        const long long e = ((long long)vx[j] - vx[k]) * ((long long)y - vy[k]) - ((long long)vy[j] - vy[k]) * ((long long)x - vx[k]);
        pos = pos && e >= 0;
        neg = neg && e <= 0;
    }
    return pos || neg;
}

// whether record r (frame box [fx0, fx1] x [fy0, fy1] already clipped to its panel) covers frame pixel (x, y); (ox, oy) its panel's origin
__device__ __forceinline__ bool record_covers(const int *r, int ox, int oy, int x, int y) {
    const int lx = x - ox, ly = y - oy;
    int x0, y0, x1, y1;
    box_of(r, x0, y0, x1, y1);
    if (lx < x0 || lx > x1 || ly < y0 || ly > y1) return false;
    if (r[0] == CONVEX) return covers_convex(r, lx, ly);
    return (r[0] == DOT || r[0] == SEGMENT) && covers(r, lx, ly);
}

__global__ __launch_bounds__(THREADS) void k_log_compose(const int *__restrict__ panels, int npanels, const int *__restrict__ prims, int nprims,
                                                         const unsigned char *__restrict__ text, const int *__restrict__ origins, int nrows,
                                                         int text_len, const unsigned char *__restrict__ font, const unsigned char *__restrict__ pal,
                                                         int npal, const unsigned long long *__restrict__ mm, int fh, int fw,
                                                         unsigned char *__restrict__ out) {
    __shared__ int s_pan[MAX_PANELS * PREC];
    __shared__ int s_list[LIST * REC];
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const int tx1 = min(tx0 + TW, fw) - 1, ty1 = min(ty0 + TH, fh) - 1;
    const int x = tx0 + tid % TW, y = ty0 + tid / TW;
    const bool inside = x < fw && y < fh;
    if (tid < npanels * PREC) s_pan[tid] = panels[tid];
    if (tid == 0) s_count = 0;
    __syncthreads();

    int colour = 0;
    if (inside) {
        for (int k = npanels - 1; k >= 0; --k) {          // the last panel that holds the pixel
            const int *p = s_pan + k * PREC;
            if (x >= p[1] && x < p[1] + p[3] && y >= p[2] && y < p[2] + p[4]) {
                colour = panel_pixel(p, k, x - p[1], y - p[2], pal, npal, mm);
                break;
            }
        }
    }

    for (int base = 0; base < nprims; base += THREADS) {   // (every lane runs every round: the barriers are uniform)
        const int i = base + tid;
        if (i < nprims) {
            const int *r = prims + (size_t)i * REC;
            const unsigned pn = (unsigned)r[7];
            if (pn < (unsigned)npanels) {
                const int *p = s_pan + pn * PREC;
                int x0, y0, x1, y1;
                box_of(r, x0, y0, x1, y1);
                // the box in frame coordinates, clipped to the panel and tested against the tile
                const int fx0 = max(x0 + p[1], p[1]), fx1 = min(x1 + p[1], p[1] + p[3] - 1);
                const int fy0 = max(y0 + p[2], p[2]), fy1 = min(y1 + p[2], p[2] + p[4] - 1);
                if (fx0 <= fx1 && fy0 <= fy1 && fx0 <= tx1 && fx1 >= tx0 && fy0 <= ty1 && fy1 >= ty0) {
                    int *d = s_list + atomicAdd(&s_count, 1) * REC;
#pragma unroll
                    for (int k = 0; k < 12; k += 2) {
                        d[k] = r[k]; d[k + 1] = r[k + 1];
                        lds_store_fence();                      // (no pairing of adjacent 64-bit LDS stores: common.hpp)
                    }
                    d[12] = i;                                  // drawing order
                }
            }
        }
        __syncthreads();
        const int n = s_count;                                  // the same in every lane
        __syncthreads();
        if (n + THREADS > LIST || base + THREADS >= nprims) {   // the next scan could overflow the list, or there is none: draw and empty it
            if (inside) {
                int best = -1;
                for (int k = 0; k < n; ++k) {
                    const int *r = s_list + k * REC;
                    if (r[12] <= best) continue;
                    const int *p = s_pan + r[7] * PREC;
                    if (x < p[1] || x >= p[1] + p[3] || y < p[2] || y >= p[2] + p[4]) continue;
                    if (record_covers(r, p[1], p[2], x, y)) { best = r[12]; colour = r[6] & 0xffffff; }
                }
            }
            __syncthreads();
            if (tid == 0) s_count = 0;
            __syncthreads();
        }
    }

    if (!inside) return;
    // text: a row has its baseline-left at its origin, a glyph's bottom row on it, glyphs GLYPH_STEP apart; white
    for (int l = 0; l < nrows; ++l) {
        const int gx = x - origins[2 * l], gy = y - (origins[2 * l + 1] - (GLYPH_H - 1));
        if (gx < 0 || gy < 0 || gy >= GLYPH_H) continue;
        const int ci = gx / GLYPH_STEP, cc = gx % GLYPH_STEP;
        if (ci >= text_len || cc >= GLYPH_W) continue;
        const int ch = text[(size_t)l * text_len + ci] & 127;
        if (font[ch * GLYPH_H + gy] >> (GLYPH_W - 1 - cc) & 1) colour = 0xffffff;
    }
    unsigned char *o = out + ((size_t)y * fw + x) * 3;
    o[0] = (unsigned char)(colour & 255); o[1] = (unsigned char)(colour >> 8 & 255); o[2] = (unsigned char)(colour >> 16 & 255);
}
}  // namespace

extern "C" int lav_log_view(const void *panels, int npanels, const void *prims, int nprims, const unsigned char *text, const int *origins,
                            int nrows, int text_len, const unsigned char *font, const unsigned char *palette, int npalette,
                            unsigned long long *minmax, int frame_h, int frame_w, unsigned char *out, void *stream) {
    LAV_REQUIRE(font && minmax && out, "lav_log_view: null argument");
    LAV_REQUIRE(npanels >= 0 && npanels <= MAX_PANELS && (panels || npanels == 0), "lav_log_view: %d panels (at most %d)", npanels, MAX_PANELS);
    LAV_REQUIRE(nprims >= 0 && nprims <= 65536 && (prims || nprims == 0), "lav_log_view: %d records (at most 65536)", nprims);
    LAV_REQUIRE(nrows >= 0 && nrows <= 64 && text_len >= 0 && text_len <= 4096 && ((text && origins && text_len >= 1) || nrows == 0),
                "lav_log_view: %d rows of %d characters", nrows, text_len);
    LAV_REQUIRE(npalette >= 0 && npalette <= 4096 && (palette || npalette == 0), "lav_log_view: %d palette entries", npalette);
    LAV_REQUIRE(frame_h >= 1 && frame_w >= 1 && frame_h <= 16384 && frame_w <= 16384, "lav_log_view: frame %d x %d", frame_h, frame_w);
    LAV_REQUIRE((reinterpret_cast<uintptr_t>(panels) & 3) == 0 && (reinterpret_cast<uintptr_t>(prims) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(origins) & 3) == 0 && (reinterpret_cast<uintptr_t>(minmax) & 7) == 0,
                "lav_log_view: tables must be 4-byte, the minimum / maximum words 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("log_view", st);
    LAV_HIP(hipMemsetAsync(minmax, 0, (size_t)MAX_PANELS * 2 * sizeof(unsigned long long), st));
    if (npanels > 0) {
        hipLaunchKernelGGL(k_log_minmax, dim3(64, npanels), dim3(THREADS), 0, st, static_cast<const int *>(panels), minmax);
    }
    hipLaunchKernelGGL(k_log_compose, dim3((frame_w + TW - 1) / TW, (frame_h + TH - 1) / TH), dim3(THREADS), 0, st,
                       static_cast<const int *>(panels), npanels, static_cast<const int *>(prims), nprims, text, origins, nrows, text_len, font,
                       palette, npalette, minmax, frame_h, frame_w, out);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
