// The agent's per-tick debug frame (team_code_v2/lav_agent_fast.py:459-518, 567-581), rendered from what the frame pipeline left in
// HBM: the cameras and the telephoto image resized to the LiDAR panel's height, the LiDAR bird's-eye histogram with the ego plan, the
// forecasts, the vehicle boxes and the route target drawn on it, the predicted BEV - side by side, halved, with four lines of text.
// The specification is lav_amd.agent.debug_view.compose_numpy and the two agree bit for bit (tests/test_gpu_debug_view.py).  What the
// specification pins against the reference and what it cannot (OpenCV's rasterisers, its resize, its font: UNPINNED) is said there.
//
// One C call, up to three stream operations: the count workspace is zeroed, k_view_hist places every point of the cloud, and
// k_view_compose writes the frame.  Everything that needs the reference's float expressions is computed on the host and uploaded as
// integers: the drawing records (lav_amd.agent.debug_view.primitives), the text and the index / weight tables of the two resizes
// (lav_amd.data.image.resize_linear_table).  Left for the device in floating point are the histogram's binning (float64 against
// np.linspace's edges: start + i * step, the last edge the stop value itself) and the BEV panel's float32 mean; this file is compiled
// with FMA contraction off and with correctly rounded float32 division (lav_amd/build.py).
//
// A workgroup of k_view_compose owns a 32 x 16 tile of the frame.  It builds the tile's footprint of the full-size canvas ONCE in
// LDS - camera pixels through the first resize, LiDAR pixels from the counts through the 11-entry grey table, then the last-drawn
// record that covers the pixel - so the 320 x 2293 canvas never reaches HBM; then the second resize reads the footprint, the text is
// laid over it and the RGB bytes are stored.  The frame is int(W / 2) x int(H / 2), so the second resize's scale lies in [2, 2 + 1 / n]
// for a frame side of n pixels and a tile's footprint is at most 69 x 37 canvas pixels (FW, FH below hold it; a table that asked for
// more would be clamped to the footprint - wrong pixels, no stray access).  Before it draws, the workgroup culls the records against
// its footprint's rectangle of the LiDAR panel into an LDS list; a pixel takes the covering record with the largest index.  When more
// than LIST records survive (every forecast dot on one spot), the tile walks the global list from its end instead: the same pixels.
#include "common.hpp"
#include "view_cover.hpp"      // covers(), touches(): the records' coverage rules, shared with log_view.hip

#pragma clang fp contract(off)

namespace {
using namespace lav;
constexpr int TW = 32, TH = 16, THREADS = 256;
constexpr int FW = 72, FH = 40;        // the largest canvas footprint of a tile
constexpr int LIST = 512;              // culled records a tile keeps in LDS (8 ints each)
constexpr int REC = 8;                 // ints per record: kind, x0, y0, x1, y1, radius, colour (r | g << 8 | b << 16), unused
constexpr int GLYPH_W = 5, GLYPH_H = 7, GLYPH_STEP = 6, LINES = 4, TEXT_X = 4, TEXT_Y = 10, TEXT_DY = 10;
constexpr int HIST_MAX = 10;

struct Geometry {
    int rh, rw, th, tw;                // camera image and telephoto image (rows, columns)
    int H, w1, w2, wl, wb;             // canvas height; panel widths: cameras, telephoto, LiDAR, BEV
    int fh, fw;                        // frame
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// np.linspace(start, stop, n + 1)[i]
__device__ __forceinline__ double edge(double start, double stop, double step, int n, int i) { return i >= n ? stop : start + (double)i * step; }

// np.histogramdd's bin of v over those edges: half-open bins, the last edge inclusive; -1 outside (and for NaN)
__device__ __forceinline__ int bin_of(double v, double start, double stop, double step, int n) {
    if (!(v >= start && v <= stop)) return -1;
    if (v == stop) return n - 1;
    int i = clampi((int)((v - start) / step), 0, n - 1);
    // the quotient is within a bin of the truth: settle against the edges themselves
    for (int k = 0; k < 3 && i > 0 && v < edge(start, stop, step, n, i); ++k) --i;
    for (int k = 0; k < 3 && i < n - 1 && v >= edge(start, stop, step, n, i + 1); ++k) ++i;
    return i;
}

__global__ __launch_bounds__(THREADS) void k_view_hist(const float *__restrict__ cloud, int npts, int stride, double x0, double x1, int nxb,
                                                       double y0, double y1, int nyb, unsigned *__restrict__ counts) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= npts) return;
    const float *p = cloud + (size_t)i * stride;
    const double x = (double)p[0], y = (double)p[1];
    const int bx = bin_of(x, x0, x1, (x1 - x0) / (double)nxb, nxb);
    const int by = bin_of(y, y0, y1, (y1 - y0) / (double)nyb, nyb);
    if (bx < 0 || by < 0) return;
    atomicAdd(counts + (size_t)bx * nyb + by, 1u);
}

// one pixel of a camera panel through the first resize: rows / cols are (i0, i1, w0, w1) tables
__device__ __forceinline__ void camera_pixel(const unsigned char *__restrict__ img, int h, int w, const int4 tx, const int4 ty, unsigned char *dst) {
    const int xa = clampi(tx.x, 0, w - 1), xb = clampi(tx.y, 0, w - 1), ya = clampi(ty.x, 0, h - 1), yb = clampi(ty.y, 0, h - 1);
    const unsigned char *r0 = img + (size_t)ya * w * 3, *r1 = img + (size_t)yb * w * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int s0 = r0[xa * 3 + c] * tx.z + r0[xb * 3 + c] * tx.w;
        const int s1 = r1[xa * 3 + c] * tx.z + r1[xb * 3 + c] * tx.w;
        dst[c] = (unsigned char)min((((ty.z * (s0 >> 4)) >> 16) + ((ty.w * (s1 >> 4)) >> 16) + 2) >> 2, 255);
    }
}

__global__ __launch_bounds__(THREADS) void k_view_compose(const unsigned char *__restrict__ rgb, const unsigned char *__restrict__ tel,
                                                          const float *__restrict__ bev, const unsigned *__restrict__ counts,
                                                          const int *__restrict__ prims, int nprims, const unsigned char *__restrict__ text,
                                                          int text_len, const unsigned char *__restrict__ font, const unsigned char *__restrict__ lut,
                                                          const int4 *__restrict__ tables, Geometry g, unsigned char *__restrict__ out) {
    __shared__ unsigned char s_canvas[FH * FW * 3];
    __shared__ int s_list[LIST * REC];
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int4 *cam_x = tables, *tel_x = cam_x + g.w1, *cam_y = tel_x + g.w2, *tel_y = cam_y + g.H, *fin_x = tel_y + g.H, *fin_y = fin_x + g.fw;
    const int W = g.w1 + g.w2 + g.wl + g.wb;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const int tw = min(TW, g.fw - tx0), th = min(TH, g.fh - ty0);
    // the tile's footprint of the canvas: the tables are monotone, their first and last entries of the tile bound it
    const int fx0 = clampi(fin_x[tx0].x, 0, W - 1), fy0 = clampi(fin_y[ty0].x, 0, g.H - 1);
    const int fw = clampi(fin_x[tx0 + tw - 1].y + 1 - fx0, 1, min(FW, W - fx0)), fh = clampi(fin_y[ty0 + th - 1].y + 1 - fy0, 1, min(FH, g.H - fy0));
    const int xl = g.w1 + g.w2;                                            // first canvas column of the LiDAR panel
    // the footprint's rectangle of the LiDAR panel, in panel coordinates (empty when the tile lies beside the panel)
    const int bx0 = max(fx0 - xl, 0), bx1 = min(fx0 + fw - 1 - xl, g.wl - 1), by0 = fy0, by1 = fy0 + fh - 1;
    const bool on_lidar = bx0 <= bx1;

    if (tid == 0) s_count = 0;
    __syncthreads();
    if (on_lidar) {
        for (int i = tid; i < nprims; i += THREADS) {
            const int *r = prims + (size_t)i * REC;
            if (!touches(r, bx0, by0, bx1, by1)) continue;
            const int slot = atomicAdd(&s_count, 1);
            if (slot < LIST) {
                int *d = s_list + slot * REC;
#pragma unroll
                for (int k = 0; k < REC - 1; ++k) d[k] = r[k];
                d[REC - 1] = i;                                             // drawing order
            }
        }
    }
    __syncthreads();
    const int nlist = s_count;                                             // the same in every lane
    const bool listed = nlist <= LIST;

    for (int i = tid; i < fw * fh; i += THREADS) {
        const int cy = fy0 + i / fw, cx = fx0 + i % fw;
        unsigned char *dst = s_canvas + i * 3;
        if (cx < g.w1) {
            camera_pixel(rgb, g.rh, g.rw, cam_x[cx], cam_y[cy], dst);
        } else if (cx < xl) {
            camera_pixel(tel, g.th, g.tw, tel_x[cx - g.w1], tel_y[cy], dst);
        } else if (cx < xl + g.wl) {
            const int px = cx - xl;
            const unsigned n = counts[(size_t)(g.H - 1 - cy) * g.wl + px];
            const int grey = lut[n > (unsigned)HIST_MAX ? HIST_MAX : n];
            int colour = grey | grey << 8 | grey << 16;
            if (listed) {
                int best = -1;
                for (int k = 0; k < nlist; ++k) {
                    const int *r = s_list + k * REC;
                    if (r[REC - 1] > best && touches(r, px, cy, px, cy) && covers(r, px, cy)) { best = r[REC - 1]; colour = r[6]; }
                }
            } else {
                for (int k = nprims - 1; k >= 0; --k) {
                    const int *r = prims + (size_t)k * REC;
                    if (touches(r, px, cy, px, cy) && covers(r, px, cy)) { colour = r[6]; break; }
                }
            }
            dst[0] = (unsigned char)(colour & 255); dst[1] = (unsigned char)(colour >> 8 & 255); dst[2] = (unsigned char)(colour >> 16 & 255);
        } else {
            // (255 * pred_bev.mean(axis=0)).astype(uint8) in float32: ((a + b) + c) / 3, times 255, truncated
            const size_t plane = (size_t)g.H * g.wb, at = (size_t)cy * g.wb + (cx - xl - g.wl);
            const float m = __fdiv_rn((bev[at] + bev[plane + at]) + bev[2 * plane + at], 3.0f) * 255.0f;
            const int v = m >= 0.0f ? (m < 256.0f ? (int)m : 255) : 0;        // (NaN -> 0)
            dst[0] = dst[1] = dst[2] = (unsigned char)v;
        }
    }
    __syncthreads();

    for (int i = tid; i < tw * th; i += THREADS) {
        const int y = ty0 + i / tw, x = tx0 + i % tw;
        const int4 ax = fin_x[x], ay = fin_y[y];
        const int xa = clampi(ax.x - fx0, 0, fw - 1), xb = clampi(ax.y - fx0, 0, fw - 1), ya = clampi(ay.x - fy0, 0, fh - 1), yb = clampi(ay.y - fy0, 0, fh - 1);
        const unsigned char *r0 = s_canvas + ya * fw * 3, *r1 = s_canvas + yb * fw * 3;
        int v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s0 = r0[xa * 3 + c] * ax.z + r0[xb * 3 + c] * ax.w;
            const int s1 = r1[xa * 3 + c] * ax.z + r1[xb * 3 + c] * ax.w;
            v[c] = min((((ay.z * (s0 >> 4)) >> 16) + ((ay.w * (s1 >> 4)) >> 16) + 2) >> 2, 255);
        }
        // text: line l has its baseline at row TEXT_Y + l * TEXT_DY, a glyph's bottom row on it, glyphs GLYPH_STEP apart from TEXT_X
        const int gx = x - TEXT_X;
        if (gx >= 0) {
            const int ci = gx / GLYPH_STEP, cc = gx % GLYPH_STEP;
            if (ci < text_len && cc < GLYPH_W) {
#pragma unroll
                for (int l = 0; l < LINES; ++l) {
                    const int gy = y - (TEXT_Y + l * TEXT_DY - (GLYPH_H - 1));
                    if (gy >= 0 && gy < GLYPH_H) {
                        const int ch = text[l * text_len + ci] & 127;
                        if (font[ch * GLYPH_H + gy] >> (GLYPH_W - 1 - cc) & 1) v[0] = v[1] = v[2] = 255;
                    }
                }
            }
        }
        unsigned char *o = out + ((size_t)y * g.fw + x) * 3;
        o[0] = (unsigned char)v[0]; o[1] = (unsigned char)v[1]; o[2] = (unsigned char)v[2];
    }
}
}  // namespace

extern "C" int lav_debug_view(const unsigned char *rgb, int rgb_h, int rgb_w, const unsigned char *tel, int tel_h, int tel_w, const float *cloud,
                              int npts, int stride, const float *bev, int bev_w, const void *prims, int nprims, const unsigned char *text,
                              int text_len, const unsigned char *font, const unsigned char *lut, const int *tables, double x_start, double x_stop,
                              int x_bins, double y_start, double y_stop, int y_bins, int w_rgb, int w_tel, unsigned *counts, unsigned char *out,
                              void *stream) {
    LAV_REQUIRE(rgb && tel && bev && text && font && lut && tables && counts && out, "lav_debug_view: null argument");
    LAV_REQUIRE(npts >= 0 && (cloud || npts == 0) && (stride >= 2 || npts == 0), "lav_debug_view: cloud of %d rows of %d floats", npts, stride);
    LAV_REQUIRE(nprims >= 0 && nprims <= 65536 && (prims || nprims == 0), "lav_debug_view: %d records (at most 65536)", nprims);
    LAV_REQUIRE((reinterpret_cast<uintptr_t>(tables) & 15) == 0 && (reinterpret_cast<uintptr_t>(prims) & 3) == 0, "lav_debug_view: tables must be 16-byte, records 4-byte aligned");
    const int lim = 16384;
    LAV_REQUIRE(rgb_h >= 1 && rgb_w >= 1 && tel_h >= 1 && tel_w >= 1 && rgb_h <= lim && rgb_w <= lim && tel_h <= lim && tel_w <= lim, "lav_debug_view: image sizes");
    LAV_REQUIRE(x_bins >= 2 && y_bins >= 1 && x_bins <= lim && y_bins <= lim && x_stop > x_start && y_stop > y_start, "lav_debug_view: bad grid");
    LAV_REQUIRE(w_rgb >= 1 && w_tel >= 1 && bev_w >= 1 && w_rgb <= lim && w_tel <= lim && bev_w <= lim, "lav_debug_view: panel widths");
    LAV_REQUIRE(text_len >= 1 && text_len <= 4096, "lav_debug_view: text length %d", text_len);
    Geometry g{rgb_h, rgb_w, tel_h, tel_w, x_bins, w_rgb, w_tel, y_bins, bev_w, x_bins / 2, (w_rgb + w_tel + y_bins + bev_w) / 2};
    // a tile side of T frame pixels reads at most (T - 1)(2 + 1 / n) + 3 < 2 T + 2 canvas pixels for a frame side of n >= T pixels
    // (a smaller frame has a canvas side of at most 2 T - 1)
    static_assert(2 * TW + 2 <= FW && 2 * TH + 2 <= FH, "tile footprint");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("debug_view", st);
    LAV_HIP(hipMemsetAsync(counts, 0, (size_t)x_bins * y_bins * sizeof(unsigned), st));
    if (npts > 0) {
        hipLaunchKernelGGL(k_view_hist, dim3((npts + THREADS - 1) / THREADS), dim3(THREADS), 0, st, cloud, npts, stride, x_start, x_stop, x_bins,
                           y_start, y_stop, y_bins, counts);
    }
    hipLaunchKernelGGL(k_view_compose, dim3((g.fw + TW - 1) / TW, (g.fh + TH - 1) / TH), dim3(THREADS), 0, st, rgb, tel, bev, counts,
                       static_cast<const int *>(prims), nprims, text, text_len, font, lut, reinterpret_cast<const int4 *>(tables), g, out);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
