// The data loaders' BEV map stacks, rendered behind the upload (train_bev_v2 / train_full_v2 --bev-on-device): every output plane is
//     out = ( W2( crop( W1(src) ) ) > 0 )
// with W1, W2 OpenCV's 8-bit bilinear warpAffine as lav_amd/data/image.py restates it (fixed point: the inverse map in 1/1024 pixel
// integers, coordinates cut to 1/32 pixel, weights (32 - a)(32 - b) * 32, + 2^14 >> 15, constant border 0) and crop a shift with zero
// fill.  ONE launch renders a batch of planes, each with its own twelve coefficients and shift; the specification is
// lav_amd.data.bev_stack.bev_stack_numpy and the two agree bit for bit (tests/test_gpu_bev_stack.py).  Parity with OpenCV itself is
// UNPINNED, as it is for the restatement.
//
// The inverse map is float64 with every product and sum rounded separately (this file is compiled with FMA contraction off), only
// along the edges of a rectangle: X(x, y) = rint((i00 x) 1024) + rint((i01 y + b1) 1024) + 16 is a column term plus a row term, so a
// workgroup fills one table per column and one per row (64-bit integers in LDS) and a pixel costs two integer additions.  Both terms
// are monotone in their index, which makes the bounding box of a rectangle's source footprint exact from its four edge values:
// footprint() below, the same code on the host (lav_bev_stack_tile_paths) and on the device.
//
// A workgroup owns a 64 x 32 output tile.  It derives the tile's footprint in the intermediate image W1(src) (through W2 and the shift)
// and that footprint's footprint in src (through W1), loads the latter into LDS, computes the former ONCE into LDS - the intermediate
// image never reaches HBM and no intermediate pixel is computed four times - and interpolates the tile from it.  An identity W1 (the
// current frame's five planes of a temporal stack) or W2 (the single-frame loaders) skips its stage: the fixed-point path passes an
// identity exactly.  A rotation's footprints always fit (at most 70 x 70 and 101 x 101 bytes for this tile); a map that shrinks the
// image can exceed the LDS budget, and such a tile takes the direct path: every output pixel interpolates its four intermediate pixels
// from global memory (16 source bytes per pixel, the naive form).  The choice is per tile and uniform in the workgroup.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {
using namespace lav;
constexpr int TW = 64, TH = 32, THREADS = 256;
constexpr int MID_CAP = 8192;        // bytes of LDS for the tile's footprint in the intermediate image
constexpr int SRC_CAP = 16384;       // bytes of LDS for that footprint's footprint in the source
constexpr int MAX_SIDE = 128;        // longest side of the staged intermediate rectangle (the length of the coordinate tables)

#define HD __host__ __device__ __forceinline__

struct Warp { double i00, i01, i10, i11, b1, b2; };
struct Box { int x0, y0, x1, y1; };          // half open; empty when x1 <= x0 or y1 <= y0
struct Plan { Box mid, src; int id1, id2, path; };

HD int imin(int a, int b) { return a < b ? a : b; }
HD int imax(int a, int b) { return a > b ? a : b; }
HD long long lmin(long long a, long long b) { return a < b ? a : b; }
HD long long lmax(long long a, long long b) { return a > b ? a : b; }
HD bool empty(const Box &b) { return b.x1 <= b.x0 || b.y1 <= b.y0; }
HD long long area(const Box &b) { return empty(b) ? 0 : (long long)(b.x1 - b.x0) * (b.y1 - b.y0); }
HD Box clip(const Box &b, int h, int w) { return Box{imax(b.x0, 0), imax(b.y0, 0), imin(b.x1, w), imin(b.y1, h)}; }

// rint(v) as a 64-bit integer; values no coefficient set within the documented 2^30 pixel limit produces are cut to +-2^62 (a sum of
// two stays inside int64) and a NaN becomes -2^62: wrong pixels for such a record, never an undefined conversion
HD long long to_fixed(double v) {
    const double lim = 4611686018427387904.0;
    v = rint(v);
    v = v < lim ? v : lim;
    v = v > -lim ? v : -lim;
    return (long long)v;
}
// the column and the row term of the inverse map's two coordinates, in 1/1024 pixel (warp_affine_linear's adelta / bdelta, X0 / Y0)
HD long long col_x(const Warp &m, int x) { return to_fixed(m.i00 * (double)x * 1024.0); }
HD long long col_y(const Warp &m, int x) { return to_fixed(m.i10 * (double)x * 1024.0); }
HD long long row_x(const Warp &m, int y) { return to_fixed((m.i01 * (double)y + m.b1) * 1024.0) + 16; }
HD long long row_y(const Warp &m, int y) { return to_fixed((m.i11 * (double)y + m.b2) * 1024.0) + 16; }
// source pixel (clamped like OpenCV's short coordinates) and the 1/32 fraction of a 1/1024 coordinate
HD int whole(long long v) { return (int)lmin(lmax(v >> 10, -32768), 32767); }
HD int frac(long long v) { return (int)((v >> 5) & 31); }
HD int bilinear(int v00, int v01, int v10, int v11, int fx, int fy) {
    const int acc = v00 * ((32 - fy) * (32 - fx) * 32) + v01 * ((32 - fy) * fx * 32) + v10 * (fy * (32 - fx) * 32) + v11 * (fy * fx * 32);
    return (acc + (1 << 14)) >> 15;
}
HD bool is_identity(const Warp &m, int h, int w) {
    return m.i00 == 1.0 && m.i01 == 0.0 && m.i10 == 0.0 && m.i11 == 1.0 && m.b1 == 0.0 && m.b2 == 0.0 && h <= 32768 && w <= 32768;
}
HD Warp warp_of(const double *c) { return Warp{c[0], c[1], c[2], c[3], c[4], c[5]}; }

// The bounding box, inside the h x w image, of the source pixels the warp reads for the output pixels of r (not empty).  Exact: the
// column and the row terms are monotone, so the extremes of their sum over r are sums of their extremes at r's edges.
HD Box footprint(const Warp &m, const Box &r, int h, int w) {
    const long long cx0 = col_x(m, r.x0), cx1 = col_x(m, r.x1 - 1), rx0 = row_x(m, r.y0), rx1 = row_x(m, r.y1 - 1);
    const long long cy0 = col_y(m, r.x0), cy1 = col_y(m, r.x1 - 1), ry0 = row_y(m, r.y0), ry1 = row_y(m, r.y1 - 1);
    const Box b{whole(lmin(cx0, cx1) + lmin(rx0, rx1)), whole(lmin(cy0, cy1) + lmin(ry0, ry1)),
                whole(lmax(cx0, cx1) + lmax(rx0, rx1)) + 2, whole(lmax(cy0, cy1) + lmax(ry0, ry1)) + 2};
    return clip(b, h, w);
}

// What the workgroup of the output tile at (tx0, ty0) does.  path 0: the tile is zero (nothing of the image under it); 1: staged in
// LDS; 2: direct from global memory.
HD Plan plan_tile(const double *coef, const int *shift, int h, int w, int tx0, int ty0) {
    Plan p;
    const Warp w1 = warp_of(coef), w2 = warp_of(coef + 6);
    p.id1 = is_identity(w1, h, w);
    p.id2 = is_identity(w2, h, w);
    const Box tile = clip(Box{tx0, ty0, tx0 + TW, ty0 + TH}, h, w);
    const Box c = p.id2 ? tile : footprint(w2, tile, h, w);                      // in the shifted image crop(W1(src))
    p.mid = Box{0, 0, 0, 0};
    p.src = Box{0, 0, 0, 0};
    p.path = 0;
    if (empty(c)) return p;
    // crop(I)[r, c] = I[r + shift[0], c + shift[1]]  (long long: any shift)
    const long long sr = shift[0], sc = shift[1];
    p.mid = Box{(int)lmin(lmax(c.x0 + sc, 0), w), (int)lmin(lmax(c.y0 + sr, 0), h), (int)lmin(lmax(c.x1 + sc, 0), w), (int)lmin(lmax(c.y1 + sr, 0), h)};
    if (empty(p.mid)) return p;
    p.src = p.id1 ? p.mid : footprint(w1, p.mid, h, w);
    if (empty(p.src)) return p;
    const bool fits = p.mid.x1 - p.mid.x0 <= MAX_SIDE && p.mid.y1 - p.mid.y0 <= MAX_SIDE && area(p.mid) <= MID_CAP && (p.id1 || area(p.src) <= SRC_CAP);
    p.path = fits ? 1 : 2;
    return p;
}

// W1(src) at intermediate pixel (x, y) straight from global memory (the direct path)
__device__ __forceinline__ int mid_direct(const unsigned char *__restrict__ src, const Warp &m, int x, int y, int h, int w) {
    if (x < 0 || x >= w || y < 0 || y >= h) return 0;
    const long long X = col_x(m, x) + row_x(m, y), Y = col_y(m, x) + row_y(m, y);
    const int sx = whole(X), sy = whole(Y);
    auto tap = [&](int yy, int xx) { return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? (int)src[(size_t)yy * w + xx] : 0; };
    return bilinear(tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1), frac(X), frac(Y));
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ Box uniform(const Box &b) { return Box{uniform(b.x0), uniform(b.y0), uniform(b.x1), uniform(b.y1)}; }

__global__ __launch_bounds__(THREADS) void k_bev_stack(const unsigned char *__restrict__ planes, const double *__restrict__ coefs,
                                                       const int *__restrict__ shifts, unsigned char *__restrict__ out, int h, int w, int threshold) {
    __shared__ unsigned char s_src[SRC_CAP];
    __shared__ unsigned char s_mid[MID_CAP];
    __shared__ long long s_col[2][MAX_SIDE], s_row[2][MAX_SIDE];
    const int plane = blockIdx.z, tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, tid = threadIdx.x;
    const double *coef = coefs + (size_t)plane * 12;
    const int *shift = shifts + (size_t)plane * 2;
    const unsigned char *src = planes + (size_t)plane * h * w;
    unsigned char *dst = out + (size_t)plane * h * w;
    const Plan P = plan_tile(coef, shift, h, w, tx0, ty0);         // the same in every lane
    const Box M = uniform(P.mid), S = uniform(P.src), T = clip(Box{tx0, ty0, tx0 + TW, ty0 + TH}, h, w);
    const int path = uniform(P.path), id1 = uniform(P.id1), id2 = uniform(P.id2);
    const int sr = shift[0], sc = shift[1];
    const int tw = T.x1 - T.x0, th = T.y1 - T.y0, mw = M.x1 - M.x0, mh = M.y1 - M.y0, sw = S.x1 - S.x0;
    const Warp w1 = warp_of(coef), w2 = warp_of(coef + 6);
    // four consecutive pixels of a row per thread: one dword store where the row allows it
    const bool wide = (w & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    const int quads = (tw + 3) >> 2;
    auto store4 = [&](int y, int x, const int (&v)[4]) {
        unsigned char *p = dst + (size_t)y * w + x;
        if (wide && x + 4 <= T.x1) {
            *reinterpret_cast<unsigned *>(p) = (unsigned)v[0] | (unsigned)v[1] << 8 | (unsigned)v[2] << 16 | (unsigned)v[3] << 24;
        } else {
            for (int k = 0; k < 4 && x + k < T.x1; ++k) p[k] = (unsigned char)v[k];
        }
    };
    auto final_value = [&](int v) { return threshold ? (v > 0 ? 1 : 0) : v; };
    // the coordinate tables of a rectangle's nx columns and ny rows (at most MAX_SIDE each): threads 0 .. take the columns, threads
    // MAX_SIDE .. the rows.  (The fence keeps the two 64-bit stores from being merged into one ds_write2_b64: common.hpp.)
    auto fill_tables = [&](const Warp &m, int x0, int nx, int y0, int ny) {
        if (tid < nx) {
            s_col[0][tid] = col_x(m, x0 + tid);
            lds_store_fence();
            s_col[1][tid] = col_y(m, x0 + tid);
        }
        const int r = tid - MAX_SIDE;
        if (r >= 0 && r < ny) {
            s_row[0][r] = row_x(m, y0 + r);
            lds_store_fence();
            s_row[1][r] = row_y(m, y0 + r);
        }
    };

    if (path == 0) {
        const int zero[4] = {0, 0, 0, 0};
        for (int i = tid; i < quads * th; i += THREADS) store4(T.y0 + i / quads, T.x0 + 4 * (i % quads), zero);
        return;
    }

    if (path == 2) {   // direct: W2's four taps, each an intermediate pixel interpolated from the source in global memory
        for (int i = tid; i < quads * th; i += THREADS) {
            const int y = T.y0 + i / quads, xq = T.x0 + 4 * (i % quads);
            int v[4] = {0, 0, 0, 0};
            for (int k = 0; k < 4 && xq + k < T.x1; ++k) {
                const int x = xq + k;
                const long long X = col_x(w2, x) + row_x(w2, y), Y = col_y(w2, x) + row_y(w2, y);
                const int sx = whole(X), sy = whole(Y);
                auto tap = [&](int r, int c) {        // crop(W1(src))[r, c]
                    if (r < 0 || r >= h || c < 0 || c >= w) return 0;
                    const long long rr = (long long)r + sr, cc = (long long)c + sc;
                    if (rr < 0 || rr >= h || cc < 0 || cc >= w) return 0;
                    return mid_direct(src, w1, (int)cc, (int)rr, h, w);
                };
                v[k] = final_value(bilinear(tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1), frac(X), frac(Y)));
            }
            store4(y, xq, v);
        }
        return;
    }

    // ---- staged path.  s_mid[(y - M.y0) * mw + (x - M.x0)] = W1(src)[y, x] over M
    if (id1) {
        for (int i = tid; i < mw * mh; i += THREADS) s_mid[i] = src[(size_t)(M.y0 + i / mw) * w + M.x0 + i % mw];
    } else {
        const int scount = sw * (S.y1 - S.y0);
        for (int i = tid; i < scount; i += THREADS) s_src[i] = src[(size_t)(S.y0 + i / sw) * w + S.x0 + i % sw];
        fill_tables(w1, M.x0, mw, M.y0, mh);
        __syncthreads();
        // a tap inside the image is inside S (footprint() is exact); the test against S keeps a wrong table from reading other LDS
        auto tap = [&](int yy, int xx) { return (yy >= S.y0 && yy < S.y1 && xx >= S.x0 && xx < S.x1) ? (int)s_src[(yy - S.y0) * sw + (xx - S.x0)] : 0; };
        for (int i = tid; i < mw * mh; i += THREADS) {
            const int my = i / mw, mx = i % mw;
            const long long X = s_col[0][mx] + s_row[0][my], Y = s_col[1][mx] + s_row[1][my];
            const int sx = whole(X), sy = whole(Y);
            s_mid[i] = (unsigned char)bilinear(tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1), frac(X), frac(Y));
        }
    }
    __syncthreads();
    // crop(W1(src))[r, c]: zero outside the image, before and after the shift; what is inside lies in M
    auto cropped = [&](int r, int c) {
        if (r < 0 || r >= h || c < 0 || c >= w) return 0;
        const long long rr = (long long)r + sr - M.y0, cc = (long long)c + sc - M.x0;
        return (rr >= 0 && rr < mh && cc >= 0 && cc < mw) ? (int)s_mid[(int)rr * mw + (int)cc] : 0;
    };
    if (id2) {
        for (int i = tid; i < quads * th; i += THREADS) {
            const int y = T.y0 + i / quads, xq = T.x0 + 4 * (i % quads);
            int v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = final_value(cropped(y, xq + k));
            store4(y, xq, v);
        }
        return;
    }
    fill_tables(w2, T.x0, tw, T.y0, th);
    __syncthreads();
    for (int i = tid; i < quads * th; i += THREADS) {
        const int ty = i / quads, tq = 4 * (i % quads);
        int v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (tq + k < tw) {
                const long long X = s_col[0][tq + k] + s_row[0][ty], Y = s_col[1][tq + k] + s_row[1][ty];
                const int sx = whole(X), sy = whole(Y);
                v[k] = final_value(bilinear(cropped(sy, sx), cropped(sy, sx + 1), cropped(sy + 1, sx), cropped(sy + 1, sx + 1), frac(X), frac(Y)));
            }
        }
        store4(T.y0 + ty, T.x0 + tq, v);
    }
}
}  // namespace

extern "C" int lav_bev_stack_tile_paths(const double *coef, const int *shift, int h, int w, int *counts) {
    LAV_REQUIRE(coef && shift && counts && h >= 1 && w >= 1, "lav_bev_stack_tile_paths: bad argument");
    counts[0] = counts[1] = counts[2] = 0;
    for (int ty0 = 0; ty0 < h; ty0 += TH)
        for (int tx0 = 0; tx0 < w; tx0 += TW) ++counts[plan_tile(coef, shift, h, w, tx0, ty0).path];
    return LAV_OK;
}

extern "C" int lav_bev_stack_u8(const unsigned char *planes, const double *coef, const int *shift, unsigned char *out, int n, int h, int w,
                                int threshold, void *stream) {
    static_assert(TW <= MAX_SIDE && TH <= MAX_SIDE && THREADS >= 2 * MAX_SIDE, "the coordinate tables are filled by one thread per entry");
    LAV_REQUIRE(n >= 0 && h >= 1 && w >= 1 && ((planes && coef && shift && out) || n == 0), "lav_bev_stack_u8: bad argument");
    if (n == 0) return LAV_OK;
    LAV_REQUIRE(n <= 65535, "lav_bev_stack_u8: %d planes in one launch (at most 65535)", n);
    const size_t bytes = (size_t)h * w * n;
    LAV_REQUIRE(planes + bytes <= out || out + bytes <= planes, "lav_bev_stack_u8: planes and out overlap (footprints are read from planes)");
    LAV_REQUIRE((h + TH - 1) / TH <= 65535 && (long)w + TW < (long)INT32_MAX && (long)h + TH < (long)INT32_MAX, "lav_bev_stack_u8: image %d x %d too large", h, w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((w + TW - 1) / TW, (h + TH - 1) / TH, n);
    const int tok = timer_begin("bev_stack_u8", st);
    hipLaunchKernelGGL(k_bev_stack, grid, dim3(THREADS), 0, st, planes, coef, shift, out, h, w, threshold);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
