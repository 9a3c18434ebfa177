// Block-bootstrap replicates of an evaluation's row table (the eval tools' --bootstrap; lav_amd.train.eval_common.EvaluatorBase.resample):
// rows [R][W] int64, one row of counters per block of consecutive frames, summed R rows at a time with replacement, B times.
//     out[0][w] = sum_r rows[r][w]                          (the identity replicate: the run's own accumulator)
//     out[b][w] = sum_{j < R} rows[idx(b, j)][w]            b = 1 .. B
//     idx(b, j) = (u * R) >> 32, u = word j & 3 of Philox4x32-10 at counter (j >> 2, b, 0x52534D50, 0), key (seed low, seed high)
// Specification: lav_amd.train.eval_common.eval_resample_numpy, equal in every word - the sums are integer sums modulo 2^64, so the
// order in which a workgroup's lanes take the draws does not show.
//
// A workgroup owns one replicate and one tile of `cols` columns (a power of two, at most 64: 512 contiguous bytes per wave load).  It
// draws the replicate's indices CHUNK at a time into LDS - one Philox call gives four of them, the calls are spread over the lanes -
// and walks them with its lanes along w; where the tile is narrower than the workgroup the lanes beyond it take every (256 / cols)-th
// draw and the partial sums meet in LDS.  Column tiles of one replicate repeat its draws: R / 4 Philox calls against R * cols loads.
// Workgroups of the same tile are neighbours in the grid (the replicate is the fast index), so that the R * cols * 8 bytes they all
// re-read are what their XCD's L2 holds at that time.  No atomics, no floating point, no dependency between workgroups.
#include "common.hpp"
#include "philox.hpp"

namespace {
using namespace lav;
constexpr int THREADS = 256, CHUNK = 4096, MAX_COLS = 64, MAX_ROWS = 1 << 20;
constexpr unsigned TAG = 0x52534D50u;          // "RSMP": the draws' own stream of the generator
typedef unsigned long long u64;                // sums wrap modulo 2^64, as NumPy's int64 sums do

__global__ __launch_bounds__(THREADS) void k_eval_resample(const u64 *__restrict__ rows, int R, int W, int reps, int cols_log2, unsigned k0,
                                                           unsigned k1, u64 *__restrict__ out) {
    __shared__ unsigned s_idx[CHUNK];
    __shared__ u64 s_part[THREADS];
    const int t = threadIdx.x, cols = 1 << cols_log2, slices = THREADS >> cols_log2;
    const unsigned b = blockIdx.x % (unsigned)reps;
    const int col = (int)(blockIdx.x / (unsigned)reps) * cols + (t & (cols - 1)), slice = t >> cols_log2;
    const bool live = col < W;
    const u64 *src = rows + (live ? col : 0);
    u64 sum = 0;
    for (int j0 = 0; j0 < R; j0 += CHUNK) {
        const int n = min(CHUNK, R - j0);
        if (b == 0) {
            for (int i = t; i < n; i += THREADS) s_idx[i] = (unsigned)(j0 + i);
        } else {
            for (int q = t; 4 * q < n; q += THREADS) {          // (4 q + 3 < CHUNK: the draws past R are stored and never read)
                unsigned u[4];
                philox4x32((unsigned)(j0 >> 2) + (unsigned)q, b, TAG, 0u, k0, k1, u);
#pragma unroll
                for (int k = 0; k < 4; ++k) s_idx[4 * q + k] = __umulhi(u[k], (unsigned)R);      // < R
            }
        }
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (int j = slice; j < n; j += slices) sum += src[(size_t)s_idx[j] * (size_t)W];
        }
        __syncthreads();
    }
    s_part[t] = sum;
    __syncthreads();
    for (int stride = THREADS / 2; stride >= cols; stride >>= 1) {      // lanes t and t + stride hold the same column
        if (t < stride) s_part[t] += s_part[t + stride];
        __syncthreads();
    }
    if (t < cols && live) out[(size_t)b * (size_t)W + col] = s_part[t];
}
}  // namespace

extern "C" int lav_eval_resample_chunk(void) { return CHUNK; }

extern "C" int lav_eval_resample(const long long *rows, int R, int W, int B, unsigned long long seed, long long *out, void *stream) {
    LAV_REQUIRE(rows && out, "lav_eval_resample: null argument");
    LAV_REQUIRE(R >= 1 && R <= MAX_ROWS, "lav_eval_resample: %d rows (1 .. %d: the index rule's bias is R / 2^32)", R, MAX_ROWS);
    LAV_REQUIRE(W >= 1 && B >= 0, "lav_eval_resample: %d words, %d replicates", W, B);
    LAV_REQUIRE((unsigned long long)R * (unsigned long long)W * 8ull <= (4ull << 30), "lav_eval_resample: a table of %d x %d words is more than 4 GiB", R, W);
    LAV_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0, "lav_eval_resample: rows and out must be 8-byte aligned");
    const long long *rows_end = rows + (size_t)R * W, *out_end = out + ((size_t)B + 1) * W;
    LAV_REQUIRE(rows_end <= out || out_end <= rows, "lav_eval_resample: rows and out overlap");
    int cols_log2 = 0;
    while ((1 << cols_log2) < W && (1 << cols_log2) < MAX_COLS) ++cols_log2;
    const long long tiles = ((long long)W + (1 << cols_log2) - 1) >> cols_log2, groups = tiles * ((long long)B + 1);
    LAV_REQUIRE(groups <= (long long)INT32_MAX, "lav_eval_resample: %d replicates of %lld column tiles are more than 2^31 - 1 workgroups", B, tiles);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("eval_resample", st);
    hipLaunchKernelGGL(k_eval_resample, dim3((unsigned)groups), dim3(THREADS), 0, st, reinterpret_cast<const u64 *>(rows), R, W, B + 1, cols_log2,
                       (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), reinterpret_cast<u64 *>(out));
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
