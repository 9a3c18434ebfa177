// Held-out metrics of the two camera checkpoints (eval_seg.py, eval_bra_v2.py; lav_amd.train.evaluate_camera): lav_eval_seg counts the
// confusion matrix of a batch of label maps against logits that stay where the network wrote them, lav_eval_scores the brake net's
// scores against the recorded flags.  Both ADD integers into a caller-owned section of an int64 accumulator in HBM; nothing returns to
// the host.  The specifications are eval_seg_numpy / eval_scores_numpy and the kernels equal them in every word
// (tests/test_gpu_eval_camera.py): every term is an integer, so no result depends on the order in which workgroups arrive.  The
// reference has no evaluator: the definitions are this project's, parity with a reference is UNPINNED.
//
// lav_eval_seg.  Label pixel (y, x) is judged by logit pixel (y / scale, x / scale): nearest up-sampling followed by argmax, without
// the up-sampled logits.  A lane takes four consecutive logit pixels of one image (16-byte loads per channel where the plane's address
// allows them, scalar loads elsewhere), keeps the running maximum in registers and reads the scale x 4 scale label bytes under them
// with the widest aligned loads there are (16 bytes per label row at scale 4; `scale` bytes per pixel and row where the row's run is not
// aligned or the four do not share a row; single bytes only under a label pointer that is itself not aligned to scale).
//
// Counting: per-wave LDS counters, not wave ballots.  A ballot counts one cell for 64 lanes; here a pixel slot can hit any of k * k
// cells (up to 64 ballots + population counts per slot, 100 at the agent's k = 5 for a lane's four pixels), and at scale > 1 one logit
// pixel owns scale^2 label pixels of several classes, which a ballot cannot express at all.  So a lane first tallies the labels under
// one logit pixel in registers - eight 8-bit fields of one 64-bit word, at most 64 each -, then adds every non-zero field with one LDS
// atomic to its wave's conf[label][prediction]: k adds at the most per logit pixel, usually one or two (label maps are blocky),
// whatever k is.  Behind a barrier 68 lanes sum the four waves and issue one 64-bit vector atomic per non-zero counter (Guideline 12).
// A workgroup's 32-bit partial counts cannot overflow: n h w scale^2 <= 2^31 is required, and no counter exceeds the pixels seen.
#include "common.hpp"

namespace {
using namespace lav;
constexpr int THREADS = 256, WAVES = THREADS / WAVE;
constexpr int MAX_K = 8, SEG_WORDS = 4 + MAX_K * MAX_K, MAX_GROUPS = 128, MAX_BINS = 1024, SCORE_HEAD = 6;
constexpr unsigned long long MAX_PIXELS = 1ull << 31;
// the sections' words; lav_amd.train.evaluate_camera.CameraLayout names the same slices
enum { S_IMAGES = 0, S_PIXELS = 1, S_IGNORED = 2, S_NONFINITE = 3, S_CONF = 4 };
enum { B_SAMPLES = 0, B_NONFINITE = 1, B_AT = 2, B_HIST = 6 };

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= 3.4028235e38f; }      // (false for a NaN)

// P label bytes (1, 2, 4 or 8) from p, aligned to P, into bytes [at, at + P) of w; `at` is a multiple of P
template <int P, int WORDS>
__device__ __forceinline__ void load_piece(const unsigned char *p, unsigned (&w)[WORDS], int at) {
    if constexpr (P == 8) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        w[at / 4] = v.x; w[at / 4 + 1] = v.y;
    } else if constexpr (P == 4) {
        w[at / 4] = *reinterpret_cast<const unsigned *>(p);
    } else if constexpr (P == 2) {
        w[at / 4] |= (unsigned)*reinterpret_cast<const unsigned short *>(p) << (8 * (at % 4));
    } else {
        w[at / 4] |= (unsigned)p[0] << (8 * (at % 4));
    }
}

// N label bytes from p into 32-bit words, first byte lowest, with the widest aligned loads there are: one load (two of 16 bytes at
// N = 32) where p is aligned to min(N, 16); else N / P loads of P bytes where p is aligned to P (a pixel's `scale` bytes: a label row
// whose width is no multiple of 4 starts anywhere, but every pixel's run in it starts on a multiple of scale); else byte loads
template <int N, int P>
__device__ __forceinline__ void load_run(const unsigned char *p, unsigned (&w)[(N + 3) / 4]) {
    constexpr int A = N < 16 ? N : 16;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    if constexpr (N >= 16) {
        if ((addr & 15) == 0) {
#pragma unroll
            for (int u = 0; u < N / 16; ++u) {
                const uint4 v = reinterpret_cast<const uint4 *>(p)[u];
                w[4 * u] = v.x; w[4 * u + 1] = v.y; w[4 * u + 2] = v.z; w[4 * u + 3] = v.w;
            }
            return;
        }
    }
#pragma unroll
    for (int u = 0; u < (N + 3) / 4; ++u) w[u] = 0;
    if constexpr (N < 16) {
        if ((addr & (A - 1)) == 0) {
            load_piece<N>(p, w, 0);
            return;
        }
    }
    if constexpr (P > 1 && P < N) {
        if ((addr & (P - 1)) == 0) {
#pragma unroll
            for (int b = 0; b < N; b += P) load_piece<P>(p + b, w, b);
            return;
        }
    }
#pragma unroll
    for (int b = 0; b < N; ++b) load_piece<1>(p + b, w, b);
}

// bytes [first, first + S) of w: a label below k adds 1 to its 8-bit field of `tally`, any other to `ignored`
template <int S, int WORDS>
__device__ __forceinline__ void tally_run(const unsigned (&w)[WORDS], int first, int k, unsigned long long &tally, unsigned &ignored) {
#pragma unroll
    for (int t = 0; t < S; ++t) {
        const int b = first + t;
        const unsigned l = (w[b / 4] >> (8 * (b % 4))) & 0xffu;
        if (l < (unsigned)k) tally += 1ull << (8 * l);
        else ignored += 1;
    }
}

struct SegArgs {
    const float *logits;
    const unsigned char *labels;
    int n, k, h, w;
    unsigned long long *acc;
};

template <int S>
__global__ __launch_bounds__(THREADS) void k_eval_seg(SegArgs a) {
    __shared__ unsigned s_cnt[WAVES][SEG_WORDS];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < WAVES * SEG_WORDS; i += THREADS) (&s_cnt[0][0])[i] = 0;
    __syncthreads();
    unsigned *cnt = s_cnt[wave];
    const size_t plane = (size_t)a.h * a.w, per_image = (plane + 3) / 4, quads = per_image * a.n;
    const size_t LW = (size_t)a.w * S, label_plane = plane * S * S;
    unsigned ignored = 0, nonfinite = 0;
    for (size_t q0 = (size_t)blockIdx.x * THREADS; q0 < quads; q0 += (size_t)gridDim.x * THREADS) {     // (uniform)
        const size_t q = q0 + tid;
        if (q >= quads) continue;
        const size_t img = q / per_image, i = 4 * (q - img * per_image);
        const int cnt_px = plane - i < 4 ? (int)(plane - i) : 4;
        const int y0 = (int)(i / a.w), x0 = (int)(i - (size_t)y0 * a.w);

        // the first maximum of the k channels, per pixel; `bad`: a channel that is not finite
        float v[MAX_K][4];
        const float *lp = a.logits + img * a.k * plane + i;
#pragma unroll
        for (int c = 0; c < MAX_K; ++c) {
            if (c < a.k) {
                const float *p = lp + (size_t)c * plane;
                if (cnt_px == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {      // (per channel: a plane of h w floats starts anywhere)
                    const float4 f = *reinterpret_cast<const float4 *>(p);
                    v[c][0] = f.x; v[c][1] = f.y; v[c][2] = f.z; v[c][3] = f.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[c][j] = j < cnt_px ? p[j] : 0.f;
                }
            }
        }
        float best[4];
        int pred[4];
        bool bad[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { best[j] = v[0][j]; pred[j] = 0; bad[j] = !finite(v[0][j]); }
#pragma unroll
        for (int c = 1; c < MAX_K; ++c) {
            if (c < a.k) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (v[c][j] > best[j]) { best[j] = v[c][j]; pred[j] = c; }
                    bad[j] = bad[j] || !finite(v[c][j]);
                }
            }
        }

        // the labels under the four pixels
        unsigned long long tally[4] = {0, 0, 0, 0};
        unsigned ign[4] = {0, 0, 0, 0};
        const unsigned char *lab = a.labels + img * label_plane;
        if (cnt_px == 4 && x0 + 3 < a.w) {                 // one row of logit pixels: 4 S label bytes per label row
            const unsigned char *row = lab + (size_t)y0 * S * LW + (size_t)x0 * S;
#pragma unroll
            for (int r = 0; r < S; ++r) {
                unsigned wd[S];
                load_run<4 * S, S>(row + (size_t)r * LW, wd);
#pragma unroll
                for (int j = 0; j < 4; ++j) tally_run<S>(wd, j * S, a.k, tally[j], ign[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < cnt_px) {
                    const size_t y = (i + j) / a.w, x = (i + j) - y * a.w;
                    const unsigned char *row = lab + y * S * LW + x * S;
#pragma unroll
                    for (int r = 0; r < S; ++r) {
                        unsigned wd[(S + 3) / 4];
                        load_run<S, S>(row + (size_t)r * LW, wd);
                        tally_run<S>(wd, 0, a.k, tally[j], ign[j]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= cnt_px) continue;
            if (bad[j]) { nonfinite += S * S; continue; }
            ignored += ign[j];
            for (int l = 0; l < a.k; ++l) {
                const unsigned c = (unsigned)(tally[j] >> (8 * l)) & 0xffu;
                if (c != 0) atomicAdd(cnt + S_CONF + MAX_K * l + pred[j], c);
            }
        }
    }
    if (ignored != 0) atomicAdd(cnt + S_IGNORED, ignored);
    if (nonfinite != 0) atomicAdd(cnt + S_NONFINITE, nonfinite);
    __syncthreads();
    if (tid < SEG_WORDS) {
        unsigned long long s = 0;
#pragma unroll
        for (int v2 = 0; v2 < WAVES; ++v2) s += s_cnt[v2][tid];
        if (blockIdx.x == 0 && tid == S_IMAGES) s = (unsigned long long)a.n;
        if (blockIdx.x == 0 && tid == S_PIXELS) s = (unsigned long long)a.n * label_plane;
        if (s != 0) atomicAdd(a.acc + tid, s);
    }
}

__global__ __launch_bounds__(THREADS) void k_eval_scores(const float *scores, const unsigned char *flags, int n, double threshold, int nbins,
                                                         unsigned long long *acc) {
    __shared__ unsigned s_cnt[SCORE_HEAD + 2 * MAX_BINS];
    const int tid = threadIdx.x, words = SCORE_HEAD + 2 * nbins;
    for (int i = tid; i < words; i += THREADS) s_cnt[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += THREADS) {
        const float s = scores[i];
        const int flag = flags[i] != 0 ? 1 : 0;
        if (!finite(s)) { atomicAdd(s_cnt + B_NONFINITE, 1u); continue; }
        atomicAdd(s_cnt + B_AT + 2 * flag + ((double)s > threshold ? 1 : 0), 1u);
        const float scaled = s * (float)nbins;             // lav_eval_frame's bin, with the scores below 0 in bin 0
        const int bin = scaled >= (float)(nbins - 1) ? nbins - 1 : (scaled < 0.f ? 0 : (int)scaled);
        atomicAdd(s_cnt + B_HIST + flag * nbins + bin, 1u);
    }
    __syncthreads();
    for (int i = tid; i < words; i += THREADS) {
        const unsigned long long s = i == B_SAMPLES ? (unsigned long long)n : s_cnt[i];
        if (s != 0) atomicAdd(acc + i, s);
    }
}
static_assert(S_CONF + MAX_K * MAX_K == SEG_WORDS && B_HIST == SCORE_HEAD && B_AT + 4 == B_HIST, "the sections' layouts");
}  // namespace

extern "C" int lav_eval_seg(const float *logits, const unsigned char *labels, int n, int k, int h, int w, int scale, unsigned long long *acc,
                            void *stream) {
    LAV_REQUIRE(logits && labels && acc, "lav_eval_seg: null argument");
    LAV_REQUIRE(k >= 2 && k <= MAX_K, "lav_eval_seg: %d classes (2 .. %d)", k, MAX_K);
    LAV_REQUIRE(scale == 1 || scale == 2 || scale == 4 || scale == 8, "lav_eval_seg: scale %d (1, 2, 4 or 8)", scale);
    LAV_REQUIRE(n >= 1 && h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "lav_eval_seg: %d maps of %d x %d", n, h, w);
    LAV_REQUIRE((unsigned long long)n * h * w * scale * scale <= MAX_PIXELS, "lav_eval_seg: %d x %d x %d logit pixels at scale %d are more than 2^31 label pixels",
                n, h, w, scale);
    LAV_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 3) == 0 && (reinterpret_cast<uintptr_t>(acc) & 7) == 0,
                "lav_eval_seg: the logits must be 4-byte, the accumulator 8-byte aligned");
    SegArgs a;
    a.logits = logits; a.labels = labels; a.n = n; a.k = k; a.h = h; a.w = w; a.acc = acc;
    const size_t quads = (((size_t)h * w + 3) / 4) * n;
    const int groups = (int)std::min<size_t>((quads + THREADS - 1) / THREADS, MAX_GROUPS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("eval_seg", st);
    if (scale == 1) hipLaunchKernelGGL(k_eval_seg<1>, dim3(groups), dim3(THREADS), 0, st, a);
    else if (scale == 2) hipLaunchKernelGGL(k_eval_seg<2>, dim3(groups), dim3(THREADS), 0, st, a);
    else if (scale == 4) hipLaunchKernelGGL(k_eval_seg<4>, dim3(groups), dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL(k_eval_seg<8>, dim3(groups), dim3(THREADS), 0, st, a);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}

extern "C" int lav_eval_scores(const float *scores, const unsigned char *flags, int n, double threshold, int nbins, unsigned long long *acc,
                               void *stream) {
    LAV_REQUIRE(scores && flags && acc, "lav_eval_scores: null argument");
    LAV_REQUIRE(n >= 1, "lav_eval_scores: %d scores", n);
    LAV_REQUIRE(nbins >= 1 && nbins <= MAX_BINS, "lav_eval_scores: %d score bins (1 .. %d)", nbins, MAX_BINS);
    LAV_REQUIRE(threshold == threshold, "lav_eval_scores: the threshold must be a number");
    LAV_REQUIRE((reinterpret_cast<uintptr_t>(scores) & 3) == 0 && (reinterpret_cast<uintptr_t>(acc) & 7) == 0,
                "lav_eval_scores: the scores must be 4-byte, the accumulator 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("eval_scores", st);
    hipLaunchKernelGGL(k_eval_scores, dim3(1), dim3(THREADS), 0, st, scores, flags, n, threshold, nbins, acc);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
