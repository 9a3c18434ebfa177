// Open-loop metrics of one evaluated frame (lav_eval_frame), added into one int64 accumulator that stays in HBM for a whole route.
// The specification is lav_amd.train.evaluate.eval_frame_numpy and the two agree in every bit (tests/test_gpu_eval.py): every counter
// is an integer, the distance sums are sums of distances quantised to 2^-20 m BEFORE they are added, so a route's result depends
// neither on the order of its frames nor on the order in which workgroups arrive.  There is no reference evaluator: the metric
// definitions are this project's, parity against the reference is UNPINNED because there is nothing to pin it to.
//
// One launch.  Workgroups 0 .. grid - 2 count the BEV segmentation (the only part with traffic: 3 float planes, 3 label planes and a
// mask): four pixels per lane, 16-byte loads of the predictions where the plane's address allows them and scalar loads elsewhere
// (a plane of H x W floats starts 16-byte aligned only when H W is a multiple of 4), one ballot + population count per pixel slot and
// counter.  The last workgroup does what is serial: wave c matches the rows of class c to the ground truth (one actor per lane, the
// nearest free one by a wave minimum, ties to the lowest index), then - behind a barrier - the four waves share the others' forecasts
// and wave 0 takes the ego plan.  Every workgroup ends with one 64-bit vector atomic per counter it has something to add to.
//
// Floating point: float64 from the float32 inputs, contraction off (lav_amd/build.py), so that (double)loc * ppm + centre,
// dx * dx + dy * dy and sqrt(.) * 2^20 round as NumPy rounds them; llrint rounds to nearest even like np.rint.
#include "eval_quantum.hpp"      // quantum(), wave_sum(), first_max(): shared with eval_plans.hip

#pragma clang fp contract(off)

namespace {
using namespace lav;
constexpr int THREADS = 256, WAVES = THREADS / WAVE;
constexpr int MAX_DET = 32, MAX_OBJS = 64, MAX_PLAN = 64, MAX_BINS = 1024, MAX_SEG_GROUPS = 256;
constexpr int CMDS = EVAL_CMDS;
// the accumulator's words; lav_amd.train.evaluate.ACC names the same slices (tests/test_eval_host.py compares the lengths)
enum { A_FRAMES = 0, A_SEG = 1, A_NGT = 10, A_DET = 12, A_PLAN = 16, A_PLAN_NONFINITE = 34, A_OTH_MATCHED = 35, A_OTH_UNMATCHED = 36,
       A_OTH_NONFINITE = 37, A_OTH_MIN = 38, A_OTH_TOP = 39, A_OTH_TOP_FINAL = 40, A_HIST = 41 };

struct Args {
    const float *pred;
    const unsigned char *labels, *mask;
    int h, w;
    float threshold;
    const float *rows;
    int max_det;
    const float *locs;
    const int *typs;
    int max_objs, num_objs, num_plan;
    const float *ego_plan, *ego_locs;
    int cmd;
    const float *other_cast, *other_cmds;
    const int *other_row;
    int num_others;
    double ppm, cx, cy, radius, min_score, det_score;
    int nbins;
    unsigned long long *acc;
};

__device__ __forceinline__ unsigned count_of(bool b) { return (unsigned)__popcll(__ballot(b)); }

// a 64-bit LDS store that is never paired with its neighbour (no ds_write2_b64: common.hpp, lds_store_fence)
__device__ __forceinline__ void lds_put(long long *p, long long v) {
    *p = v;
    lds_store_fence();
}

__device__ void segmentation(const Args &a, int groups) {
    __shared__ unsigned s_seg[WAVES][9];
    const int tid = threadIdx.x;
    const size_t plane = (size_t)a.h * a.w, quads = (plane + 3) / 4;
    unsigned n[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // the same in every lane of a wave: sums of ballots
    for (size_t q0 = (size_t)blockIdx.x * THREADS; q0 < quads; q0 += (size_t)groups * THREADS) {   // (uniform: the ballots see whole waves)
        const size_t q = q0 + tid, i = 4 * q;
        const int cnt = q < quads ? (plane - i < 4 ? (int)(plane - i) : 4) : 0;
        unsigned m = 0;                                // bit k: pixel i + k counts
        if (cnt == 4 && (reinterpret_cast<uintptr_t>(a.mask + i) & 3) == 0) {
            const unsigned v = *reinterpret_cast<const unsigned *>(a.mask + i);
            m = (v & 0xffu ? 1u : 0u) | (v & 0xff00u ? 2u : 0u) | (v & 0xff0000u ? 4u : 0u) | (v & 0xff000000u ? 8u : 0u);
        } else {
            for (int k = 0; k < cnt; ++k) m |= (a.mask[i + k] != 0 ? 1u : 0u) << k;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *p = a.pred + (size_t)c * plane + i;
            const unsigned char *l = a.labels + (size_t)c * plane + i;
            unsigned pb = 0, lb = 0;
            if (cnt == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                const float4 v = *reinterpret_cast<const float4 *>(p);
                pb = (v.x > a.threshold ? 1u : 0u) | (v.y > a.threshold ? 2u : 0u) | (v.z > a.threshold ? 4u : 0u) | (v.w > a.threshold ? 8u : 0u);
            } else {
                for (int k = 0; k < cnt; ++k) pb |= (p[k] > a.threshold ? 1u : 0u) << k;
            }
            if (cnt == 4 && (reinterpret_cast<uintptr_t>(l) & 3) == 0) {
                const unsigned v = *reinterpret_cast<const unsigned *>(l);
                lb = (v & 0xffu ? 1u : 0u) | (v & 0xff00u ? 2u : 0u) | (v & 0xff0000u ? 4u : 0u) | (v & 0xff000000u ? 8u : 0u);
            } else {
                for (int k = 0; k < cnt; ++k) lb |= (l[k] != 0 ? 1u : 0u) << k;
            }
            const unsigned tp = pb & lb & m, fp = pb & ~lb & m, fn = ~pb & lb & m;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                n[3 * c] += count_of(tp >> k & 1);
                n[3 * c + 1] += count_of(fp >> k & 1);
                n[3 * c + 2] += count_of(fn >> k & 1);
            }
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s_seg[tid >> 6][k] = n[k];
    }
    __syncthreads();
    if (tid < 9) {
        unsigned long long s = 0;
        for (int v = 0; v < WAVES; ++v) s += s_seg[v][tid];
        if (s != 0) atomicAdd(a.acc + A_SEG + tid, s);
    }
}

__device__ void actors(const Args &a) {
    __shared__ int s_match[2][MAX_DET];                // per class and row: the ground-truth actor it took, or -1
    __shared__ int s_hist[4 * MAX_BINS];               // [class][true / false positive][bin]
    __shared__ long long s_cnt[A_HIST];                // the frame's share of the accumulator's head
    __shared__ long long s_oth[WAVES][6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.num_plan, D = a.max_det;
    for (int i = tid; i < 4 * a.nbins; i += THREADS) s_hist[i] = 0;
    for (int i = tid; i < A_HIST; i += THREADS) lds_put(s_cnt + i, 0);
    for (int i = tid; i < 2 * MAX_DET; i += THREADS) s_match[i / MAX_DET][i % MAX_DET] = -1;
    __syncthreads();

    if (wave < 2) {                                    // detection of class `wave`: lane g holds ground-truth actor g
        const int c = wave;
        bool valid = false, taken = false;
        double px = 0.0, py = 0.0;
        if (lane < a.num_objs && a.typs[lane] == c) {
            const float *loc = a.locs + (size_t)lane * (T + 1) * 2;
            px = (double)loc[0] * a.ppm + a.cx;
            py = (double)loc[1] * a.ppm + a.cy;
            valid = px >= 0.0 && px < (double)a.w && py >= 0.0 && py < (double)a.h;
        }
        const int n_gt = (int)count_of(valid);
        const double r2 = a.radius * a.radius;
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        int tp_det = 0, fp_det = 0;
        for (int r = 0; r < D; ++r) {                  // (uniform: every lane reads the same row)
            const float *row = a.rows + ((size_t)c * D + r) * 7;
            const float score = row[0];
            if (!((double)score > a.min_score)) continue;
            const double dx = (double)row[1] - px, dy = (double)row[2] - py;
            const double d2 = dx * dx + dy * dy;
            const bool cand = valid && !taken && d2 <= r2;
            double best = cand ? d2 : inf;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const double other = __shfl_xor(best, o, 64);
                best = other < best ? other : best;
            }
            const unsigned long long winners = __ballot(cand && d2 == best);
            const int g = winners ? __ffsll((long long)winners) - 1 : -1;       // the lowest index among the nearest
            if (lane == g) taken = true;
            const float scaled = score * (float)a.nbins;
            const int bin = scaled >= (float)(a.nbins - 1) ? a.nbins - 1 : (int)scaled;
            if (lane == 0) {
                s_match[c][r] = g;
                s_hist[(2 * c + (g < 0 ? 1 : 0)) * a.nbins + bin] += 1;
            }
            if ((double)score > a.det_score) {
                tp_det += g >= 0;
                fp_det += g < 0;
            }
        }
        if (lane == 0) {
            lds_put(s_cnt + A_NGT + c, n_gt);
            lds_put(s_cnt + A_DET + 2 * c, tp_det);
            lds_put(s_cnt + A_DET + 2 * c + 1, fp_det);
        }
    }
    __syncthreads();

    // the others' forecasts: forecast k came from row other_row[k] of class 1; lane t holds waypoint t
    long long o_matched = 0, o_unmatched = 0, o_nonfinite = 0, o_min = 0, o_top = 0, o_final = 0;
    for (int k = wave; k < a.num_others; k += WAVES) {
        const int r = a.other_row[k];
        const int g = r >= 0 && r < D ? s_match[1][r] : -1;
        if (g < 0) { o_unmatched += 1; continue; }
        const int top = first_max(a.other_cmds + (size_t)k * CMDS);
        long long s_min = 0, s_top = 0, q_top = 0;
        bool finite = true;
        for (int m = 0; m < CMDS; ++m) {
            long long q = 0;
            bool ok = true;
            if (lane < T) ok = quantum(a.other_cast + (((size_t)k * CMDS + m) * T + lane) * 2, a.locs + ((size_t)g * (T + 1) + lane + 1) * 2, q);
            finite = finite && __ballot(!ok) == 0;
            const long long s = wave_sum(q);
            s_min = m == 0 || s < s_min ? s : s_min;
            if (m == top) { s_top = s; q_top = __shfl(q, T - 1, 64); }
        }
        if (!finite) { o_nonfinite += 1; continue; }
        o_matched += 1; o_min += s_min; o_top += s_top; o_final += q_top;
    }
    if (lane == 0) {
        lds_put(&s_oth[wave][0], o_matched); lds_put(&s_oth[wave][1], o_unmatched); lds_put(&s_oth[wave][2], o_nonfinite);
        lds_put(&s_oth[wave][3], o_min); lds_put(&s_oth[wave][4], o_top); lds_put(&s_oth[wave][5], o_final);
    }
    if (wave == 0) {                                   // the ego plan against ego_locs[t + 1]
        long long q = 0;
        bool ok = true;
        if (lane < T) ok = quantum(a.ego_plan + (size_t)lane * 2, a.ego_locs + (size_t)(lane + 1) * 2, q);
        const bool finite = __ballot(!ok) == 0;
        const long long s = wave_sum(q), last = __shfl(q, T - 1, 64);
        if (lane == 0) {
            lds_put(s_cnt + A_FRAMES, 1);
            if (finite) {
                lds_put(s_cnt + A_PLAN + 3 * a.cmd, 1);
                lds_put(s_cnt + A_PLAN + 3 * a.cmd + 1, s);
                lds_put(s_cnt + A_PLAN + 3 * a.cmd + 2, last);
            } else {
                lds_put(s_cnt + A_PLAN_NONFINITE, 1);
            }
        }
    }
    __syncthreads();
    if (tid < 6) {
        long long s = 0;
        for (int v = 0; v < WAVES; ++v) s += s_oth[v][tid];
        lds_put(s_cnt + A_OTH_MATCHED + tid, s);
    }
    __syncthreads();
    for (int i = tid; i < A_HIST; i += THREADS)
        if (s_cnt[i] != 0) atomicAdd(a.acc + i, (unsigned long long)s_cnt[i]);
    for (int i = tid; i < 4 * a.nbins; i += THREADS)
        if (s_hist[i] != 0) atomicAdd(a.acc + A_HIST + i, (unsigned long long)s_hist[i]);
}

__global__ __launch_bounds__(THREADS) void k_eval_frame(Args a) {
    const int groups = (int)gridDim.x - 1;
    if ((int)blockIdx.x < groups) segmentation(a, groups);
    else actors(a);
}
static_assert(A_OTH_UNMATCHED == A_OTH_MATCHED + 1 && A_OTH_NONFINITE == A_OTH_MATCHED + 2 && A_OTH_MIN == A_OTH_MATCHED + 3 &&
              A_OTH_TOP == A_OTH_MATCHED + 4 && A_OTH_TOP_FINAL == A_OTH_MATCHED + 5 && A_HIST == A_OTH_TOP_FINAL + 1 &&
              A_PLAN_NONFINITE == A_PLAN + 3 * CMDS, "the others' counters follow each other, the histograms close the layout");
}  // namespace

extern "C" size_t lav_eval_acc_words(int nbins) { return nbins >= 1 && nbins <= MAX_BINS ? (size_t)A_HIST + 4 * (size_t)nbins : 0; }

extern "C" int lav_eval_frame(const float *pred_bev, const unsigned char *labels, const unsigned char *mask, int h, int w, float threshold,
                              const float *rows, int max_det, const float *locs, const int *typs, int max_objs, int num_objs, int num_plan,
                              const float *ego_plan, const float *ego_locs, int cmd, const float *other_cast, const float *other_cmds,
                              const int *other_row, int num_others, double ppm, double centre_x, double centre_y, double radius_px,
                              double min_score, double det_score, int nbins, long long *acc, void *stream) {
    LAV_REQUIRE(pred_bev && labels && mask && rows && ego_plan && ego_locs && acc, "lav_eval_frame: null argument");
    LAV_REQUIRE(h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "lav_eval_frame: map %d x %d", h, w);
    LAV_REQUIRE(max_det >= 1 && max_det <= MAX_DET, "lav_eval_frame: %d rows per class (1 .. %d)", max_det, MAX_DET);
    LAV_REQUIRE(max_objs >= 0 && max_objs <= MAX_OBJS && num_objs >= 0 && num_objs <= max_objs && ((locs && typs) || max_objs == 0),
                "lav_eval_frame: %d of %d ground-truth actors (at most %d)", num_objs, max_objs, MAX_OBJS);
    LAV_REQUIRE(num_plan >= 1 && num_plan <= MAX_PLAN, "lav_eval_frame: %d waypoints (1 .. %d)", num_plan, MAX_PLAN);
    LAV_REQUIRE(cmd >= 0 && cmd < CMDS, "lav_eval_frame: command %d (0 .. %d)", cmd, CMDS - 1);
    LAV_REQUIRE(num_others >= 0 && num_others <= max_det && ((other_cast && other_cmds && other_row) || num_others == 0),
                "lav_eval_frame: %d forecasts from %d rows", num_others, max_det);
    LAV_REQUIRE(num_others == 0 || max_objs > 0, "lav_eval_frame: forecasts without ground truth");
    LAV_REQUIRE(nbins >= 1 && nbins <= MAX_BINS, "lav_eval_frame: %d score bins (1 .. %d)", nbins, MAX_BINS);
    LAV_REQUIRE(ppm > 0.0 && radius_px >= 0.0 && centre_x == centre_x && centre_y == centre_y && min_score == min_score && det_score == det_score &&
                threshold == threshold, "lav_eval_frame: scalars must be numbers, pixels per metre positive, the radius not negative");
    const uintptr_t words = reinterpret_cast<uintptr_t>(pred_bev) | reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(locs) |
                            reinterpret_cast<uintptr_t>(typs) | reinterpret_cast<uintptr_t>(ego_plan) | reinterpret_cast<uintptr_t>(ego_locs) |
                            reinterpret_cast<uintptr_t>(other_cast) | reinterpret_cast<uintptr_t>(other_cmds) | reinterpret_cast<uintptr_t>(other_row);
    LAV_REQUIRE((words & 3) == 0 && (reinterpret_cast<uintptr_t>(acc) & 7) == 0,
                "lav_eval_frame: float32 / int32 tensors must be 4-byte, the accumulator 8-byte aligned");
    Args a;
    a.pred = pred_bev; a.labels = labels; a.mask = mask; a.h = h; a.w = w; a.threshold = threshold;
    a.rows = rows; a.max_det = max_det; a.locs = locs; a.typs = typs; a.max_objs = max_objs; a.num_objs = num_objs; a.num_plan = num_plan;
    a.ego_plan = ego_plan; a.ego_locs = ego_locs; a.cmd = cmd;
    a.other_cast = other_cast; a.other_cmds = other_cmds; a.other_row = other_row; a.num_others = num_others;
    a.ppm = ppm; a.cx = centre_x; a.cy = centre_y; a.radius = radius_px; a.min_score = min_score; a.det_score = det_score;
    a.nbins = nbins; a.acc = reinterpret_cast<unsigned long long *>(acc);
    const size_t quads = ((size_t)h * w + 3) / 4;
    const int groups = (int)std::min<size_t>((quads + THREADS - 1) / THREADS, MAX_SEG_GROUPS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("eval_frame", st);
    hipLaunchKernelGGL(k_eval_frame, dim3(groups + 1), dim3(THREADS), 0, st, a);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
