// Rotated-box metrics of one evaluated frame's detections (lav_eval_det): the box and orientation heads' (w, h, cos, sin) against the
// loader's own regression targets, added into one int64 accumulator that stays in HBM for a whole route.  The specification is
// lav_amd.train.evaluate_det.eval_det_numpy, which has the definitions in full and the final word on the order of every operation; the
// two agree in every word (tests/test_gpu_eval_det.py).  Every counter is an integer and every error is quantised to 2^-20 BEFORE it is
// added, so a route's result does not depend on the order of its frames.  There is no reference evaluator: the definitions are this
// project's, parity is UNPINNED.
//
// One launch, ONE workgroup of eight waves; lane g of EVERY wave holds ground-truth actor g (pixel, box corners, range bin: registers,
// no hand-off).  First the waves share the rows (row = wave, wave + 8, ... over both classes) and each lane clips the row's
// quadrilateral against its actor's - Sutherland-Hodgman on at most 8 vertices - and leaves iou_q in the (class, row, actor) table in
// LDS (32-bit words).  Then wave 2 a + c is matching arm a on class c (the arms and the classes share nothing but the table): it walks
// the class's rows in order and takes the nearest (arm 0) or the best-overlapping (arms 1 ..) free actor by a wave minimum / maximum,
// ties to the lowest index by a ballot.  The head of the
// accumulator is gathered in LDS with 64-bit LDS atomics (no store that could be paired) and leaves as one vector atomic per counter
// that changed; the score histograms are 4 x 2 x 32 (arm, class, row) outcomes at most, one vector atomic each.
//
// Floating point: float64 from the float32 inputs, + - * /, sqrt and comparisons only, contraction off (here and in lav_amd/build.py),
// so that every product and sum rounds as Python rounds it; llrint rounds to nearest even like np.rint.
#include "eval_quantum.hpp"      // EVAL_Q, EVAL_FAR

#pragma clang fp contract(off)

namespace {
using namespace lav;
constexpr int THREADS = 512, WAVES = THREADS / WAVE;
constexpr int MAX_DET = 32, MAX_OBJS = 64, MAX_BINS = 1024, ARMS = 4, MAX_IOU = 3, MAX_RANGE = 3, MAX_HEADING = 7, MAX_VERTS = 8;
constexpr int IOU_ONE = 1 << 20;
// the accumulator's words; lav_amd.train.evaluate_det.DetLayout names the same slices (tests/test_eval_det_host.py compares the lengths)
constexpr int A_FRAMES = 0, A_NGT = 1, A_GT_INVALID = A_NGT + 8, A_PRED_INVALID = A_GT_INVALID + 2, A_DET = A_PRED_INVALID + 2,
              A_PAIRS = A_DET + ARMS * 16, A_PAIR_INVALID = A_PAIRS + 8, A_SUM_CENTRE = A_PAIR_INVALID + 2, A_SUM_DW = A_SUM_CENTRE + 8,
              A_SUM_DH = A_SUM_DW + 8, A_SUM_IOU = A_SUM_DH + 8, A_HEADING = A_SUM_IOU + 8, A_HIST = A_HEADING + 16;
static_assert(A_HIST == 135, "135 + 16 nbins words");

struct Args {
    const float *rows;
    int max_det;
    const float *locs;
    const int *typs;
    int num_objs, num_plan;
    const float *size_map, *ori_map;
    int h, w;
    double ppm, cx, cy, radius, min_score, det_score;
    long long iou_q[MAX_IOU];
    double range2[MAX_RANGE], heading_cos[MAX_HEADING];
    int num_iou, num_range, num_heading, nbins;
    unsigned long long *acc;
};

struct Box {
    bool valid;
    double x[4], y[4];      // corners, counter-clockwise
    double w, h, c, s;      // half extents, the unit direction
};

__device__ __forceinline__ bool finite(double v) { return fabs(v) < __longlong_as_double(0x7ff0000000000000ll); }      // (false for a NaN)

__device__ __forceinline__ void add(unsigned long long *s_cnt, int word, long long v) { atomicAdd(s_cnt + word, (unsigned long long)v); }

__device__ Box make_box(double cx, double cy, double w, double h, double c, double s) {
    Box b;
    b.valid = false;
    b.w = w; b.h = h; b.c = 0.0; b.s = 0.0;
    for (int k = 0; k < 4; ++k) b.x[k] = b.y[k] = 0.0;
    if (!(finite(cx) && finite(cy) && finite(w) && finite(h) && finite(c) && finite(s))) return b;
    if (!(w > 0.0 && h > 0.0)) return b;
    const double n = c * c + s * s;
    if (!(finite(n) && n > 0.0)) return b;
    const double r = sqrt(n);
    const double ch = c / r, sh = s / r;
    const double ux = sh, uy = -ch, vx = ch, vy = sh;
    b.x[0] = cx - w * ux - h * vx; b.y[0] = cy - w * uy - h * vy;
    b.x[1] = cx + w * ux - h * vx; b.y[1] = cy + w * uy - h * vy;
    b.x[2] = cx + w * ux + h * vx; b.y[2] = cy + w * uy + h * vy;
    b.x[3] = cx - w * ux + h * vx; b.y[3] = cy - w * uy + h * vy;
    b.c = ch; b.s = sh;
    b.valid = true;
    return b;
}

// iou_q of a prediction against a ground-truth box
__device__ int iou_quanta(const Box &p, const Box &g) {
    if (!p.valid || !g.valid) return 0;
    double ax[MAX_VERTS], ay[MAX_VERTS], bx[MAX_VERTS], by[MAX_VERTS];
    int n = 4;
    for (int k = 0; k < 4; ++k) { ax[k] = p.x[k]; ay[k] = p.y[k]; }
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        const double gx = g.x[k], gy = g.y[k], ex = g.x[k1] - gx, ey = g.y[k1] - gy;
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int j = i + 1 == n ? 0 : i + 1;
            const double dS = ex * (ay[i] - gy) - ey * (ax[i] - gx), dE = ex * (ay[j] - gy) - ey * (ax[j] - gx);
            const bool in_s = dS >= 0.0, in_e = dE >= 0.0;
            if (in_s && m < MAX_VERTS) { bx[m] = ax[i]; by[m] = ay[i]; ++m; }
            if (in_s != in_e && m < MAX_VERTS) {
                const double t = dS / (dS - dE);
                bx[m] = ax[i] + t * (ax[j] - ax[i]);
                by[m] = ay[i] + t * (ay[j] - ay[i]);
                ++m;
            }
        }
        n = m;
        for (int i = 0; i < n; ++i) { ax[i] = bx[i]; ay[i] = by[i]; }
    }
    double total = 0.0;
    for (int i = 1; i + 1 < n; ++i) {
        const double px = ax[i] - ax[0], py = ay[i] - ay[0], qx = ax[i + 1] - ax[0], qy = ay[i + 1] - ay[0];
        total = total + (px * qy - py * qx);
    }
    const double area = 0.5 * fabs(total);
    const double uni = ((2.0 * p.w) * (2.0 * p.h) + (2.0 * g.w) * (2.0 * g.h)) - area;
    if (!(area > 0.0 && uni > 0.0)) return 0;
    const double q = area / uni;
    if (!finite(q)) return 0;
    const double x = q * EVAL_Q;
    return x >= EVAL_Q ? IOU_ONE : (int)llrint(x);
}

// llrint(min(x, 2^32) 2^20) of a non-negative finite x
__device__ __forceinline__ long long quanta_of(double x) { return llrint((x < EVAL_FAR ? x : EVAL_FAR) * EVAL_Q); }

__device__ __forceinline__ int range_bin(const Args &a, double d2) {
    int b = 0;
    for (int k = 0; k < a.num_range; ++k) b += d2 >= a.range2[k] ? 1 : 0;
    return b;
}

// whether make_box would call the row's box valid (no square root, no division)
__device__ __forceinline__ bool row_valid(const float *row) {
    const double x = (double)row[1], y = (double)row[2], w = (double)row[3], h = (double)row[4], c = (double)row[5], s = (double)row[6];
    const double n = c * c + s * s;
    return finite(x) && finite(y) && finite(w) && finite(h) && finite(c) && finite(s) && w > 0.0 && h > 0.0 && finite(n) && n > 0.0;
}

__device__ __forceinline__ Box row_box(const float *row) {
    return make_box((double)row[1], (double)row[2], (double)row[3], (double)row[4], (double)row[5], (double)row[6]);
}

__global__ __launch_bounds__(THREADS) void k_eval_det(Args a) {
    __shared__ int s_iou[2][MAX_DET][MAX_OBJS];          // iou_q of (class, row, actor); 0 where the pair does not exist
    __shared__ unsigned long long s_cnt[A_HIST];         // the frame's share of the accumulator's head
    __shared__ int s_hit[ARMS][2][MAX_DET];              // per arm, class and row: 0 not counted, 1 true positive, 2 false positive
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.max_det;
    for (int i = tid; i < A_HIST; i += THREADS) {
        s_cnt[i] = 0;
        lds_store_fence();
    }
    for (int i = tid; i < ARMS * 2 * MAX_DET; i += THREADS) (&s_hit[0][0][0])[i] = 0;

    // ground-truth actor `lane`: its class (-1: none, or outside the map), pixel, box and range bin
    int cls = -1, rb_g = 0;
    double px = 0.0, py = 0.0;
    Box gb = make_box(0.0, 0.0, 0.0, 0.0, 0.0, 0.0);     // (invalid)
    if (lane < a.num_objs) {
        const int typ = a.typs[lane];
        const float *loc = a.locs + (size_t)lane * (a.num_plan + 1) * 2;
        px = (double)loc[0] * a.ppm + a.cx;
        py = (double)loc[1] * a.ppm + a.cy;
        if ((typ == 0 || typ == 1) && px >= 0.0 && px < (double)a.w && py >= 0.0 && py < (double)a.h) {
            cls = typ;
            int ix = (int)(px + 0.5), iy = (int)(py + 0.5);
            ix = ix < a.w - 1 ? ix : a.w - 1;
            iy = iy < a.h - 1 ? iy : a.h - 1;
            const size_t plane = (size_t)a.h * a.w, at = (size_t)iy * a.w + ix;
            gb = make_box(px, py, (double)a.size_map[at], (double)a.size_map[plane + at], (double)a.ori_map[at], (double)a.ori_map[plane + at]);
            const double dx = px - a.cx, dy = py - a.cy;
            rb_g = range_bin(a, dx * dx + dy * dy);
        }
    }
    __syncthreads();
    if (tid == 0) add(s_cnt, A_FRAMES, 1);
    if (wave == 0 && cls >= 0) {
        add(s_cnt, A_NGT + cls * 4 + rb_g, 1);
        if (!gb.valid) add(s_cnt, A_GT_INVALID + cls, 1);
    }

    // the table: the waves share the 2 D rows
    for (int cr = wave; cr < 2 * D; cr += WAVES) {
        const int c = cr / D, r = cr - c * D;
        const float *row = a.rows + (size_t)cr * 7;
        int q = 0;
        if ((double)row[0] > a.min_score && cls == c) q = iou_quanta(row_box(row), gb);
        s_iou[c][r][lane] = q;
    }
    __syncthreads();

    if ((wave >> 1) <= a.num_iou) {                      // wave 2 arm + class: one walk over that class's rows
        const int arm = wave >> 1;
        const double r2 = a.radius * a.radius, inf = __longlong_as_double(0x7ff0000000000000ll);
        const long long need = arm > 0 ? a.iou_q[arm - 1] : 0;
        {
            const int c = wave & 1;
            const bool mine = cls == c;
            bool taken = false;
            for (int r = 0; r < D; ++r) {                // (uniform: every lane reads the same row)
                const float *row = a.rows + ((size_t)c * D + r) * 7;
                const float score = row[0];
                if (!((double)score > a.min_score)) continue;
                const double x = (double)row[1], y = (double)row[2];
                const double dx = x - px, dy = y - py;
                const double d2 = dx * dx + dy * dy;
                unsigned long long winners;
                if (arm == 0) {                          // lav_eval_frame's centre rule
                    const bool cand = mine && !taken && d2 <= r2;
                    double best = cand ? d2 : inf;
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) {
                        const double other = __shfl_xor(best, o, 64);
                        best = other < best ? other : best;
                    }
                    winners = __ballot(cand && d2 == best);
                } else {
                    const int q = s_iou[c][r][lane];
                    const bool cand = mine && !taken && (long long)q >= need && q > 0;
                    int best = cand ? q : -1;
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) {
                        const int other = __shfl_xor(best, o, 64);
                        best = other > best ? other : best;
                    }
                    winners = __ballot(cand && q == best);
                }
                const int g = winners ? __ffsll((long long)winners) - 1 : -1;       // the lowest index among the best
                const bool hit = g >= 0;
                if (lane == g) taken = true;
                if (lane == 0) s_hit[arm][c][r] = hit ? 1 : 2;
                bool pred_valid = true;
                if (arm == 0) {                          // (uniform: the row's own box)
                    pred_valid = row_valid(row);
                    if (!pred_valid && lane == 0) add(s_cnt, A_PRED_INVALID + c, 1);
                }
                if (!((double)score > a.det_score)) continue;
                const double ex = x - a.cx, ey = y - a.cy;
                const int rb_row = range_bin(a, ex * ex + ey * ey), rb_hit = __shfl(rb_g, hit ? g : 0, 64);
                const int rb = hit ? rb_hit : rb_row;
                if (lane == 0) add(s_cnt, A_DET + ((arm * 2 + c) * 4 + rb) * 2 + (hit ? 0 : 1), 1);
                if (arm == 0 && lane == g) {             // the matched pair, by the actor's lane
                    add(s_cnt, A_PAIRS + c * 4 + rb, 1);
                    if (!pred_valid || !gb.valid) add(s_cnt, A_PAIR_INVALID + c, 1);
                    else {
                        const Box pb = row_box(row);
                        add(s_cnt, A_SUM_CENTRE + c * 4 + rb, quanta_of(sqrt(d2) / a.ppm));
                        add(s_cnt, A_SUM_DW + c * 4 + rb, quanta_of(fabs(pb.w - gb.w) / a.ppm));
                        add(s_cnt, A_SUM_DH + c * 4 + rb, quanta_of(fabs(pb.h - gb.h) / a.ppm));
                        add(s_cnt, A_SUM_IOU + c * 4 + rb, s_iou[c][r][lane]);
                        const double dot = pb.c * gb.c + pb.s * gb.s;
                        int bin = a.num_heading;         // a NaN goes to the last bin
                        if (dot == dot) {
                            bin = 0;
                            for (int k = 0; k < a.num_heading; ++k) bin += dot < a.heading_cos[k] ? 1 : 0;
                        }
                        add(s_cnt, A_HEADING + c * 8 + bin, 1);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < A_HIST; i += THREADS)
        if (s_cnt[i] != 0) atomicAdd(a.acc + i, s_cnt[i]);
    if (tid < ARMS * 2 * MAX_DET) {                      // the score histograms: thread = (arm, class, row)
        const int arm = tid >> 6, c = (tid >> 5) & 1, r = tid & 31;
        const int hit = r < D ? s_hit[arm][c][r] : 0;
        if (hit != 0) {
            const float score = a.rows[((size_t)c * D + r) * 7];
            const float scaled = score * (float)a.nbins;
            const int bin = scaled >= (float)(a.nbins - 1) ? a.nbins - 1 : (int)scaled;
            atomicAdd(a.acc + A_HIST + (size_t)((arm * 2 + c) * 2 + (hit == 1 ? 0 : 1)) * a.nbins + bin, 1ull);
        }
    }
}
static_assert(THREADS >= ARMS * 2 * MAX_DET && WAVES == ARMS * 2 && MAX_OBJS == WAVE && MAX_DET == 32,
              "a thread per (arm, class, row), a wave per (arm, class), a lane per actor");
}  // namespace

extern "C" size_t lav_eval_det_words(int nbins) { return nbins >= 1 && nbins <= MAX_BINS ? (size_t)A_HIST + 16 * (size_t)nbins : 0; }

extern "C" int lav_eval_det(const float *rows, int max_det, const float *locs, const int *typs, int max_objs, int num_objs, int num_plan,
                            const float *size_map, const float *ori_map, int h, int w, double ppm, double centre_x, double centre_y,
                            double radius_px, double min_score, double det_score, const long long *iou_q, int num_iou, const double *range2,
                            int num_range, const double *heading_cos, int num_heading, int nbins, long long *acc, void *stream) {
    LAV_REQUIRE(rows && size_map && ori_map && acc, "lav_eval_det: null argument");
    LAV_REQUIRE(h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "lav_eval_det: map %d x %d", h, w);
    LAV_REQUIRE(max_det >= 1 && max_det <= MAX_DET, "lav_eval_det: %d rows per class (1 .. %d)", max_det, MAX_DET);
    LAV_REQUIRE(max_objs >= 0 && max_objs <= MAX_OBJS && num_objs >= 0 && num_objs <= max_objs && ((locs && typs) || num_objs == 0),
                "lav_eval_det: %d of %d ground-truth actors (at most %d, with their two tensors)", num_objs, max_objs, MAX_OBJS);
    LAV_REQUIRE(num_plan >= 0 && num_plan <= 4096, "lav_eval_det: %d waypoints behind an actor's position", num_plan);
    LAV_REQUIRE(nbins >= 1 && nbins <= MAX_BINS, "lav_eval_det: %d score bins (1 .. %d)", nbins, MAX_BINS);
    LAV_REQUIRE(num_iou >= 0 && num_iou <= MAX_IOU && (iou_q || num_iou == 0), "lav_eval_det: %d IoU thresholds (0 .. %d)", num_iou, MAX_IOU);
    LAV_REQUIRE(num_range >= 0 && num_range <= MAX_RANGE && (range2 || num_range == 0), "lav_eval_det: %d range edges (0 .. %d)", num_range, MAX_RANGE);
    LAV_REQUIRE(num_heading >= 0 && num_heading <= MAX_HEADING && (heading_cos || num_heading == 0), "lav_eval_det: %d heading edges (0 .. %d)",
                num_heading, MAX_HEADING);
    LAV_REQUIRE(ppm > 0.0 && ppm <= 1e6 && radius_px >= 0.0 && centre_x == centre_x && centre_y == centre_y && min_score >= 0.0 &&
                    det_score == det_score, "lav_eval_det: scalars must be numbers, pixels per metre positive, the radius and min_score not negative");
    Args a;
    for (int k = 0; k < MAX_IOU; ++k) a.iou_q[k] = k < num_iou ? iou_q[k] : 0;
    for (int k = 0; k < MAX_RANGE; ++k) a.range2[k] = k < num_range ? range2[k] : 0.0;
    for (int k = 0; k < MAX_HEADING; ++k) a.heading_cos[k] = k < num_heading ? heading_cos[k] : 0.0;
    for (int k = 0; k < num_iou; ++k) LAV_REQUIRE(a.iou_q[k] >= 1 && a.iou_q[k] <= IOU_ONE, "lav_eval_det: IoU threshold %d of 2^20", (int)a.iou_q[k]);
    for (int k = 0; k < num_range; ++k) LAV_REQUIRE(a.range2[k] == a.range2[k], "lav_eval_det: range edge %d is not a number", k);
    for (int k = 0; k < num_heading; ++k) LAV_REQUIRE(a.heading_cos[k] == a.heading_cos[k], "lav_eval_det: heading edge %d is not a number", k);
    const uintptr_t words = reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(locs) | reinterpret_cast<uintptr_t>(typs) |
                            reinterpret_cast<uintptr_t>(size_map) | reinterpret_cast<uintptr_t>(ori_map);
    LAV_REQUIRE((words & 3) == 0 && (reinterpret_cast<uintptr_t>(acc) & 7) == 0,
                "lav_eval_det: float32 / int32 tensors must be 4-byte, the accumulator 8-byte aligned");
    a.rows = rows; a.max_det = max_det; a.locs = locs; a.typs = typs; a.num_objs = num_objs; a.num_plan = num_plan;
    a.size_map = size_map; a.ori_map = ori_map; a.h = h; a.w = w;
    a.ppm = ppm; a.cx = centre_x; a.cy = centre_y; a.radius = radius_px; a.min_score = min_score; a.det_score = det_score;
    a.num_iou = num_iou; a.num_range = num_range; a.num_heading = num_heading; a.nbins = nbins;
    a.acc = reinterpret_cast<unsigned long long *>(acc);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("eval_det", st);
    hipLaunchKernelGGL(k_eval_det, dim3(1), dim3(THREADS), 0, st, a);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
