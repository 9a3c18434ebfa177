// The LiDAR student beside the BEV teacher it was distilled from, on the same frames and the same crops (lav_eval_distill), added into one
// int64 accumulator that stays in HBM for a whole run.  The specification is lav_amd.train.evaluate_distill.eval_distill_numpy and the
// two agree in every word (tests/test_gpu_eval_distill.py): every counter is an integer, every comparison is between integers (sums of
// distances quantised to 2^-20 m BEFORE they are added: quantum(), eval_quantum.hpp), so a route's result depends neither on the batch
// size nor on the order of its frames or of the workgroups.  There is no reference evaluator: the definitions are this project's
// (DESIGN 4.7k), parity is UNPINNED.
//
// One launch, built as eval_plans.hip is.  The group's B frames and K forecasts are B + K items, one WAVE each, four to a workgroup
// (items 0 .. B - 1 the frames); lane t holds waypoint t (T <= 64).  A frame's wave walks its S = I + 1 stages - stage 0 the cast, stage
// s refinement s - 1 of the plan - and in each the six modes, student against teacher, then both against the recorded future at the
// frame's command; a forecast's wave its six modes three times (student and teacher against the vehicle's future, student against
// teacher).  Each is a wave sum and a ballot; there is no traffic to speak of (a frame reads 2 (6 S T + 6) + T + 2 points), the cost is
// the launch.  Lane 0 of a wave adds its item's integers into the workgroup's copy of the accumulator in LDS (64-bit LDS atomics: no
// store that could be paired), and the workgroup ends with one 64-bit vector atomic per counter it has something to add to.
#include "eval_quantum.hpp"

#pragma clang fp contract(off)

namespace {
using namespace lav;
constexpr int THREADS = 256, WAVES = THREADS / WAVE;
constexpr int CMDS = EVAL_CMDS, MAX_PLAN = 64, MAX_ITERS = 8, MAX_STAGES = MAX_ITERS + 1;
constexpr int MAX_BATCH = 1 << 20, MAX_OTHERS = 1 << 24;
// the accumulator's words for S stages; lav_amd.train.evaluate_distill.PairLayout names the same slices (tests/test_eval_distill_host.py
// compares the lengths): frames, bad_cmd, ego_gap [S][6][3], ego_gap_nonfinite [S], ego_closer [S][6][3], ego_unjudged [S], cmd_agree
// [6][6], cmd_gap [6][2], cmd_nonfinite, others, oth_nonfinite, oth_gap [6][2], oth_closer [3], oth_closer_top [3], oth_same_min,
// oth_top_agree [6][6], oth_cmd_gap [6]
struct Words {
    int ego_gap = 0, ego_gap_nonfinite = 0, ego_closer = 0, ego_unjudged = 0, cmd_agree = 0, cmd_gap = 0, cmd_nonfinite = 0, others = 0,
        oth_nonfinite = 0, oth_gap = 0, oth_closer = 0, oth_closer_top = 0, oth_same_min = 0, oth_top_agree = 0, oth_cmd_gap = 0, total = 0;
    constexpr __host__ __device__ explicit Words(int S) {
        ego_gap = 2;
        ego_gap_nonfinite = ego_gap + S * CMDS * 3;
        ego_closer = ego_gap_nonfinite + S;
        ego_unjudged = ego_closer + S * CMDS * 3;
        cmd_agree = ego_unjudged + S;
        cmd_gap = cmd_agree + CMDS * CMDS;
        cmd_nonfinite = cmd_gap + CMDS * 2;
        others = cmd_nonfinite + 1;
        oth_nonfinite = others + 1;
        oth_gap = oth_nonfinite + 1;
        oth_closer = oth_gap + CMDS * 2;
        oth_closer_top = oth_closer + 3;
        oth_same_min = oth_closer_top + 3;
        oth_top_agree = oth_same_min + 1;
        oth_cmd_gap = oth_top_agree + CMDS * CMDS;
        total = oth_cmd_gap + CMDS;
    }
};
constexpr int A_FRAMES = 0, A_BAD_CMD = 1;
constexpr int MAX_WORDS = 114 + 38 * MAX_STAGES;
constexpr int STUDENT = 0, TEACHER = 1, TIE = 2;        // the three words of a "closer" counter

struct Arm {                                            // one network's outputs (BatchInference's, without the indices)
    const float *ego_plan, *ego_cast, *ego_cmds, *other_cast, *other_cmds;
};

struct Args {
    Arm s, t;                                           // the student's, the teacher's
    const float *ego_locs, *other_locs;
    const int *cmds;
    int batch, iters, num_plan, num_others;
    unsigned long long *acc;
};

__device__ __forceinline__ void add(unsigned long long *s_cnt, int word, long long v) { atomicAdd(s_cnt + word, (unsigned long long)v); }

// which of two integer errors is the smaller: the word of a "closer" counter
__device__ __forceinline__ int closer(long long student, long long teacher) { return student < teacher ? STUDENT : teacher < student ? TEACHER : TIE; }

// stage s, mode m of frame b of one arm
__device__ __forceinline__ const float *stage_of(const Arm &arm, int b, int s, int m, int I, int T) {
    return s == 0 ? arm.ego_cast + ((size_t)b * CMDS + m) * T * 2 : arm.ego_plan + (((size_t)b * I + (s - 1)) * CMDS + m) * T * 2;
}

// the wave's sum of q_t of `a` against `b` (T points each) and q_{T-1}; false where a distance is not below 2^32 m
__device__ __forceinline__ bool path_gap(const float *a, const float *b, int T, int lane, long long &sum, long long &last) {
    long long q = 0;
    bool ok = true;
    if (lane < T) ok = quantum(a + (size_t)lane * 2, b + (size_t)lane * 2, q);
    const bool finite = __ballot(!ok) == 0;
    sum = wave_sum(q);
    last = __shfl(q, T - 1, 64);
    return finite;
}

// frame b: every stage and mode of the student against the teacher's, both at the frame's command against ego_locs[b][t + 1], and the
// two sets of command scores
__device__ void frame(const Args &a, const Words &w, int b, int lane, unsigned long long *s_cnt) {
    const int T = a.num_plan, I = a.iters, S = I + 1;
    const int cmd = a.cmds[b];
    if (lane == 0) add(s_cnt, A_FRAMES, 1);
    if (cmd < 0 || cmd >= CMDS) {                       // (uniform: one frame per wave)
        if (lane == 0) add(s_cnt, A_BAD_CMD, 1);
        return;
    }
    const float *target = a.ego_locs + ((size_t)b * (T + 1) + 1) * 2;
    for (int s = 0; s < S; ++s) {
        for (int m = 0; m < CMDS; ++m) {
            long long sum, last;
            const bool finite = path_gap(stage_of(a.s, b, s, m, I, T), stage_of(a.t, b, s, m, I, T), T, lane, sum, last);
            if (lane == 0) {
                if (finite) {
                    const int at = w.ego_gap + (s * CMDS + m) * 3;
                    add(s_cnt, at, 1);
                    add(s_cnt, at + 1, sum);
                    add(s_cnt, at + 2, last);
                } else {
                    add(s_cnt, w.ego_gap_nonfinite + s, 1);
                }
            }
        }
        long long sum_s, sum_t, last;
        const bool ok_s = path_gap(stage_of(a.s, b, s, cmd, I, T), target, T, lane, sum_s, last);
        const bool ok_t = path_gap(stage_of(a.t, b, s, cmd, I, T), target, T, lane, sum_t, last);
        if (lane == 0) {
            if (ok_s && ok_t) add(s_cnt, w.ego_closer + (s * CMDS + cmd) * 3 + closer(sum_s, sum_t), 1);
            else add(s_cnt, w.ego_unjudged + s, 1);
        }
    }
    if (lane != 0) return;
    const float *cs = a.s.ego_cmds + (size_t)b * CMDS, *ct = a.t.ego_cmds + (size_t)b * CMDS;
    add(s_cnt, w.cmd_agree + first_max(ct) * CMDS + first_max(cs), 1);
    for (int m = 0; m < CMDS; ++m) {
        long long g = 0;
        if (scalar_gap(cs[m], ct[m], g)) {
            add(s_cnt, w.cmd_gap + m * 2, 1);
            add(s_cnt, w.cmd_gap + m * 2 + 1, g);
        } else {
            add(s_cnt, w.cmd_nonfinite, 1);
        }
    }
}

// forecast k: the six modes of both arms against other_locs[k][t] and against each other, and the two sets of mode scores
__device__ void forecast(const Args &a, const Words &w, int k, int lane, unsigned long long *s_cnt) {
    const int T = a.num_plan;
    const float *cs = a.s.other_cmds + (size_t)k * CMDS, *ct = a.t.other_cmds + (size_t)k * CMDS;
    const int top_s = first_max(cs), top_t = first_max(ct);
    const float *target = a.other_locs + (size_t)k * T * 2;
    long long min_s = 0, min_t = 0, at_top_s = 0, at_top_t = 0, gap_sum[CMDS], gap_last[CMDS], score[CMDS];
    int m_min_s = 0, m_min_t = 0;
    bool finite = true;
#pragma unroll
    for (int m = 0; m < CMDS; ++m) {
        const float *ps = a.s.other_cast + ((size_t)k * CMDS + m) * T * 2, *pt = a.t.other_cast + ((size_t)k * CMDS + m) * T * 2;
        long long sum_s, sum_t, last;
        finite = path_gap(ps, target, T, lane, sum_s, last) && finite;
        finite = path_gap(pt, target, T, lane, sum_t, last) && finite;
        finite = path_gap(ps, pt, T, lane, gap_sum[m], gap_last[m]) && finite;
        finite = scalar_gap(cs[m], ct[m], score[m]) && finite;
        if (m == 0 || sum_s < min_s) { min_s = sum_s; m_min_s = m; }             // the first minimum, each arm its own
        if (m == 0 || sum_t < min_t) { min_t = sum_t; m_min_t = m; }
        if (m == top_s) at_top_s = sum_s;
        if (m == top_t) at_top_t = sum_t;
    }
    if (lane != 0) return;
    if (!finite) {
        add(s_cnt, w.oth_nonfinite, 1);
        return;
    }
    add(s_cnt, w.others, 1);
#pragma unroll
    for (int m = 0; m < CMDS; ++m) {
        add(s_cnt, w.oth_gap + m * 2, gap_sum[m]);
        add(s_cnt, w.oth_gap + m * 2 + 1, gap_last[m]);
        add(s_cnt, w.oth_cmd_gap + m, score[m]);
    }
    add(s_cnt, w.oth_closer + closer(min_s, min_t), 1);
    add(s_cnt, w.oth_closer_top + closer(at_top_s, at_top_t), 1);
    if (m_min_s == m_min_t) add(s_cnt, w.oth_same_min, 1);
    add(s_cnt, w.oth_top_agree + top_t * CMDS + top_s, 1);
}

__global__ __launch_bounds__(THREADS) void k_eval_distill(Args a) {
    __shared__ unsigned long long s_cnt[MAX_WORDS];     // the workgroup's share of the accumulator
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Words w(a.iters + 1);
    for (int i = tid; i < w.total; i += THREADS) {
        s_cnt[i] = 0;
        lds_store_fence();
    }
    __syncthreads();
    const long long item = (long long)blockIdx.x * WAVES + wave;      // (uniform within a wave)
    if (item < a.batch) frame(a, w, (int)item, lane, s_cnt);
    else if (item < (long long)a.batch + a.num_others) forecast(a, w, (int)(item - a.batch), lane, s_cnt);
    __syncthreads();
    for (int i = tid; i < w.total; i += THREADS)
        if (s_cnt[i] != 0) atomicAdd(a.acc + i, s_cnt[i]);
}
}  // namespace

extern "C" size_t lav_eval_distill_words(int iters) { return iters >= 1 && iters <= MAX_ITERS ? (size_t)Words(iters + 1).total : 0; }

extern "C" int lav_eval_distill(const float *s_ego_plan, const float *s_ego_cast, const float *s_ego_cmds, const float *t_ego_plan,
                                const float *t_ego_cast, const float *t_ego_cmds, const float *ego_locs, const int *cmds, int batch, int iters,
                                int num_plan, const float *s_other_cast, const float *s_other_cmds, const float *t_other_cast,
                                const float *t_other_cmds, const float *other_locs, int num_others, long long *acc, void *stream) {
    static_assert(Words(MAX_STAGES).total == MAX_WORDS && Words(2).total == 114 + 38 * 2, "114 + 38 S words");
    LAV_REQUIRE(s_ego_plan && s_ego_cast && s_ego_cmds && t_ego_plan && t_ego_cast && t_ego_cmds && ego_locs && cmds && acc,
                "lav_eval_distill: null argument");
    LAV_REQUIRE(batch >= 1 && batch <= MAX_BATCH, "lav_eval_distill: %d frames (1 .. %d)", batch, MAX_BATCH);
    LAV_REQUIRE(iters >= 1 && iters <= MAX_ITERS, "lav_eval_distill: %d plan iterations (1 .. %d)", iters, MAX_ITERS);
    LAV_REQUIRE(num_plan >= 1 && num_plan <= MAX_PLAN, "lav_eval_distill: %d waypoints (1 .. %d)", num_plan, MAX_PLAN);
    LAV_REQUIRE(num_others >= 0 && num_others <= MAX_OTHERS &&
                    ((s_other_cast && s_other_cmds && t_other_cast && t_other_cmds && other_locs) || num_others == 0),
                "lav_eval_distill: %d forecasts (0 .. %d, with their five tensors)", num_others, MAX_OTHERS);
    const uintptr_t words = reinterpret_cast<uintptr_t>(s_ego_plan) | reinterpret_cast<uintptr_t>(s_ego_cast) | reinterpret_cast<uintptr_t>(s_ego_cmds) |
                            reinterpret_cast<uintptr_t>(t_ego_plan) | reinterpret_cast<uintptr_t>(t_ego_cast) | reinterpret_cast<uintptr_t>(t_ego_cmds) |
                            reinterpret_cast<uintptr_t>(ego_locs) | reinterpret_cast<uintptr_t>(cmds) | reinterpret_cast<uintptr_t>(s_other_cast) |
                            reinterpret_cast<uintptr_t>(s_other_cmds) | reinterpret_cast<uintptr_t>(t_other_cast) |
                            reinterpret_cast<uintptr_t>(t_other_cmds) | reinterpret_cast<uintptr_t>(other_locs);
    LAV_REQUIRE((words & 3) == 0 && (reinterpret_cast<uintptr_t>(acc) & 7) == 0,
                "lav_eval_distill: float32 / int32 tensors must be 4-byte, the accumulator 8-byte aligned");
    Args a;
    a.s = Arm{s_ego_plan, s_ego_cast, s_ego_cmds, s_other_cast, s_other_cmds};
    a.t = Arm{t_ego_plan, t_ego_cast, t_ego_cmds, t_other_cast, t_other_cmds};
    a.ego_locs = ego_locs; a.other_locs = other_locs; a.cmds = cmds;
    a.batch = batch; a.iters = iters; a.num_plan = num_plan; a.num_others = num_others;
    a.acc = reinterpret_cast<unsigned long long *>(acc);
    const long long items = (long long)batch + num_others;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("eval_distill", st);
    hipLaunchKernelGGL(k_eval_distill, dim3((unsigned)((items + WAVES - 1) / WAVES)), dim3(THREADS), 0, st, a);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
