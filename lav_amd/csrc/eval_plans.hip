// Held-out metrics of the privileged BEV teacher over one loader batch (lav_eval_plans), added into one int64 accumulator that stays in
// HBM for a whole run.  The specification is lav_amd.train.evaluate_bev.eval_plans_numpy and the two agree in every word
// (tests/test_gpu_eval_bev.py): every counter is an integer, the distance sums are sums of distances quantised to 2^-20 m BEFORE they
// are added (quantum(), eval_quantum.hpp), so a route's result depends neither on the batch size nor on the order of its frames or of
// the workgroups.  There is no reference evaluator: the definitions are this project's, parity is UNPINNED.
//
// One launch.  The batch's B frames and K forecasts are B + K items, one WAVE each, four to a workgroup (items 0 .. B - 1 the frames);
// lane t holds waypoint t (T <= 64).  A frame's wave walks its S = I + 1 stages - stage 0 the cast at the frame's command, stage s
// refinement s - 1 of the plan at that command -, a forecast's wave its six modes; each is a wave sum and a ballot.  Nothing here has
// traffic (a frame reads S T + T + 7 points): the cost is the launch.  Lane 0 of a wave adds its item's integers into the workgroup's
// copy of the accumulator in LDS (64-bit LDS atomics: no store that could be paired), and the workgroup ends with one 64-bit vector
// atomic per counter it has something to add to.
#include "eval_quantum.hpp"

#pragma clang fp contract(off)

namespace {
using namespace lav;
constexpr int THREADS = 256, WAVES = THREADS / WAVE;
constexpr int CMDS = EVAL_CMDS, MAX_PLAN = 64, MAX_ITERS = 8, MAX_STAGES = MAX_ITERS + 1;
constexpr int MAX_BATCH = 1 << 20, MAX_OTHERS = 1 << 24;
// the accumulator's words for S stages; lav_amd.train.evaluate_bev.PlanLayout names the same slices (tests/test_eval_bev_host.py
// compares the lengths): frames, bad_cmd, plan [2][S][6][3], plan_nonfinite [S], cmd_conf [6][6], others, oth_nonfinite, oth [4],
// oth_min_mode [6], oth_top_mode [6], oth_top_is_min
struct Words {
    int plan = 0, plan_nonfinite = 0, cmd_conf = 0, others = 0, oth_nonfinite = 0, oth = 0, min_mode = 0, top_mode = 0, top_is_min = 0, total = 0;
    constexpr __host__ __device__ explicit Words(int S) {
        plan = 2;
        plan_nonfinite = plan + 2 * S * CMDS * 3;
        cmd_conf = plan_nonfinite + S;
        others = cmd_conf + CMDS * CMDS;
        oth_nonfinite = others + 1;
        oth = oth_nonfinite + 1;
        min_mode = oth + 4;
        top_mode = min_mode + CMDS;
        top_is_min = top_mode + CMDS;
        total = top_is_min + 1;
    }
};
constexpr int A_FRAMES = 0, A_BAD_CMD = 1;
constexpr int MAX_WORDS = 57 + 37 * MAX_STAGES;

struct Args {
    const float *ego_plan, *ego_cast, *ego_cmds, *ego_locs;
    const int *cmds;
    const unsigned char *bras;
    int batch, iters, num_plan;
    const float *other_cast, *other_cmds, *other_locs;
    int num_others;
    unsigned long long *acc;
};

__device__ __forceinline__ void add(unsigned long long *s_cnt, int word, long long v) { atomicAdd(s_cnt + word, (unsigned long long)v); }

// frame b: the cast and every refinement of the plan at the frame's command against ego_locs[b][t + 1]
__device__ void frame(const Args &a, const Words &w, int b, int lane, unsigned long long *s_cnt) {
    const int T = a.num_plan, I = a.iters, S = I + 1;
    const int cmd = a.cmds[b];
    if (lane == 0) add(s_cnt, A_FRAMES, 1);
    if (cmd < 0 || cmd >= CMDS) {                       // (uniform: one frame per wave)
        if (lane == 0) add(s_cnt, A_BAD_CMD, 1);
        return;
    }
    const int bra = a.bras[b] != 0 ? 1 : 0;
    const float *target = a.ego_locs + ((size_t)b * (T + 1) + 1) * 2;
    for (int s = 0; s < S; ++s) {
        const float *src = s == 0 ? a.ego_cast + ((size_t)b * CMDS + cmd) * T * 2
                                  : a.ego_plan + (((size_t)b * I + (s - 1)) * CMDS + cmd) * T * 2;
        long long q = 0;
        bool ok = true;
        if (lane < T) ok = quantum(src + (size_t)lane * 2, target + (size_t)lane * 2, q);
        const bool finite = __ballot(!ok) == 0;
        const long long sum = wave_sum(q), last = __shfl(q, T - 1, 64);
        if (lane == 0) {
            if (finite) {
                const int at = w.plan + ((bra * S + s) * CMDS + cmd) * 3;
                add(s_cnt, at, 1);
                add(s_cnt, at + 1, sum);
                add(s_cnt, at + 2, last);
            } else {
                add(s_cnt, w.plan_nonfinite + s, 1);
            }
        }
    }
    const int top = first_max(a.ego_cmds + (size_t)b * CMDS);
    if (lane == 0) add(s_cnt, w.cmd_conf + cmd * CMDS + top, 1);
}

// forecast k: its six modes against other_locs[k][t]
__device__ void forecast(const Args &a, const Words &w, int k, int lane, unsigned long long *s_cnt) {
    const int T = a.num_plan;
    const int top = first_max(a.other_cmds + (size_t)k * CMDS);
    const float *target = a.other_locs + (size_t)k * T * 2;
    long long s_min = 0, s_top = 0, last_min = 0, last_top = 0;
    int m_min = 0;
    bool finite = true;
    for (int m = 0; m < CMDS; ++m) {
        long long q = 0;
        bool ok = true;
        if (lane < T) ok = quantum(a.other_cast + (((size_t)k * CMDS + m) * T + lane) * 2, target + (size_t)lane * 2, q);
        finite = finite && __ballot(!ok) == 0;
        const long long s = wave_sum(q), last = __shfl(q, T - 1, 64);
        if (m == 0 || s < s_min) { s_min = s; last_min = last; m_min = m; }      // the first minimum
        if (m == top) { s_top = s; last_top = last; }
    }
    if (lane != 0) return;
    if (!finite) {
        add(s_cnt, w.oth_nonfinite, 1);
        return;
    }
    add(s_cnt, w.others, 1);
    add(s_cnt, w.oth, s_min);
    add(s_cnt, w.oth + 1, s_top);
    add(s_cnt, w.oth + 2, last_top);
    add(s_cnt, w.oth + 3, last_min);
    add(s_cnt, w.min_mode + m_min, 1);
    add(s_cnt, w.top_mode + top, 1);
    if (top == m_min) add(s_cnt, w.top_is_min, 1);
}

__global__ __launch_bounds__(THREADS) void k_eval_plans(Args a) {
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

extern "C" size_t lav_eval_plans_words(int iters) { return iters >= 1 && iters <= MAX_ITERS ? (size_t)Words(iters + 1).total : 0; }

extern "C" int lav_eval_plans(const float *ego_plan, const float *ego_cast, const float *ego_cmds, const float *ego_locs, const int *cmds,
                              const unsigned char *bras, int batch, int iters, int num_plan, const float *other_cast,
                              const float *other_cmds, const float *other_locs, int num_others, long long *acc, void *stream) {
    static_assert(Words(MAX_STAGES).total == MAX_WORDS && Words(2).total == 57 + 37 * 2, "57 + 37 S words");
    LAV_REQUIRE(ego_plan && ego_cast && ego_cmds && ego_locs && cmds && bras && acc, "lav_eval_plans: null argument");
    LAV_REQUIRE(batch >= 1 && batch <= MAX_BATCH, "lav_eval_plans: %d frames (1 .. %d)", batch, MAX_BATCH);
    LAV_REQUIRE(iters >= 1 && iters <= MAX_ITERS, "lav_eval_plans: %d plan iterations (1 .. %d)", iters, MAX_ITERS);
    LAV_REQUIRE(num_plan >= 1 && num_plan <= MAX_PLAN, "lav_eval_plans: %d waypoints (1 .. %d)", num_plan, MAX_PLAN);
    LAV_REQUIRE(num_others >= 0 && num_others <= MAX_OTHERS && ((other_cast && other_cmds && other_locs) || num_others == 0),
                "lav_eval_plans: %d forecasts (0 .. %d, with their three tensors)", num_others, MAX_OTHERS);
    const uintptr_t words = reinterpret_cast<uintptr_t>(ego_plan) | reinterpret_cast<uintptr_t>(ego_cast) | reinterpret_cast<uintptr_t>(ego_cmds) |
                            reinterpret_cast<uintptr_t>(ego_locs) | reinterpret_cast<uintptr_t>(cmds) | reinterpret_cast<uintptr_t>(other_cast) |
                            reinterpret_cast<uintptr_t>(other_cmds) | reinterpret_cast<uintptr_t>(other_locs);
    LAV_REQUIRE((words & 3) == 0 && (reinterpret_cast<uintptr_t>(acc) & 7) == 0,
                "lav_eval_plans: float32 / int32 tensors must be 4-byte, the accumulator 8-byte aligned");
    Args a;
    a.ego_plan = ego_plan; a.ego_cast = ego_cast; a.ego_cmds = ego_cmds; a.ego_locs = ego_locs; a.cmds = cmds; a.bras = bras;
    a.batch = batch; a.iters = iters; a.num_plan = num_plan;
    a.other_cast = other_cast; a.other_cmds = other_cmds; a.other_locs = other_locs; a.num_others = num_others;
    a.acc = reinterpret_cast<unsigned long long *>(acc);
    const long long items = (long long)batch + num_others;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("eval_plans", st);
    hipLaunchKernelGGL(k_eval_plans, dim3((unsigned)((items + WAVES - 1) / WAVES)), dim3(THREADS), 0, st, a);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
