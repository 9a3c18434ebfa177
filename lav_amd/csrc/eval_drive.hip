// Open-loop metrics of the agent's rule layer over one evaluated frame (lav_eval_drive): LAVAgent.plan_collide and pid_control's brake
// flag, restated on quantised distances, against the expert's brake label and the recorded futures, added into one int64 accumulator
// that stays in HBM for a whole run.  The specification is lav_amd.train.evaluate_drive.eval_drive_numpy and the two agree in every word
// (tests/test_gpu_eval_drive.py): every counter is an integer and every distance is quantised to 2^-20 m BEFORE it is summed or compared
// (quantum(), eval_quantum.hpp), so a route's result does not depend on the order of its frames.  There is no reference evaluator: the
// definitions are this project's, parity is UNPINNED.
//
// One launch, ONE workgroup of four waves.  The items are the 6 N forecast modes and the n tracks, one WAVE each; a wave loops over its
// share (item = wave, wave + 4, ...); lane t holds waypoint t (T <= 64).  An item is a wave sum (the path length), a wave minimum (the
// clearance) and a ballot.  The frame's counters need every item's result - any hit, the least clearance per kind -, which is why there
// is one workgroup: 6 * 64 + 64 items of at most 64 points are microseconds, the cost is the launch, and a second workgroup would need a
// grid-wide hand-off.  Every wave checks the driven path for itself (T points) so that a frame without one leaves before anything is
// shared; wave 0 also measures it against the expert.  Lane 0 of a wave adds its items' integers into the workgroup's copy of the
// accumulator in LDS (64-bit LDS atomics: no store that could be paired) and leaves its bits and clearances there; thread 0 makes the
// frame's counters of them, and the workgroup ends with one 64-bit vector atomic per counter it has something to add to.
#include "eval_quantum.hpp"

#pragma clang fp contract(off)

namespace {
using namespace lav;
constexpr int THREADS = 256, WAVES = THREADS / WAVE;
constexpr int CMDS = EVAL_CMDS, MIN_PLAN = 2, MAX_PLAN = 64, MAX_OTHERS = 64, MAX_OBJS = 64, MAX_BINS = 1024;
constexpr int SPEED_SHIFT = 14, CLEAR_SHIFT = 17;          // 1/64 m per step, 1/8 m
constexpr double MAX_RULE = 1e6;                           // the rule parameters' bound: S and L stay far inside 64 bits
// the accumulator's words; lav_amd.train.evaluate_drive.DriveLayout names the same slices (tests/test_eval_drive_host.py compares the
// lengths): frames, plan_nonfinite, expert_nonfinite, cause [2][8], gt_cause [2][8], collide_conf [2][2], ped [2][2], expert [2][2],
// speed [6][4], aim [6][2], modes [4], vehicles_behind, clear_none [2][2], speed_hist [2][nbins], clear_hist [2][2][nbins]
constexpr int A_FRAMES = 0, A_PLAN_NONFINITE = 1, A_EXPERT_NONFINITE = 2, A_CAUSE = 3, A_GT_CAUSE = A_CAUSE + 16, A_CONF = A_GT_CAUSE + 16,
              A_PED = A_CONF + 4, A_EXPERT = A_PED + 4, A_SPEED = A_EXPERT + 4, A_AIM = A_SPEED + CMDS * 4, A_MODES = A_AIM + CMDS * 2,
              A_BEHIND = A_MODES + 4, A_CLEAR_NONE = A_BEHIND + 1, A_SPEED_HIST = A_CLEAR_NONE + 4;
constexpr int M_CONSIDERED = 0, M_STATIC = 1, M_HITS = 2, M_NONFINITE = 3;
constexpr __host__ __device__ int words_of(int nbins) { return A_SPEED_HIST + 6 * nbins; }
constexpr int MAX_WORDS = words_of(MAX_BINS);
// a wave's bits: bit kind of a forecast hit, bit 2 + kind of a ground-truth hit (kind 0 static, 1 moving), bit 4 a pedestrian near
constexpr unsigned HIT = 1, GT_HIT = 4, PED_NEAR = 16;
constexpr unsigned long long NONE = ~0ull;                 // no clearance of that kind

struct Args {
    const float *wp, *ego_locs;             // the driven path (ego_cast for commands 4 and 5, else ego_plan), the expert's track
    int num_plan, cmd, bra, aim;
    const float *other_cast, *other_cmds;
    int num_others;
    const float *locs;
    const int *typs;
    int num_objs, nbins;
    double brake_speed, cmd_thresh, dist_static, dist_moving, behind, ego_radius;
    unsigned long long *acc;
};

__device__ __forceinline__ void add(unsigned long long *s_cnt, int word, long long v) { atomicAdd(s_cnt + word, (unsigned long long)v); }

__device__ __forceinline__ long long wave_min(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const long long w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// P(p) of T points: the sum of its T - 1 step quanta; false where a step is not finite
__device__ __forceinline__ bool path(const float *p, int T, int lane, long long &P) {
    long long q = 0;
    bool ok = true;
    if (lane < T - 1) ok = quantum(p + (size_t)(lane + 1) * 2, p + (size_t)lane * 2, q);
    P = wave_sum(q);
    return __ballot(!ok) == 0;
}

// D = min_t q(traj[t], wp[t]); false where a distance is not finite
__device__ __forceinline__ bool clearance(const float *traj, const float *wp, int T, int lane, long long &D) {
    long long q = 0;
    bool ok = true;
    if (lane < T) ok = quantum(traj + (size_t)lane * 2, wp + (size_t)lane * 2, q);
    D = wave_min(lane < T ? q : 0x7fffffffffffffffLL);
    return __ballot(!ok) == 0;
}

// plan_collide's test of one trajectory: kind (0 static, 1 moving) and whether it hits; false where it is not finite
__device__ __forceinline__ bool rule(const Args &a, const float *traj, int lane, long long S, long long L_static, long long L_moving, int &kind,
                                     long long &D, bool &hit) {
    long long P;
    const bool steps = path(traj, a.num_plan, lane, P), dists = clearance(traj, a.wp, a.num_plan, lane, D);
    kind = P < S ? 0 : 1;
    hit = D < (kind == 0 ? L_static : L_moving);
    return steps && dists;
}

__global__ __launch_bounds__(THREADS) void k_eval_drive(Args a) {
    __shared__ unsigned long long s_cnt[MAX_WORDS];     // the workgroup's copy of the accumulator
    __shared__ unsigned long long s_clear[WAVES][2];
    __shared__ unsigned s_bits[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.num_plan, total = words_of(a.nbins);
    const long long S = llrint(a.brake_speed * (double)(T - 1) * EVAL_Q);
    const long long L_static = llrint(a.dist_static * EVAL_Q), L_moving = llrint(a.dist_moving * EVAL_Q);

    // the driven path (every wave: uniform over the workgroup)
    long long P_wp, q_aim;
    const float *target = a.ego_locs + (size_t)(1 + a.aim) * 2;
    const bool steps_ok = path(a.wp, T, lane, P_wp), aim_ok = quantum(a.wp + (size_t)a.aim * 2, target, q_aim);
    if (!steps_ok || !aim_ok) {
        if (tid == 0) {
            atomicAdd(a.acc + A_FRAMES, 1ull);
            atomicAdd(a.acc + A_PLAN_NONFINITE, 1ull);
        }
        return;
    }
    for (int i = tid; i < total; i += THREADS) {
        s_cnt[i] = 0;
        lds_store_fence();
    }
    __syncthreads();

    unsigned bits = 0;                                   // (uniform within a wave, like everything an item yields)
    unsigned long long clear[2] = {NONE, NONE};
    const int modes = CMDS * a.num_others, items = modes + a.num_objs;
    for (int i = wave; i < items; i += WAVES) {
        int kind;
        long long D;
        bool hit;
        if (i < modes) {                                 // mode m of vehicle k
            const int k = i / CMDS, m = i - k * CMDS;
            const float *cast = a.other_cast + (size_t)k * CMDS * T * 2;
            if ((double)cast[1] > a.behind) {            // mode 0's first waypoint speaks for all six
                if (m == 0 && lane == 0) add(s_cnt, A_BEHIND, 1);
                continue;
            }
            if ((double)a.other_cmds[i] < a.cmd_thresh) continue;
            const bool finite = rule(a, cast + (size_t)m * T * 2, lane, S, L_static, L_moving, kind, D, hit);
            if (lane == 0) {
                add(s_cnt, A_MODES + M_CONSIDERED, 1);
                if (!finite) add(s_cnt, A_MODES + M_NONFINITE, 1);
                else {
                    if (kind == 0) add(s_cnt, A_MODES + M_STATIC, 1);
                    if (hit) add(s_cnt, A_MODES + M_HITS, 1);
                }
            }
            if (finite) {
                if (hit) bits |= HIT << kind;
                if ((unsigned long long)D < clear[kind]) clear[kind] = (unsigned long long)D;
            }
        } else {                                         // track g < n
            const int g = i - modes, typ = a.typs[g];
            const float *track = a.locs + (size_t)g * (T + 1) * 2;
            if (typ == 1) {
                const double x = (double)track[0], y = (double)track[1], r = a.ego_radius;
                if (x * x + y * y <= r * r || (double)track[3] > a.behind) continue;        // the ego's own track; behind at frame 1
                if (rule(a, track + 2, lane, S, L_static, L_moving, kind, D, hit) && hit) bits |= GT_HIT << kind;
            } else if (typ == 0) {
                if (clearance(track + 2, a.wp, T, lane, D) && D < L_static) bits |= PED_NEAR;
            }
        }
    }
    if (lane == 0) {
        s_bits[wave] = bits;
        s_clear[wave][0] = clear[0];
        lds_store_fence();
        s_clear[wave][1] = clear[1];
    }

    // the expert (wave 0; thread 0 keeps the results)
    long long P_exp = 0;
    bool exp_ok = false;
    if (wave == 0) exp_ok = path(a.ego_locs + 2, T, lane, P_exp);
    __syncthreads();

    if (tid == 0) {
        for (int w = 0; w < WAVES; ++w) {
            bits |= s_bits[w];
            for (int kind = 0; kind < 2; ++kind)
                if (s_clear[w][kind] < clear[kind]) clear[kind] = s_clear[w][kind];
        }
        const int bra = a.bra, slow = P_wp < S ? 1 : 0, nbins = a.nbins;
        const int fc = (int)(bits & 3u), gt = (int)((bits >> 2) & 3u);
        add(s_cnt, A_FRAMES, 1);
        add(s_cnt, A_CAUSE + bra * 8 + (slow | fc << 1), 1);
        add(s_cnt, A_GT_CAUSE + bra * 8 + (slow | gt << 1), 1);
        add(s_cnt, A_CONF + (gt != 0 ? 2 : 0) + (fc != 0 ? 1 : 0), 1);
        add(s_cnt, A_PED + bra * 2 + ((bits & PED_NEAR) != 0 ? 1 : 0), 1);
        const long long speed_bin = (P_wp / (T - 1)) >> SPEED_SHIFT;
        add(s_cnt, A_SPEED_HIST + bra * nbins + (int)(speed_bin < nbins - 1 ? speed_bin : nbins - 1), 1);
        for (int kind = 0; kind < 2; ++kind) {
            if (clear[kind] == NONE) add(s_cnt, A_CLEAR_NONE + bra * 2 + kind, 1);
            else {
                const unsigned long long bin = clear[kind] >> CLEAR_SHIFT;
                add(s_cnt, A_SPEED_HIST + 2 * nbins + (bra * 2 + kind) * nbins + (int)(bin < (unsigned long long)(nbins - 1) ? bin : nbins - 1), 1);
            }
        }
        if (!exp_ok) add(s_cnt, A_EXPERT_NONFINITE, 1);
        else {
            const double lateral = fabs((double)a.wp[(size_t)a.aim * 2] - (double)target[0]);      // <= the aim distance: finite
            add(s_cnt, A_EXPERT + bra * 2 + (P_exp < S ? 1 : 0), 1);
            add(s_cnt, A_SPEED + a.cmd * 4, 1);
            add(s_cnt, A_SPEED + a.cmd * 4 + 1, P_wp);
            add(s_cnt, A_SPEED + a.cmd * 4 + 2, P_exp);
            add(s_cnt, A_SPEED + a.cmd * 4 + 3, P_wp > P_exp ? P_wp - P_exp : P_exp - P_wp);
            add(s_cnt, A_AIM + a.cmd * 2, q_aim);
            add(s_cnt, A_AIM + a.cmd * 2 + 1, llrint(lateral * EVAL_Q));
        }
    }
    __syncthreads();
    for (int i = tid; i < total; i += THREADS)
        if (s_cnt[i] != 0) atomicAdd(a.acc + i, s_cnt[i]);
}

bool rule_ok(double v, double lowest) { return v >= lowest && v <= MAX_RULE; }      // (false for a NaN)
}  // namespace

extern "C" size_t lav_eval_drive_words(int nbins) { return nbins >= 1 && nbins <= MAX_BINS ? (size_t)words_of(nbins) : 0; }

extern "C" int lav_eval_drive(const float *ego_plan, const float *ego_cast, const float *ego_locs, int num_plan, int cmd, int bra, int aim,
                              const float *other_cast, const float *other_cmds, int num_others, const float *locs, const int *typs, int max_objs,
                              int num_objs, double brake_speed, double cmd_thresh, double dist_static, double dist_moving, double behind,
                              double ego_radius, int nbins, long long *acc, void *stream) {
    static_assert(words_of(64) == 92 + 6 * 64 && MAX_WORDS * 8 + WAVES * 24 <= 64 * 1024, "92 + 6 nbins words, within the static LDS limit");
    LAV_REQUIRE(ego_plan && ego_cast && ego_locs && acc, "lav_eval_drive: null argument");
    LAV_REQUIRE(num_plan >= MIN_PLAN && num_plan <= MAX_PLAN, "lav_eval_drive: %d waypoints (%d .. %d)", num_plan, MIN_PLAN, MAX_PLAN);
    LAV_REQUIRE(cmd >= 0 && cmd < CMDS && (bra == 0 || bra == 1), "lav_eval_drive: command %d (0 .. 5), brake label %d (0 or 1)", cmd, bra);
    LAV_REQUIRE(aim >= 0 && aim < num_plan, "lav_eval_drive: aim point %d of %d waypoints", aim, num_plan);
    LAV_REQUIRE(num_others >= 0 && num_others <= MAX_OTHERS && ((other_cast && other_cmds) || num_others == 0),
                "lav_eval_drive: %d vehicles (0 .. %d, with their two tensors)", num_others, MAX_OTHERS);
    LAV_REQUIRE(max_objs >= 0 && max_objs <= MAX_OBJS && num_objs >= 0 && num_objs <= max_objs && ((locs && typs) || num_objs == 0),
                "lav_eval_drive: %d of %d tracks (at most %d, with their two tensors)", num_objs, max_objs, MAX_OBJS);
    LAV_REQUIRE(nbins >= 1 && nbins <= MAX_BINS, "lav_eval_drive: %d histogram bins (1 .. %d)", nbins, MAX_BINS);
    LAV_REQUIRE(rule_ok(brake_speed, 0) && rule_ok(dist_static, 0) && rule_ok(dist_moving, 0) && rule_ok(ego_radius, 0) &&
                    rule_ok(cmd_thresh, -MAX_RULE) && rule_ok(behind, -MAX_RULE),
                "lav_eval_drive: the rule parameters must be finite, at most 1e6, and speeds, limits and the radius not negative");
    const uintptr_t words = reinterpret_cast<uintptr_t>(ego_plan) | reinterpret_cast<uintptr_t>(ego_cast) | reinterpret_cast<uintptr_t>(ego_locs) |
                            reinterpret_cast<uintptr_t>(other_cast) | reinterpret_cast<uintptr_t>(other_cmds) | reinterpret_cast<uintptr_t>(locs) |
                            reinterpret_cast<uintptr_t>(typs);
    LAV_REQUIRE((words & 3) == 0 && (reinterpret_cast<uintptr_t>(acc) & 7) == 0,
                "lav_eval_drive: float32 / int32 tensors must be 4-byte, the accumulator 8-byte aligned");
    Args a;
    a.wp = cmd == 4 || cmd == 5 ? ego_cast : ego_plan;      // run_step drives the cast on lane changes
    a.ego_locs = ego_locs; a.num_plan = num_plan; a.cmd = cmd; a.bra = bra; a.aim = aim;
    a.other_cast = other_cast; a.other_cmds = other_cmds; a.num_others = num_others;
    a.locs = locs; a.typs = typs; a.num_objs = num_objs; a.nbins = nbins;
    a.brake_speed = brake_speed; a.cmd_thresh = cmd_thresh; a.dist_static = dist_static; a.dist_moving = dist_moving; a.behind = behind;
    a.ego_radius = ego_radius;
    a.acc = reinterpret_cast<unsigned long long *>(acc);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("eval_drive", st);
    hipLaunchKernelGGL(k_eval_drive, dim3(1), dim3(THREADS), 0, st, a);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
