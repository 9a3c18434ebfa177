"""The LiDAR student beside the BEV teacher it was distilled from, on the same frames and the same crops (eval_distill_v2.py).

train_full_v2 freezes a teacher and distils the student from it; three of its four motion losses compare student outputs with teacher
outputs on the same crops.  eval_bev_v2 scores the teacher alone and eval_full_v2 the student the way the agent runs it; this module
puts the two side by side without a random draw: per group of frames the LiDAR trunk makes the student's feature map,
UniPlanner.infer_batch and BEVPlanner.infer_batch run the SAME picks (every vehicle's un-jittered crop at its ground-truth pose, and the
B ego crops), the outputs stay in HBM, and three launches ADD integer counters into three sections of one int64 accumulator that is read
once, at the end: lav_eval_plans on the teacher's outputs, lav_eval_plans on the student's, and lav_eval_distill (lav_amd.ops.eval_distill)
on the pair - the quantities two separate accumulators cannot give, such as which of the two was closer on a frame.
`eval_distill_numpy` below is that kernel's specification and the two agree in every word (tests/test_gpu_eval_distill.py).

The student is scored here on GROUND-TRUTH poses: its others are the recorded vehicles, not its own detections.  The deployed path,
with others taken from detections, is what eval_full_v2.py measures.

The reference has no evaluator: the metric definitions are this project's, and parity with a reference is UNPINNED because there is
nothing to pin it to.  What is pinned: the kernel to this specification, the specification to hand-derived counters
(tests/test_eval_distill_host.py), both infer_batch methods to UniPlanner.forward with its jitters at zero, bit for bit.

Definitions of the `pair` section (DESIGN 4.7k has the reasons), in evaluate_bev's notation.  S = I + 1 stages, I = num_plan_iter: stage
0 is the cast, stage s the s-th refinement of the plan.  q_t = rint(sqrt(dx^2 + dy^2) * 2^20), float64 (eval_common._quanta); a path
with a distance that is not below FAR = 2^32 m (NaN, Inf) is non-finite.  A score gap is rint(|float64(s) - float64(t)| * 2^20), non-finite
where the difference is not below FAR (NaN, Inf; sigmoid scores are four thousand million times smaller).
  frames, bad_cmd    frames seen; frames whose command is outside 0 .. 5, which add to nothing else.
  ego_gap            [stage][mode][items, sum_t q_t, q_{T-1}] of the student's waypoints against the teacher's, all six modes: the
                     distillation losses' quantity on clean data.  ego_gap_nonfinite [stage]: the non-finite (stage, mode) pairs.
  ego_closer         [stage][cmd][student, teacher, tie] at the frame's command: whose sum_t q_t against ego_locs[:, 1:] is the smaller
                     integer.  ego_unjudged [stage]: frames where either arm's is non-finite, which count here instead.
  cmd_agree          [teacher's first maximum of ego_cmds][student's]; a NaN counts as a maximum (np.argmax).
  cmd_gap            [mode][items, sum of the score gaps]; cmd_nonfinite: the non-finite (frame, mode) gaps.
  others             forecasts scored.  oth_nonfinite: forecasts with a non-finite path - either arm against other_locs or student
                     against teacher, in any mode - or a non-finite score gap, which add to nothing else.
  oth_gap            [mode][sum_t q_t, q_{T-1}], the student's forecast against the teacher's.
  oth_closer         [student, teacher, tie] by each arm's own min-mode sum against other_locs (the first minimum); oth_closer_top the
                     same by each arm's own top mode (the first maximum of its other_cmds).
  oth_same_min       forecasts whose min mode is the same in both arms; oth_top_agree [teacher's top mode][student's].
  oth_cmd_gap        [mode]: sums of the score gaps.
Every comparison is between integers and every term an integer before it is added, so the kernel and this file cannot differ by a
rounding and a route's counters depend neither on how its frames are split over launches nor on any order, given the two networks'
outputs; DistillEvaluator.run keeps those independent of the loader's batch, as BevEvaluator.run does.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import evaluate_bev
from .eval_common import FAR, NUM_CMDS, QUANTA, AccLayout, EvaluatorBase, _np, _quanta, _ratio, run_cli, synthetic_batches
from .evaluate_bev import MAX_ITERS, OTHERS, PRECISIONS, PlanLayout, eval_plans_numpy

CLOSER = ("student", "teacher", "tie")
NOTE = ("the student is scored on ground-truth poses (the recorded vehicles' un-jittered crops, the teacher's picks); the deployed path, "
        "with others taken from the student's own detections, is what eval_full_v2.py measures")


def _pair_fields(S):
    return (("frames", ()), ("bad_cmd", ()), ("ego_gap", (S, NUM_CMDS, 3)), ("ego_gap_nonfinite", (S,)), ("ego_closer", (S, NUM_CMDS, 3)),
            ("ego_unjudged", (S,)), ("cmd_agree", (NUM_CMDS, NUM_CMDS)), ("cmd_gap", (NUM_CMDS, 2)), ("cmd_nonfinite", ()), ("others", ()),
            ("oth_nonfinite", ()), ("oth_gap", (NUM_CMDS, 2)), ("oth_closer", (3,)), ("oth_closer_top", (3,)), ("oth_same_min", ()),
            ("oth_top_agree", (NUM_CMDS, NUM_CMDS)), ("oth_cmd_gap", (NUM_CMDS,)))


def _iters(iters):
    if not 1 <= int(iters) <= MAX_ITERS:
        raise ValueError(f"{iters} plan iterations (1 .. {MAX_ITERS})")
    return int(iters)


class PairLayout(AccLayout):
    """lav_eval_distill's accumulator for `iters` plan iterations as named slices, in words of int64 (csrc/eval_distill.hip,
    include/lav_amd.h): 114 + 38 (iters + 1) words."""

    def __init__(self, iters: int):
        self.iters = _iters(iters)
        self.stages = self.iters + 1
        super().__init__(_pair_fields(self.stages))

    @classmethod
    def of(cls, acc) -> "PairLayout":
        stages, rest = divmod(len(acc) - 114, 38)
        if rest or not 1 <= stages - 1 <= MAX_ITERS:
            raise ValueError(f"an accumulator of {len(acc)} words")
        return cls(stages - 1)


class DistillLayout(AccLayout):
    """DistillEvaluator's accumulator: three sections - `teacher` and `student`, a PlanLayout(iters) each (lav_eval_plans on each
    network's outputs), and `pair`, a PairLayout(iters) -, 228 + 112 (iters + 1) words."""

    def __init__(self, iters: int):
        self.iters = _iters(iters)
        self.stages = self.iters + 1
        self.plan, self.pair = PlanLayout(self.iters), PairLayout(self.iters)
        plan = tuple((name, shape) for name, (_, shape) in self.plan.fields.items())
        super().__init__((("teacher", "plan", plan), ("student", "plan", plan), ("pair", "pair", _pair_fields(self.stages))), sectioned=True)

    @classmethod
    def of(cls, acc) -> "DistillLayout":
        stages, rest = divmod(len(acc) - 228, 112)
        if rest or not 1 <= stages - 1 <= MAX_ITERS:
            raise ValueError(f"an accumulator of {len(acc)} words")
        return cls(stages - 1)


def _score_gap(s, t):
    """The gap of two float32 scores in quanta, or None where their difference is not below FAR."""
    with np.errstate(all="ignore"):
        d = abs(np.float64(s) - np.float64(t))
        return int(np.rint(d * float(QUANTA))) if d < FAR else None


def _closer(student: int, teacher: int) -> int:
    return 0 if student < teacher else 1 if teacher < student else 2


def eval_distill_numpy(acc, s_ego_plan, s_ego_cast, s_ego_cmds, t_ego_plan, t_ego_cast, t_ego_cmds, ego_locs, cmds, s_other_cast=None,
                       s_other_cmds=None, t_other_cast=None, t_other_cmds=None, other_locs=None):
    """The specification of lav_amd.ops.eval_distill, same arguments (tensors or arrays; s_* the student's, t_* the teacher's), on the
    host: adds one group's counters to `acc` (int64 array of len(PairLayout(I))) and returns it.  Written to be read: loops over frames,
    stages, forecasts and modes, float64 throughout."""
    f32 = lambda t: _np(t, np.float32)
    s_ego_plan, s_ego_cast, s_ego_cmds, t_ego_plan, t_ego_cast, t_ego_cmds = (f32(t) for t in (s_ego_plan, s_ego_cast, s_ego_cmds, t_ego_plan, t_ego_cast, t_ego_cmds))
    ego_locs, cmds = f32(ego_locs), _np(cmds, np.int32)
    if s_ego_plan.ndim != 5:
        raise ValueError(f"s_ego_plan {s_ego_plan.shape}")
    B, I, _, T, _ = s_ego_plan.shape
    lay = PairLayout(I)
    if not (isinstance(acc, np.ndarray) and acc.dtype == np.int64 and acc.shape == (lay.words,)):
        raise ValueError(f"acc must be an int64 array of {lay.words} words")
    if (B < 1 or not 1 <= T <= 64 or s_ego_plan.shape != (B, I, NUM_CMDS, T, 2) or t_ego_plan.shape != s_ego_plan.shape
            or s_ego_cast.shape != (B, NUM_CMDS, T, 2) or t_ego_cast.shape != s_ego_cast.shape or s_ego_cmds.shape != (B, NUM_CMDS)
            or t_ego_cmds.shape != s_ego_cmds.shape or ego_locs.shape != (B, T + 1, 2) or cmds.shape != (B,)):
        raise ValueError(f"ego_plan {s_ego_plan.shape} / {t_ego_plan.shape}, ego_cast {s_ego_cast.shape} / {t_ego_cast.shape}, ego_cmds "
                         f"{s_ego_cmds.shape} / {t_ego_cmds.shape}, ego_locs {ego_locs.shape}, cmds {cmds.shape}")
    v = lambda name: lay.view(acc, name)
    for b in range(B):
        v("frames")[...] += 1
        cmd = int(cmds[b])
        if not 0 <= cmd < NUM_CMDS:
            v("bad_cmd")[...] += 1
            continue
        for s in range(I + 1):
            student = s_ego_cast[b] if s == 0 else s_ego_plan[b, s - 1]          # (6, T, 2)
            teacher = t_ego_cast[b] if s == 0 else t_ego_plan[b, s - 1]
            for m in range(NUM_CMDS):
                q = _quanta(student[m], teacher[m])
                if q is None:
                    v("ego_gap_nonfinite")[s] += 1
                else:
                    v("ego_gap")[s, m] += (1, int(q.sum()), int(q[-1]))
            qs, qt = _quanta(student[cmd], ego_locs[b, 1:]), _quanta(teacher[cmd], ego_locs[b, 1:])
            if qs is None or qt is None:
                v("ego_unjudged")[s] += 1
            else:
                v("ego_closer")[s, cmd, _closer(int(qs.sum()), int(qt.sum()))] += 1
        v("cmd_agree")[int(np.argmax(t_ego_cmds[b])), int(np.argmax(s_ego_cmds[b]))] += 1          # first maxima; a NaN counts as one
        for m in range(NUM_CMDS):
            g = _score_gap(s_ego_cmds[b, m], t_ego_cmds[b, m])
            if g is None:
                v("cmd_nonfinite")[...] += 1
            else:
                v("cmd_gap")[m] += (1, g)

    given = (s_other_cast, s_other_cmds, t_other_cast, t_other_cmds, other_locs)
    counts = {0 if t is None else len(t) for t in given}
    if len(counts) != 1:
        raise ValueError("the five forecast tensors must have the same number of rows (or all be None / empty)")
    K = counts.pop()
    if K:
        s_other_cast, s_other_cmds, t_other_cast, t_other_cmds, other_locs = (f32(t) for t in given)
        if (s_other_cast.shape != (K, NUM_CMDS, T, 2) or t_other_cast.shape != s_other_cast.shape or s_other_cmds.shape != (K, NUM_CMDS)
                or t_other_cmds.shape != s_other_cmds.shape or other_locs.shape != (K, T, 2)):
            raise ValueError(f"other_cast {s_other_cast.shape} / {t_other_cast.shape}, other_cmds {s_other_cmds.shape} / {t_other_cmds.shape}, "
                             f"other_locs {other_locs.shape}")
    for k in range(K):
        of_s = [_quanta(s_other_cast[k, m], other_locs[k]) for m in range(NUM_CMDS)]
        of_t = [_quanta(t_other_cast[k, m], other_locs[k]) for m in range(NUM_CMDS)]
        gaps = [_quanta(s_other_cast[k, m], t_other_cast[k, m]) for m in range(NUM_CMDS)]
        scores = [_score_gap(s_other_cmds[k, m], t_other_cmds[k, m]) for m in range(NUM_CMDS)]
        if any(x is None for x in of_s + of_t + gaps + scores):
            v("oth_nonfinite")[...] += 1
            continue
        v("others")[...] += 1
        sums_s, sums_t = [int(q.sum()) for q in of_s], [int(q.sum()) for q in of_t]
        best_s, best_t = sums_s.index(min(sums_s)), sums_t.index(min(sums_t))          # the first minimum, each arm its own
        top_s, top_t = int(np.argmax(s_other_cmds[k])), int(np.argmax(t_other_cmds[k]))   # the first maximum; a NaN counts as one
        for m in range(NUM_CMDS):
            v("oth_gap")[m] += (int(gaps[m].sum()), int(gaps[m][-1]))
            v("oth_cmd_gap")[m] += scores[m]
        v("oth_closer")[_closer(sums_s[best_s], sums_t[best_t])] += 1
        v("oth_closer_top")[_closer(sums_s[top_s], sums_t[top_t])] += 1
        if best_s == best_t:
            v("oth_same_min")[...] += 1
        v("oth_top_agree")[top_t, top_s] += 1
    return acc


def _shares(row):
    """[student, teacher, tie] counts -> their shares of the judged items."""
    n = int(np.sum(row))
    return dict(judged=n, **{name: _ratio(int(x), n) for name, x in zip(CLOSER, row)})


def summarise(acc, num_plan: int = 20) -> dict:
    """Metrics from a DistillEvaluator accumulator (array or tensor); a zero denominator gives None, never a NaN.  `teacher` and
    `student` are evaluate_bev.summarise of their sections (per stage ADE / FDE with per-command rows, command accuracy, the others' min
    / top ADE); `pair` has, per stage, the student - teacher gap ADE / FDE per mode (metres between the two networks' waypoints) and the
    closer shares per command, and for the others the gap per mode, the closer shares by min and by top mode, the same-min share, the
    top-mode agreement and the mean score gap."""
    acc = _np(acc, np.int64)
    lay = DistillLayout.of(acc)
    T, S = int(num_plan), lay.stages
    teacher, student = (evaluate_bev.summarise(lay.view(acc, name), T) for name in ("teacher", "student"))
    p = lay.fields(acc, "pair")
    one = lambda name: int(p[name].reshape(-1)[0])

    def gap(rows):                                # rows: (..., 3) [items, sum, final], summed over the leading axes
        n, total, final = (int(x) for x in rows.reshape(-1, 3).sum(axis=0))
        return dict(items=n, ade=_ratio(total, QUANTA * T * n), fde=_ratio(final, QUANTA * n))

    stages = []
    for s in range(S):
        row = gap(p["ego_gap"][s])
        row.update(per_mode=[gap(p["ego_gap"][s, m]) for m in range(NUM_CMDS)], nonfinite=int(p["ego_gap_nonfinite"][s]),
                   closer=dict(_shares(p["ego_closer"][s].sum(axis=0)), unjudged=int(p["ego_unjudged"][s]),
                               per_cmd=[_shares(p["ego_closer"][s, c]) for c in range(NUM_CMDS)]),
                   teacher=dict(ade=teacher["plan"]["all"][s]["ade"], fde=teacher["plan"]["all"][s]["fde"]),
                   student=dict(ade=student["plan"]["all"][s]["ade"], fde=student["plan"]["all"][s]["fde"]))
        stages.append(row)
    agree, cmd_gap = p["cmd_agree"], p["cmd_gap"]
    n, top = one("others"), p["oth_top_agree"]
    pair = dict(frames=one("frames"), bad_cmd=one("bad_cmd"), stages=stages,
                command=dict(agreement=_ratio(int(np.trace(agree)), int(agree.sum())), matrix=agree.tolist(),
                             mean_gap=_ratio(int(cmd_gap[:, 1].sum()), QUANTA * int(cmd_gap[:, 0].sum())),
                             mean_gap_per_mode=[_ratio(int(cmd_gap[m, 1]), QUANTA * int(cmd_gap[m, 0])) for m in range(NUM_CMDS)],
                             nonfinite=one("cmd_nonfinite")),
                others=dict(scored=n, nonfinite=one("oth_nonfinite"),
                            gap_ade_per_mode=[_ratio(int(p["oth_gap"][m, 0]), QUANTA * T * n) for m in range(NUM_CMDS)],
                            gap_fde_per_mode=[_ratio(int(p["oth_gap"][m, 1]), QUANTA * n) for m in range(NUM_CMDS)],
                            gap_ade=_ratio(int(p["oth_gap"][:, 0].sum()), QUANTA * T * n * NUM_CMDS),
                            closer_min=_shares(p["oth_closer"]), closer_top=_shares(p["oth_closer_top"]), same_min=_ratio(one("oth_same_min"), n),
                            top_agreement=_ratio(int(np.trace(top)), n), top_matrix=top.tolist(),
                            mean_score_gap=_ratio(int(p["oth_cmd_gap"].sum()), QUANTA * n * NUM_CMDS),
                            teacher=dict(min_ade=teacher["others"]["min_ade"], top_ade=teacher["others"]["top_ade"]),
                            student=dict(min_ade=student["others"]["min_ade"], top_ade=student["others"]["top_ade"])))
    return dict(frames=pair["frames"], stages=teacher["stages"], teacher=teacher, student=student, pair=pair)


# ------------------------------------------------------------------------------------------------------------ the evaluator
PAIR_ARGS = ("s_ego_plan", "s_ego_cast", "s_ego_cmds", "t_ego_plan", "t_ego_cast", "t_ego_cmds", "ego_locs", "cmds", "s_other_cast", "s_other_cmds",
             "t_other_cast", "t_other_cmds", "other_locs")
_TAKEN = (0, 1, 5, 6, 7, 8, 9, 10, 11, 12)     # of train_lidar's tuple: lidars, num_points, bev, ego_locs, cmds, nxps, bras, locs, oris, typs


class DistillEvaluator(EvaluatorBase):
    """Runs loader batches (train_lidar's tuple) through the student and its teacher and accumulates the metrics of each and of the pair.

        ev = DistillEvaluator(lav)           # a lav_amd.train.LAV of stage "lidar", or (lidar_model, uniplanner)
        ev.run(loader, max_frames=None)      # -> frames evaluated
        ev.counters()                        # the accumulator (DistillLayout: teacher, student, pair), read once

    The teacher is uniplanner.bev_planner - the one the checkpoint was distilled from - unless `teacher` names another.  others:
    "ahead" scores the vehicles that pass filter_cars (what both were trained on), "all" every vehicle.  device "cpu": the three
    specifications on the host (EvaluatorBase).

    run() regroups the loader's frames into runs of `frames_per_forward`, whatever the loader's batch was, as BevEvaluator.run does and
    for its reason: the convolution engines and lav_gru_plan choose their schedules by batch size, which moves the outputs in their last
    bits, so the forward's batch must not be a loader setting if a route's counters are to be the route's.  upload() + batch() run
    whatever batch they are given."""

    def __init__(self, lav_or_modules, precision=None, device=None, others="ahead", frames_per_forward=8, teacher=None):
        if isinstance(lav_or_modules, (tuple, list)):
            lidar_model, uniplanner = lav_or_modules
        else:
            lidar_model, uniplanner = lav_or_modules.lidar_model, lav_or_modules.uniplanner
        if others not in OTHERS:
            raise ValueError(f"others={others!r} (ahead or all)")
        if int(frames_per_forward) < 1:
            raise ValueError(f"frames_per_forward={frames_per_forward}")
        self.student = uniplanner.eval()
        self.teacher = (uniplanner.bev_planner if teacher is None else getattr(teacher, "bev_planner", teacher)).eval()
        if (int(self.teacher.num_plan_iter), int(self.teacher.num_plan)) != (int(uniplanner.num_plan_iter), int(uniplanner.num_plan)):
            raise ValueError("the teacher and the student differ in num_plan_iter or num_plan")
        super().__init__(lidar_model, DistillLayout(int(uniplanner.num_plan_iter)), precision, device)
        self.others = others
        self.group = int(frames_per_forward)
        self.num_plan = int(uniplanner.num_plan)
        self.frames = 0
        self._batch = None

    def upload(self, batch, limit=None):
        """One loader batch (train_lidar's tuple: lidars, num_points, heatmaps, sizemaps, orimaps, bev, ego_locs, cmds, nxps, bras, locs,
        oris, typs, num_objs), its first `limit` frames, uploaded once.  The detection targets are not read."""
        lidars, num_points, bev, ego_locs, cmds, nxps, bras, locs, oris, typs = [torch.as_tensor(batch[i])[:limit] for i in _TAKEN]
        d = self.model_device
        self._batch = dict(lidars=lidars.to(d, torch.float32), num_points=[int(n) for n in num_points.tolist()], bev=bev.to(d).float(),
                           ego_locs=ego_locs.to(d, torch.float32).contiguous(), cmds=cmds.to(d, torch.int32).contiguous(),
                           nxps=nxps.to(d, torch.float32), bras=(bras != 0).to(torch.uint8).to(d).contiguous(), locs=locs.to(d, torch.float32),
                           oris=oris.to(d, torch.float32), typs=typs.to(d))
        return int(self._batch["cmds"].shape[0])

    def infer(self):
        """The uploaded batch through the LiDAR trunk and both infer_batch methods, on the same picks, at the evaluator's arithmetic:
        (student, teacher), two BatchInference."""
        from .. import ops
        from .evaluate_camera import trunk_arithmetic
        b = self._batch
        poses = (b["ego_locs"], b["locs"], b["oris"], b["nxps"], b["typs"])
        with ops.precision(self.code):
            features = self.model(b["lidars"], b["num_points"])[0]
            student = self.student.infer_batch(features, *poses, others=self.others)
            teacher = self.teacher.infer_batch(b["bev"], *poses, others=self.others)
        self.in_force.add("student " + trunk_arithmetic(self.student.lidar_conv_emb[0], self.code))
        self.in_force.add("teacher " + trunk_arithmetic(self.teacher.bev_conv_emb[0], self.code))
        return student, teacher

    @torch.no_grad()
    def batch(self):
        """The uploaded batch: the forwards, then the three metrics launches."""
        b = self._batch
        student, teacher = self.infer()
        c = lambda t: t.contiguous()
        for section, out in (("teacher", teacher), ("student", student)):
            self._add("eval_plans", eval_plans_numpy, section, c(out.ego_plan), c(out.ego_cast), c(out.ego_cmds), b["ego_locs"], b["cmds"], b["bras"],
                      c(out.other_cast), c(out.other_cmds), c(out.other_locs))
        self._add("eval_distill", eval_distill_numpy, "pair", c(student.ego_plan), c(student.ego_cast), c(student.ego_cmds), c(teacher.ego_plan),
                  c(teacher.ego_cast), c(teacher.ego_cmds), b["ego_locs"], b["cmds"], c(student.other_cast), c(student.other_cmds),
                  c(teacher.other_cast), c(teacher.other_cmds), c(teacher.other_locs))
        self.frames += int(b["cmds"].shape[0])

    def _groups(self, batches, budget):
        """The frames of `batches`, at most `budget` of them, in order and in runs of self.group (the last one may be shorter), as
        train_lidar's tuples whose unread entries are None."""
        held = None
        for batch in batches:
            if budget is not None and budget <= 0:
                break
            part = [torch.as_tensor(batch[i])[:budget] for i in _TAKEN]
            if budget is not None:
                budget -= int(part[4].shape[0])
            if held is not None and held[0].shape[1] != part[0].shape[1]:          # clouds padded to different lengths
                n = max(held[0].shape[1], part[0].shape[1])
                pad = lambda t: torch.nn.functional.pad(t, (0, 0, 0, n - t.shape[1]))
                held[0], part[0] = pad(held[0]), pad(part[0])
            held = part if held is None else [torch.cat([h, p]) for h, p in zip(held, part)]
            while held[4].shape[0] >= self.group:
                yield self._as_batch([h[:self.group] for h in held])
                held = [h[self.group:] for h in held]
        if held is not None and held[4].shape[0]:
            yield self._as_batch(held)

    @staticmethod
    def _as_batch(taken):
        batch = [None] * 14
        for i, t in zip(_TAKEN, taken):
            batch[i] = t
        return batch

    def run(self, batches, max_frames=None) -> int:
        for group in self._groups(batches, None if max_frames is None else max_frames - self.frames):
            self.upload(group)
            self.batch()
        return self.frames


# ------------------------------------------------------------------------------------------------------------ command line
def _build(args, cfg, device):
    from .lav import LAV
    ck = {k: torch.load(getattr(args, k), map_location="cpu") for k in ("lidar", "uniplanner") if getattr(args, k)}
    lav = LAV(cfg, device, what="lidar", checkpoints=ck, distributed=False)
    lav.student.eval()
    if args.bev:           # another teacher than the one the uniplanner checkpoint carries
        if not os.path.isfile(args.bev):
            raise SystemExit(f"--bev {args.bev}: no such file (a bev_*.th teacher checkpoint)")
        lav.bev_planner.load_state_dict(torch.load(args.bev, map_location="cpu"))
        lav.bev_planner.eval()
    return lav


def _batches(args, cfg):
    from .evaluate import held_out_frames
    from .synthetic import synthetic_lidar_batch
    if args.synthetic:
        return synthetic_batches(synthetic_lidar_batch, args.frames, args.batch_size, args.seed, max_points=args.max_points or cfg.max_lidar_points,
                                 num_plan=cfg.num_plan)
    return held_out_frames(args.config_path, args.data_dir, args.seed)


TOOL = dict(
    name="eval_distill_v2", about="the LiDAR student beside the BEV teacher it was distilled from, on the same held-out frames and crops",
    unit="frames", checkpoints=dict(lidar="lidar_model_dir", uniplanner="uniplanner_dir"), precisions=PRECISIONS, batch_size=8, frames=8, synthetic="synthetic_lidar_batch samples",
    epilog=NOTE,
    help=dict(batch_size="loader batch; the forwards and the metrics launches take 8 frames at a time whatever it is, so that it cannot move "
                         "the counters"),
    flags=[("--bev", dict(default=None, help="bev_*.th: a teacher to put beside the student INSTEAD of the one its uniplanner checkpoint carries "
                                             "(default: that one, the teacher it was distilled from)")),
           ("--others", dict(default="ahead", choices=OTHERS,
                             help="which vehicles' forecasts are scored: those ahead of the ego (what both were trained on) or all")),
           ("--max-points", dict(type=int, default=None, help="--synthetic: points per cloud (default: the config's max_lidar_points)"))],
    build=_build, batches=_batches, make_evaluator=lambda lav, name, args: DistillEvaluator(lav, precision=name, others=args.others),
    line=lambda ev, acc, args, cfg: dict(others=args.others, teacher="--bev " + args.bev if args.bev else "the uniplanner checkpoint's", note=NOTE,
                                         summary=summarise(acc, cfg.num_plan)),
    contrasts=(("student", "teacher"),),          # (--bootstrap: the paired difference of the two sections' metrics)
    keys=("what", "precision", "asked", "others", "teacher", "note", "data", "batch_size", "frames_per_s", "summary", "counters"))


def main(argv=None):
    """eval_distill_v2.py: one JSON line per precision, with the arithmetic that was in force (eval_common.run_cli)."""
    return run_cli(TOOL, argv)


if __name__ == "__main__":
    main()
