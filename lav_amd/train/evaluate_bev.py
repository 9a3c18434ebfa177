"""Held-out metrics of the privileged BEV teacher, bev_{epoch}.th (eval_bev_v2.py).

train_bev_v2 prints L1 losses on jittered, randomly sub-sampled training batches; train_full_v2 then freezes the teacher it is given and
distils the student from it, so a poor choice of epoch costs a whole student run.  This module measures a teacher on routes it never
trained on, without a random draw: BEVPlanner.infer_batch runs a loader batch - every vehicle's forecast from its un-jittered crop, the
ego's cast, command scores and every refinement of its plan -, the outputs stay in HBM, and ONE launch per batch of frames (lav_eval_plans:
lav_amd.ops.eval_plans) ADDS integer counters into an int64 accumulator that is read once, at the end.  `eval_plans_numpy` below is that
kernel's specification and the two agree in every word (tests/test_gpu_eval_bev.py).

The reference has no evaluator: the metric definitions are this project's, and parity with a reference is UNPINNED because there is
nothing to pin it to.  What is pinned: the kernel to this specification, the specification to hand-derived counters
(tests/test_eval_bev_host.py), infer_batch to BEVPlanner.forward with its jitters at zero, bit for bit.

Definitions (DESIGN 4.7i has the reasons).  S = I + 1 stages, I = num_plan_iter: stage 0 is the cast at the frame's command, stage s the
s-th refinement of the plan at the frame's command.  q_t = rint(sqrt(dx^2 + dy^2) * 2^20), float64 (eval_common._quanta).
  frames, bad_cmd   frames seen; frames whose command is outside 0 .. 5, which add to nothing else.
  plan              [bra != 0][stage][cmd][frames, sum_t q_t, q_{T-1}] against ego_locs[:, 1:].
  plan_nonfinite    [stage]: a stage with a distance that is not below 2^32 m (NaN, Inf) counts here and not in `plan`; the stages of a
                    frame are judged independently.
  cmd_conf          [cmd][first maximum of ego_cmds; a NaN counts as a maximum, as in evaluate.eval_frame_numpy].
  others            forecasts scored.  oth_nonfinite: forecasts with a non-finite distance in any mode, which add to nothing else.
  oth               sums over the scored forecasts of: the min mode's sum_t q_t, the top mode's, the top mode's q_{T-1}, the min mode's
                    q_{T-1}.  The min mode has the smallest sum_t q_t against other_locs (the first minimum), the top mode is the first
                    maximum of other_cmds.  other_locs is the vehicle's future in ITS OWN frame, what the training loss compares with.
  oth_min_mode, oth_top_mode   histograms of the two; oth_top_is_min: forecasts whose top mode is the min mode.
Every term is an integer before it is added, so a route's counters depend neither on how its frames are split over launches nor on
any order, given the teacher's outputs; BevEvaluator.run keeps those independent of the loader's batch (its docstring).
"""
from __future__ import annotations

import numpy as np
import torch

from .eval_common import FAR, NUM_CMDS, QUANTA, AccLayout, EvaluatorBase, SeededFrames, _np, _quanta, _ratio, run_cli, synthetic_batches  # noqa: F401  (FAR: the rule's other constant, for readers)

MAX_ITERS = 8
OTHERS = ("ahead", "all")


class PlanLayout(AccLayout):
    """The accumulator's named slices, in words of int64: lav_eval_plans' layout for `iters` plan iterations (csrc/eval_plans.hip,
    include/lav_amd.h), 57 + 37 (iters + 1) words.  plan [bra][stage][cmd][frames, sum, final]; cmd_conf [cmd][predicted]; oth [min sum,
    top sum, top final, min final]."""

    def __init__(self, iters: int):
        if not 1 <= int(iters) <= MAX_ITERS:
            raise ValueError(f"{iters} plan iterations (1 .. {MAX_ITERS})")
        self.iters = int(iters)
        self.stages = S = self.iters + 1
        super().__init__((("frames", ()), ("bad_cmd", ()), ("plan", (2, S, NUM_CMDS, 3)), ("plan_nonfinite", (S,)), ("cmd_conf", (NUM_CMDS, NUM_CMDS)),
                          ("others", ()), ("oth_nonfinite", ()), ("oth", (4,)), ("oth_min_mode", (NUM_CMDS,)), ("oth_top_mode", (NUM_CMDS,)),
                          ("oth_top_is_min", ())))

    @classmethod
    def of(cls, acc) -> "PlanLayout":
        stages, rest = divmod(len(acc) - 57, 37)
        if rest or not 1 <= stages - 1 <= MAX_ITERS:
            raise ValueError(f"an accumulator of {len(acc)} words")
        return cls(stages - 1)


def eval_plans_numpy(acc, ego_plan, ego_cast, ego_cmds, ego_locs, cmds, bras, other_cast=None, other_cmds=None, other_locs=None):
    """The specification of lav_amd.ops.eval_plans, same arguments (tensors or arrays), on the host: adds one batch's counters to `acc`
    (int64 array of len(PlanLayout(I))) and returns it.  Written to be read: loops over frames, stages, forecasts and modes, float64
    throughout."""
    ego_plan, ego_cast, ego_cmds, ego_locs = (_np(t, np.float32) for t in (ego_plan, ego_cast, ego_cmds, ego_locs))
    cmds, bras = _np(cmds, np.int32), _np(bras, np.uint8)
    if ego_plan.ndim != 5:
        raise ValueError(f"ego_plan {ego_plan.shape}")
    B, I, _, T, _ = ego_plan.shape
    lay = PlanLayout(I)
    if not (isinstance(acc, np.ndarray) and acc.dtype == np.int64 and acc.shape == (lay.words,)):
        raise ValueError(f"acc must be an int64 array of {lay.words} words")
    if (B < 1 or not 1 <= T <= 64 or ego_plan.shape != (B, I, NUM_CMDS, T, 2) or ego_cast.shape != (B, NUM_CMDS, T, 2) or ego_cmds.shape != (B, NUM_CMDS)
            or ego_locs.shape != (B, T + 1, 2) or cmds.shape != (B,) or bras.shape != (B,)):
        raise ValueError(f"ego_plan {ego_plan.shape}, ego_cast {ego_cast.shape}, ego_cmds {ego_cmds.shape}, ego_locs {ego_locs.shape}, "
                         f"cmds {cmds.shape}, bras {bras.shape}")
    plan, plan_nonfinite, cmd_conf = lay.view(acc, "plan"), lay.view(acc, "plan_nonfinite"), lay.view(acc, "cmd_conf")
    for b in range(B):
        lay.view(acc, "frames")[...] += 1
        cmd = int(cmds[b])
        if not 0 <= cmd < NUM_CMDS:
            lay.view(acc, "bad_cmd")[...] += 1
            continue
        bra = 1 if bras[b] != 0 else 0
        for s in range(I + 1):
            points = ego_cast[b, cmd] if s == 0 else ego_plan[b, s - 1, cmd]
            q = _quanta(points, ego_locs[b, 1:])
            if q is None:
                plan_nonfinite[s] += 1
            else:
                plan[bra, s, cmd] += (1, int(q.sum()), int(q[-1]))
        cmd_conf[cmd, int(np.argmax(ego_cmds[b]))] += 1          # the first maximum; a NaN counts as one

    K = 0 if other_cast is None else len(other_cast)
    if K:
        other_cast, other_cmds, other_locs = _np(other_cast, np.float32), _np(other_cmds, np.float32), _np(other_locs, np.float32)
        if other_cast.shape != (K, NUM_CMDS, T, 2) or other_cmds.shape != (K, NUM_CMDS) or other_locs.shape != (K, T, 2):
            raise ValueError(f"other_cast {other_cast.shape}, other_cmds {other_cmds.shape}, other_locs {other_locs.shape}")
    oth, min_mode, top_mode = lay.view(acc, "oth"), lay.view(acc, "oth_min_mode"), lay.view(acc, "oth_top_mode")
    for k in range(K):
        per_mode = [_quanta(other_cast[k, m], other_locs[k]) for m in range(NUM_CMDS)]
        if any(p is None for p in per_mode):
            lay.view(acc, "oth_nonfinite")[...] += 1
            continue
        sums = [int(p.sum()) for p in per_mode]
        best = sums.index(min(sums))                            # the first minimum
        top = int(np.argmax(other_cmds[k]))                     # the first maximum; a NaN counts as one
        lay.view(acc, "others")[...] += 1
        oth += (sums[best], sums[top], int(per_mode[top][-1]), int(per_mode[best][-1]))
        min_mode[best] += 1
        top_mode[top] += 1
        if top == best:
            lay.view(acc, "oth_top_is_min")[...] += 1
    return acc


def summarise(acc, num_plan: int = 20) -> dict:
    """Metrics from an accumulator (array or tensor); a zero denominator gives None, never a NaN.  Distances in metres: sum of q /
    (2^20 * num_plan * count) for the averages (ADE), final q / (2^20 * count) for the final displacement (FDE).  `gain` of a stage is
    its ADE minus the ADE of the stage before (negative: that refinement step improved on it)."""
    acc = _np(acc, np.int64)
    lay = PlanLayout.of(acc)
    v = lambda name: lay.view(acc, name)
    one = lambda name: int(v(name).reshape(-1)[0])
    T, S = int(num_plan), lay.stages
    plan = v("plan")

    def stage_metrics(rows):                      # rows: (..., 3) counters that are summed over their leading axes
        n, total, final = (int(x) for x in rows.reshape(-1, 3).sum(axis=0))
        return dict(frames=n, ade=_ratio(total, QUANTA * T * n), fde=_ratio(final, QUANTA * n))

    def stages_of(block):                         # block: (S, 6, 3) or (2, S, 6, 3) moved to (S, ..., 3)
        out = []
        for s in range(S):
            m = stage_metrics(block[s])
            m["per_cmd"] = [stage_metrics(block[s][..., k, :]) for k in range(NUM_CMDS)]
            before = out[-1]["ade"] if out else None
            m["gain"] = None if s == 0 or m["ade"] is None or before is None else m["ade"] - before
            out.append(m)
        return out

    conf = v("cmd_conf")
    seen = int(conf.sum())
    n = one("others")
    out = dict(frames=one("frames"), bad_cmd=one("bad_cmd"), stages=["cast"] + [f"plan_{i}" for i in range(lay.iters)],
               frames_per_cmd=[int(x) for x in conf.sum(axis=1)],
               plan=dict(all=stages_of(np.moveaxis(plan, 0, 1)), driving=stages_of(plan[0]), braking=stages_of(plan[1]),
                         nonfinite=[int(x) for x in v("plan_nonfinite")]),
               command=dict(accuracy=_ratio(int(np.trace(conf)), seen), per_cmd=[_ratio(int(conf[k, k]), int(conf[k].sum())) for k in range(NUM_CMDS)],
                            confusion=conf.tolist()))
    oth = v("oth")
    out["others"] = dict(scored=n, nonfinite=one("oth_nonfinite"), min_ade=_ratio(oth[0], QUANTA * T * n), top_ade=_ratio(oth[1], QUANTA * T * n),
                         top_fde=_ratio(oth[2], QUANTA * n), min_fde=_ratio(oth[3], QUANTA * n), min_mode=v("oth_min_mode").tolist(),
                         top_mode=v("oth_top_mode").tolist(), top_is_min=_ratio(one("oth_top_is_min"), n))
    return out


# ------------------------------------------------------------------------------------------------------------ the evaluator
PRECISIONS = ("f16x3", "bf16x6", "f32")


class BevEvaluator(EvaluatorBase):
    """Runs loader batches (train_bev's tuple) through the teacher and accumulates their metrics, one launch per batch.

        ev = BevEvaluator(lav)               # a lav_amd.train.LAV of stage "bev", or a BEVPlanner
        ev.run(loader, max_frames=None)      # -> frames evaluated
        ev.counters()                        # the accumulator, read once

    others: "ahead" scores the vehicles that pass filter_cars (what the teacher was trained on), "all" every vehicle.  device "cpu":
    eval_plans_numpy on the host (EvaluatorBase).

    run() regroups the loader's frames into runs of `frames_per_forward`, whatever the loader's batch was: the convolution engines and
    lav_gru_plan choose their schedules (split-K, which plan kernel) by batch size, which moves the teacher's outputs in their last
    bits (up to 2.3e-5 m between four frames together and each alone), so the forward's batch must not be a loader
    setting if a route's counters are to be the route's.  upload() + batch() run whatever batch they are given."""

    def __init__(self, bev_planner, precision=None, device=None, others="ahead", frames_per_forward=8):
        model = getattr(bev_planner, "bev_planner", bev_planner)
        if others not in OTHERS:
            raise ValueError(f"others={others!r} (ahead or all)")
        if int(frames_per_forward) < 1:
            raise ValueError(f"frames_per_forward={frames_per_forward}")
        super().__init__(model, PlanLayout(int(model.num_plan_iter)), precision, device)
        self.others = others
        self.group = int(frames_per_forward)
        self.num_plan = int(model.num_plan)
        self.frames = 0
        self._batch = None

    def upload(self, batch, limit=None):
        """One loader batch (bev, ego_locs, cmds, nxps, bras, locs, oris, typs, num_objs), its first `limit` frames, uploaded once."""
        bev, ego_locs, cmds, nxps, bras, locs, oris, typs = [torch.as_tensor(t)[:limit] for t in batch[:8]]
        d = self.model_device
        self._batch = dict(bev=bev.to(d).float(), ego_locs=ego_locs.to(d, torch.float32).contiguous(), cmds=cmds.to(d, torch.int32).contiguous(),
                           nxps=nxps.to(d, torch.float32), bras=(bras != 0).to(torch.uint8).to(d).contiguous(), locs=locs.to(d, torch.float32),
                           oris=oris.to(d, torch.float32), typs=typs.to(d))
        return int(self._batch["cmds"].shape[0])

    def infer(self):
        """BEVPlanner.infer_batch over the uploaded batch at the evaluator's arithmetic."""
        from .. import ops
        from .evaluate_camera import trunk_arithmetic
        b = self._batch
        with ops.precision(self.code):
            out = self.model.infer_batch(b["bev"], b["ego_locs"], b["locs"], b["oris"], b["nxps"], b["typs"], others=self.others)
        self.in_force.add(trunk_arithmetic(self.model.bev_conv_emb[0], self.code))
        return out

    @torch.no_grad()
    def batch(self):
        """The uploaded batch: the teacher's forward, then the metrics launch."""
        b, out = self._batch, self.infer()
        args = (out.ego_plan.contiguous(), out.ego_cast.contiguous(), out.ego_cmds.contiguous(), b["ego_locs"], b["cmds"], b["bras"],
                out.other_cast.contiguous(), out.other_cmds.contiguous(), out.other_locs.contiguous())
        self._add("eval_plans", eval_plans_numpy, None, *args)
        self.frames += int(b["cmds"].shape[0])

    def _groups(self, batches, budget):
        """The frames of `batches`, at most `budget` of them, in order and in runs of self.group (the last one may be shorter)."""
        held = None
        for batch in batches:
            if budget is not None and budget <= 0:
                break
            part = [torch.as_tensor(t)[:budget] for t in batch[:8]]
            if budget is not None:
                budget -= int(part[2].shape[0])
            held = part if held is None else [torch.cat([h, p]) for h, p in zip(held, part)]
            while held[2].shape[0] >= self.group:
                yield [h[:self.group] for h in held]
                held = [h[self.group:] for h in held]
        if held is not None and held[2].shape[0]:
            yield held

    def run(self, batches, max_frames=None) -> int:
        for group in self._groups(batches, None if max_frames is None else max_frames - self.frames):
            self.upload(group)
            self.batch()
        return self.frames


# ------------------------------------------------------------------------------------------------------------ command line
def held_out_bev_frames(config_path, data_dir=None, seed=2021):
    """The 'temporal_bev' loader's dataset over `data_dir` (default: the config's) with both of its jitters at 0, seeded per sample."""
    from ..data.datasets import TemporalBEVDataset
    ds = TemporalBEVDataset(config_path, seed=seed, overrides=dict(data_dir=data_dir) if data_dir else None)
    ds.x_jitter = ds.angle_jitter = 0
    return SeededFrames(ds, seed)


def _build(args, cfg, device):
    from .lav import LAV
    return LAV(cfg, device, what="bev", checkpoints={"bev": torch.load(args.bev, map_location="cpu")} if args.bev else {},
               distributed=False)       # (an evaluation is one process's own: no collective, also inside a trainer's process group)


def _batches(args, cfg):
    from .synthetic import synthetic_bev_batch
    if args.synthetic:
        return synthetic_batches(synthetic_bev_batch, args.frames, args.batch_size, args.seed, num_plan=cfg.num_plan)
    return held_out_bev_frames(args.config_path, args.data_dir, args.seed)


TOOL = dict(
    name="eval_bev_v2", about="held-out metrics of a privileged BEV teacher checkpoint (bev_*.th) on recorded routes", unit="frames",
    checkpoints=dict(bev="bev_model_dir"), precisions=PRECISIONS, batch_size=8, frames=8, synthetic="synthetic_bev_batch samples",
    help=dict(batch_size="loader batch; the teacher's forward and the metrics launch take 8 frames at a time whatever it is, so that it cannot "
                         "move the counters"),
    flags=[("--others", dict(default="ahead", choices=OTHERS,
                             help="which vehicles' forecasts are scored: those ahead of the ego (what the teacher was trained on) or all"))],
    build=_build, batches=_batches, make_evaluator=lambda lav, name, args: BevEvaluator(lav, precision=name, others=args.others),
    line=lambda ev, acc, args, cfg: dict(others=args.others, summary=summarise(acc, cfg.num_plan)),
    keys=("what", "precision", "asked", "others", "data", "batch_size", "frames_per_s", "summary", "counters"))


def main(argv=None):
    """eval_bev_v2.py: one JSON line per precision, with the arithmetic that was in force (eval_common.run_cli)."""
    return run_cli(TOOL, argv)


if __name__ == "__main__":
    main()
