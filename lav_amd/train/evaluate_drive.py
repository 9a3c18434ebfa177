"""Open-loop evaluation of the agent's rule layer on recorded routes (eval_drive_v2.py).

eval_full_v2 measures what the LiDAR student and the planner output; this module measures what LAVAgent does with those outputs
between InferModel.forward and VehicleControl: the brake decision of plan_collide (a likely forecast comes close to the driven path)
and of pid_control (the desired speed is below brake_speed), and the two inputs of the PIDs, desired speed and aim point, against the
expert's brake label `bra` and the expert's and the actors' recorded futures.  A frame runs exactly as Evaluator.frame runs it; its
counters are ADDED to one int64 accumulator in HBM by one launch (lav_eval_drive, lav_amd.ops.eval_drive).  `eval_drive_numpy` below
is that kernel's specification and the two agree in every word (tests/test_gpu_eval_drive.py).

Not evaluated: the camera brake net (pred_bra > 0.1; the 'temporal_lidar_painted' loader carries no images, eval_bra_v2 covers that
net) and the PID dynamics (throttle and steer need a speed history).  What is measured is the LiDAR path's share of the decision.

The reference tuned these rules in closed-loop CARLA and has no evaluator: the definitions are this project's, parity
with a reference is UNPINNED.  What is pinned: the kernel to this specification, the specification to hand-derived counters, and the
restated rules to LAVAgent.plan_collide and LAVAgent.pid_control themselves on random scenes (tests/test_eval_drive_host.py).

Definitions.  q(a, b) = rint(|a - b| * 2^20) in float64 from the float32 inputs (eval_common._quanta), None where the distance is not
below 2^32 m.  P(p) = sum over t < T - 1 of q(p[t + 1], p[t]): the path length in quanta.  S = rint(float64(brake_speed) * (T - 1) *
2^20), L(x) = rint(float64(x) * 2^20); slow(p) = P(p) < S, which is pid_control's `mean step < brake_speed` without the division.
  driven path   wp = ego_cast for cmd 4 and 5 (run_step's lane-change substitution), else ego_plan.  A step of wp or its aim quantum
                q(wp[a], ego_locs[1 + a]), a = aim_point[cmd], that is not finite: plan_nonfinite, and the frame adds nothing else
                but `frames` (the agent outputs zero controls; an aim TARGET that is not finite lands here too).
  forecast rule plan_collide, with its quirks kept: (1) a vehicle is "behind" by mode 0's first waypoint, y > behind, for all six of
                its modes; (2) a mode is dropped when float64(score) < cmd_thresh, so a NaN score is considered; (3) the comparison
                with the limit is strict; (4) static or moving is the forecast's own mean step against brake_speed, the ego's
                threshold.  A considered mode with a step or a distance to wp that is not finite counts in modes[nonfinite] and cannot
                hit; otherwise static = P(traj) < S, D = min_t q(traj[t], wp[t]), hit = D < L(dist_static if static else
                dist_moving).  Per frame: the bits collide_static and collide_moving, and the clearances C_static and C_moving (the
                least D over the finite considered modes of that kind, or none).
  ground truth  the same rule on "perfect forecasts": the tracks g < n with typs[g] == 1 whose frame-0 position is not within
                ego_radius of the origin (dx^2 + dy^2 <= r^2: the ego's own track, others_from_detections' rule) and whose
                locs[g, 1, 1] is not > behind; traj = locs[g, 1:], no score.  Pedestrians (typs[g] == 0, g < n) are near when
                min_t q(locs[g, 1 + t], wp[t]) < L(dist_static); a pedestrian with a distance that is not finite is not near.
  expert        slow(ego_locs[1:]).  An expert path with a step that is not finite counts in expert_nonfinite and the frame skips
                expert, speed and aim.
  speed, aim    per command: frames, P(wp), P(expert), |P(wp) - P(expert)|; q(wp[a], ego_locs[1 + a]) and rint(|dx| * 2^20) of it.
  histograms    speed_hist[bra][min(nbins - 1, (P(wp) // (T - 1)) >> 14)]: 1/64 m per step; clear_hist[bra][kind][min(nbins - 1,
                C_kind >> 17)]: 1/8 m; clear_none[bra][kind] where there is no C_kind.  summarise() sweeps them for other thresholds.
Every term is an integer before it is added, so the sums do not depend on the order of frames.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from .eval_common import NUM_CMDS, QUANTA, AccLayout, _np, _quanta, _ratio, run_cli
from .evaluate import PRECISIONS, Evaluator, _batches, _build

NBINS = 64
MAX_PLAN, MAX_OTHERS, MAX_OBJS = 64, 64, 64
SPEED_SHIFT, CLEAR_SHIFT = 14, 17          # 2^20 >> 14 = 64 speed bins per m/step, 2^20 >> 17 = 8 clearance bins per metre
STATIC, MOVING = 0, 1                      # the kinds of a forecast: clear_none / clear_hist's index, bit 1 + kind of a cause
M_CONSIDERED, M_STATIC, M_HITS, M_NONFINITE = range(4)


@dataclasses.dataclass(frozen=True)
class DriveRules:
    """The hand-tuned constants of LAVAgent's rule layer (lav_agent.DEFAULT_CONFIG, plan_collide's defaults; 4 pixels per metre)."""
    brake_speed: float = 0.2
    cmd_thresh: float = 0.2
    dist_static: float = 1.0
    dist_moving: float = 2.5
    behind: float = 2.0                    # 0.5 * pixels_per_meter, compared with metres: plan_collide's own units
    aim_point: tuple = (4, 4, 4, 3, 6, 6)
    ego_radius: float = 1.0                # 4 px / pixels_per_meter

    def __post_init__(self):
        object.__setattr__(self, "aim_point", tuple(int(a) for a in self.aim_point))
        numbers = [float(getattr(self, k)) for k in ("brake_speed", "cmd_thresh", "dist_static", "dist_moving", "behind", "ego_radius")]
        if not all(np.isfinite(numbers)) or min(self.brake_speed, self.dist_static, self.dist_moving, self.ego_radius) < 0 or max(abs(x) for x in numbers) > 1e6:
            raise ValueError(f"{self}: the rule parameters must be finite, at most 1e6, and speeds, limits and the radius not negative")
        if len(self.aim_point) != NUM_CMDS or min(self.aim_point) < 0:
            raise ValueError(f"aim_point {self.aim_point}: one waypoint index per command")

    @classmethod
    def from_config(cls, config: dict, **given) -> "DriveRules":
        """The rules an agent configured by `config` (DEFAULT_CONFIG's keys; missing ones at their defaults) drives with; `given`
        overrides."""
        from ..lav_agent import DEFAULT_CONFIG
        c = {**DEFAULT_CONFIG, **(config or {})}
        ppm = float(c["pixels_per_meter"])
        kw = dict(brake_speed=float(c["brake_speed"]), cmd_thresh=float(c["cmd_thresh"]), aim_point=tuple(c["aim_point"]), behind=0.5 * ppm,
                  ego_radius=4.0 / ppm)
        kw.update({k: v for k, v in given.items() if v is not None})
        return cls(**kw)

    def named(self) -> dict:
        return {k: list(v) if isinstance(v, tuple) else v for k, v in dataclasses.asdict(self).items()}


class DriveLayout(AccLayout):
    """The accumulator's named slices, in words of int64: lav_eval_drive's layout (csrc/eval_drive.hip, include/lav_amd.h), 92 + 6 nbins
    words.  cause / gt_cause [bra][slow | collide_static << 1 | collide_moving << 2]; collide_conf [any gt hit][any forecast hit];
    ped [bra][near]; expert [bra][slow]; speed [cmd][frames, P(wp), P(expert), |difference|]; aim [cmd][aim, lateral]; modes
    [considered, static, hits, nonfinite]; clear_none [bra][kind]; speed_hist [bra][bin]; clear_hist [bra][kind][bin]."""
    FIELDS = (("frames", ()), ("plan_nonfinite", ()), ("expert_nonfinite", ()), ("cause", (2, 8)), ("gt_cause", (2, 8)), ("collide_conf", (2, 2)),
              ("ped", (2, 2)), ("expert", (2, 2)), ("speed", (NUM_CMDS, 4)), ("aim", (NUM_CMDS, 2)), ("modes", (4,)), ("vehicles_behind", ()),
              ("clear_none", (2, 2)))

    def __init__(self, nbins: int = NBINS):
        if not 1 <= int(nbins) <= 1024:
            raise ValueError(f"{nbins} histogram bins (1 .. 1024)")
        self.nbins = int(nbins)
        super().__init__(self.FIELDS + (("speed_hist", (2, self.nbins)), ("clear_hist", (2, 2, self.nbins))))

    @classmethod
    def of(cls, acc) -> "DriveLayout":
        nbins, rest = divmod(len(acc) - (cls(1).words - 6), 6)
        if rest or not 1 <= nbins <= 1024:
            raise ValueError(f"an accumulator of {len(acc)} words")
        return cls(nbins)


def _path(p):
    """P(p) in quanta, or None where a step is not finite."""
    q = _quanta(p[1:], p[:-1])
    return None if q is None else int(q.sum())


def _rule(traj, wp, S, L_static, L_moving):
    """One forecast (or track) against the driven path: None where a step or a distance is not finite, else (kind, D, hit)."""
    P, D = _path(traj), _quanta(traj, wp)
    if P is None or D is None:
        return None
    kind = STATIC if P < S else MOVING
    D = int(D.min())
    return kind, D, D < (L_static if kind == STATIC else L_moving)


def eval_drive_numpy(acc, ego_plan, ego_cast, cmd, bra, ego_locs, other_cast, other_cmds, locs, typs, n, *, rules: DriveRules, nbins=NBINS):
    """The specification of lav_amd.ops.eval_drive, same arguments (tensors or arrays), on the host: adds one frame's counters to `acc`
    (int64 array of len(DriveLayout(nbins))) and returns it.  Written to be read: loops over vehicles and modes, float64 throughout."""
    lay = DriveLayout(nbins)
    if not (isinstance(acc, np.ndarray) and acc.dtype == np.int64 and acc.shape == (lay.words,)):
        raise ValueError(f"acc must be an int64 array of {lay.words} words")
    ego_plan, ego_cast, ego_locs = _np(ego_plan, np.float32), _np(ego_cast, np.float32), _np(ego_locs, np.float32)
    locs, typs = _np(locs, np.float32), _np(typs, np.int32)
    T, G = ego_plan.shape[0], locs.shape[0]
    n, cmd = int(n), int(cmd)
    if not 2 <= T <= MAX_PLAN or ego_plan.shape != (T, 2) or ego_cast.shape != (T, 2) or ego_locs.shape != (T + 1, 2):
        raise ValueError(f"ego_plan {ego_plan.shape}, ego_cast {ego_cast.shape}, ego_locs {ego_locs.shape} (2 .. {MAX_PLAN} waypoints)")
    if G > MAX_OBJS or locs.shape != (G, T + 1, 2) or typs.shape != (G,) or not 0 <= n <= G:
        raise ValueError(f"locs {locs.shape}, typs {typs.shape}, n = {n} (at most {MAX_OBJS} tracks)")
    if not 0 <= cmd < NUM_CMDS:
        raise ValueError(f"command {cmd}")
    if isinstance(bra, (torch.Tensor, np.ndarray)):
        bra = bra.item()
    if bra not in (0, 1):
        raise ValueError(f"bra {bra!r} (0 or 1)")
    bra = int(bra)
    if max(rules.aim_point) >= T:
        raise ValueError(f"aim_point {rules.aim_point} of {T} waypoints")
    N = 0 if other_cast is None else len(other_cast)
    if N:
        other_cast, other_cmds = _np(other_cast, np.float32), _np(other_cmds, np.float32)
        if N > MAX_OTHERS or other_cast.shape != (N, NUM_CMDS, T, 2) or other_cmds.shape != (N, NUM_CMDS):
            raise ValueError(f"other_cast {other_cast.shape}, other_cmds {other_cmds.shape} (at most {MAX_OTHERS} vehicles)")
    v = lambda name: lay.view(acc, name)
    S = int(np.rint(float(rules.brake_speed) * (T - 1) * float(QUANTA)))
    L = lambda x: int(np.rint(float(x) * float(QUANTA)))
    L_static, L_moving = L(rules.dist_static), L(rules.dist_moving)
    behind, a = float(rules.behind), rules.aim_point[cmd]
    v("frames")[...] += 1

    # the driven path
    wp = ego_cast if cmd in (4, 5) else ego_plan
    P_wp, aim = _path(wp), _quanta(wp[a:a + 1], ego_locs[1 + a:2 + a])
    if P_wp is None or aim is None:
        v("plan_nonfinite")[...] += 1
        return acc
    slow = int(P_wp < S)

    # plan_collide on the forecasts
    hit, clear, modes = [0, 0], [None, None], v("modes")
    for k in range(N):
        if float(other_cast[k, 0, 0, 1]) > behind:         # mode 0's first waypoint speaks for all six modes (a NaN is not behind)
            v("vehicles_behind")[...] += 1
            continue
        for m in range(NUM_CMDS):
            if float(other_cmds[k, m]) < float(rules.cmd_thresh):      # (a NaN score is considered)
                continue
            modes[M_CONSIDERED] += 1
            got = _rule(other_cast[k, m], wp, S, L_static, L_moving)
            if got is None:
                modes[M_NONFINITE] += 1
                continue
            kind, D, hits = got
            modes[M_STATIC] += int(kind == STATIC)
            modes[M_HITS] += int(hits)
            hit[kind] |= int(hits)
            clear[kind] = D if clear[kind] is None else min(clear[kind], D)

    # the same rule on the recorded futures, and the pedestrians
    gt_hit, near = [0, 0], 0
    r = float(rules.ego_radius)
    for g in range(n):
        if typs[g] == 1:
            x, y = float(locs[g, 0, 0]), float(locs[g, 0, 1])
            if x * x + y * y <= r * r or float(locs[g, 1, 1]) > behind:
                continue
            got = _rule(locs[g, 1:], wp, S, L_static, L_moving)
            if got is not None:
                gt_hit[got[0]] |= int(got[2])
        elif typs[g] == 0:
            D = _quanta(locs[g, 1:], wp)
            near |= int(D is not None and int(D.min()) < L_static)

    v("cause")[bra, slow | hit[STATIC] << 1 | hit[MOVING] << 2] += 1
    v("gt_cause")[bra, slow | gt_hit[STATIC] << 1 | gt_hit[MOVING] << 2] += 1
    v("collide_conf")[int(any(gt_hit)), int(any(hit))] += 1
    v("ped")[bra, near] += 1
    v("speed_hist")[bra, min(nbins - 1, (P_wp // (T - 1)) >> SPEED_SHIFT)] += 1
    for kind in (STATIC, MOVING):
        if clear[kind] is None:
            v("clear_none")[bra, kind] += 1
        else:
            v("clear_hist")[bra, kind, min(nbins - 1, clear[kind] >> CLEAR_SHIFT)] += 1

    # the expert
    P_exp = _path(ego_locs[1:])
    if P_exp is None:
        v("expert_nonfinite")[...] += 1
        return acc
    v("expert")[bra, int(P_exp < S)] += 1
    v("speed")[cmd] += (1, P_wp, P_exp, abs(P_wp - P_exp))
    lateral = abs(float(wp[a, 0]) - float(ego_locs[1 + a, 0]))
    v("aim")[cmd] += (int(aim[0]), int(np.rint(lateral * float(QUANTA))))
    return acc


# ------------------------------------------------------------------------------------------------------------ the summary
def _prf(tp, fp, fn):
    p, r = _ratio(tp, tp + fp), _ratio(tp, tp + fn)
    return dict(tp=int(tp), fp=int(fp), fn=int(fn), precision=p, recall=r, f1=_ratio(2 * tp, 2 * tp + fp + fn))


def _brake(cause):
    """[bra][mask] -> the rule "brake when mask != 0" against the label, and how the rule's brakes divide over their causes."""
    brakes = int(cause[:, 1:].sum())
    share = lambda bit: _ratio(int(cause[:, [m for m in range(8) if m & bit]].sum()), brakes)
    return dict(**_prf(cause[1, 1:].sum(), cause[0, 1:].sum(), cause[1, 0]), brakes=brakes,
                share=dict(slow=share(1), collide_static=share(2), collide_moving=share(4), slow_only=_ratio(int(cause[:, 1].sum()), brakes)))


def _sweep(neg, pos, edge, extra_pos=0):
    """A precision / recall table of "brake when the value is below the edge of bin i" (i = 1 .. nbins - 1; the last bin is open) from
    the histograms of the value on driving (`neg`) and braking (`pos`) frames.  extra_pos: braking frames without a value, which no
    threshold makes brake.  Each table moves ONE threshold with nothing else: brake_speed's is the desired-speed rule alone (and the
    forecasts keep the kind they had at the brake_speed in force), a distance limit's is that kind's collisions alone."""
    out, tp, fp = [], 0, 0
    total_pos = int(pos.sum()) + extra_pos
    for i in range(1, len(pos)):
        tp, fp = tp + int(pos[i - 1]), fp + int(neg[i - 1])
        out.append(dict(threshold=edge(i), **_prf(tp, fp, total_pos - tp)))
    return out


def summarise(acc, num_plan: int = 20) -> dict:
    """Metrics from an accumulator (array or tensor); a zero denominator gives None, never a NaN.  Distances in metres (quanta / 2^20),
    speeds in metres per step (path quanta / (2^20 (T - 1)))."""
    acc = _np(acc, np.int64)
    lay = DriveLayout.of(acc)
    v = lambda name: lay.view(acc, name)
    one = lambda name: int(v(name).reshape(-1)[0])
    steps = int(num_plan) - 1
    cause, gt_cause, conf, ped, expert, speed, aim, modes = (v(k) for k in ("cause", "gt_cause", "collide_conf", "ped", "expert", "speed", "aim", "modes"))
    out = dict(frames=one("frames"), plan_nonfinite=one("plan_nonfinite"), expert_nonfinite=one("expert_nonfinite"), evaluated=int(cause.sum()),
               labelled_brake=int(cause[1].sum()), brake=_brake(cause), brake_gt_futures=_brake(gt_cause),
               collide_agreement=dict(both=int(conf[1, 1]), forecast_only=int(conf[0, 1]), gt_only=int(conf[1, 0]), neither=int(conf[0, 0]),
                                      agreement=_ratio(int(conf[0, 0] + conf[1, 1]), int(conf.sum())), **{k: val for k, val in
                                      _prf(conf[1, 1], conf[0, 1], conf[1, 0]).items() if k in ("precision", "recall", "f1")}),
               pedestrian_near=dict(braking=_ratio(int(ped[1, 1]), int(ped[1].sum())), driving=_ratio(int(ped[0, 1]), int(ped[0].sum()))),
               expert_slow=dict(braking=_ratio(int(expert[1, 1]), int(expert[1].sum())), driving=_ratio(int(expert[0, 1]), int(expert[0].sum()))),
               modes=dict(considered=int(modes[M_CONSIDERED]), static=int(modes[M_STATIC]), hits=int(modes[M_HITS]), nonfinite=int(modes[M_NONFINITE]),
                          vehicles_behind=one("vehicles_behind")))
    per_cmd = []
    for k in range(NUM_CMDS):
        f = int(speed[k, 0])
        per_cmd.append(dict(frames=f, desired_speed=_ratio(speed[k, 1], QUANTA * steps * f), expert_speed=_ratio(speed[k, 2], QUANTA * steps * f),
                            speed_error=_ratio(speed[k, 3], QUANTA * steps * f), aim_error=_ratio(aim[k, 0], QUANTA * f),
                            lateral_error=_ratio(aim[k, 1], QUANTA * f)))
    out["per_cmd"] = per_cmd
    speed_hist, clear_hist, clear_none = v("speed_hist"), v("clear_hist"), v("clear_none")
    out["sweep"] = dict(brake_speed=_sweep(speed_hist[0], speed_hist[1], lambda i: i / float(QUANTA >> SPEED_SHIFT)),
                        dist_static=_sweep(clear_hist[0, STATIC], clear_hist[1, STATIC], lambda i: i / float(QUANTA >> CLEAR_SHIFT),
                                           int(clear_none[1, STATIC])),
                        dist_moving=_sweep(clear_hist[0, MOVING], clear_hist[1, MOVING], lambda i: i / float(QUANTA >> CLEAR_SHIFT),
                                           int(clear_none[1, MOVING])))
    return out


# ------------------------------------------------------------------------------------------------------------ the evaluator
class DriveEvaluator(Evaluator):
    """Evaluator's per-frame chain with lav_eval_drive as its metrics launch.

        ev = DriveEvaluator(lav, rules=DriveRules())   # a lav_amd.train.LAV of stage "lidar", or (lidar_model, uniplanner)
        ev.run(loader, max_frames=None)                # -> frames evaluated
        ev.counters()                                  # the accumulator, read once

    device "cpu": eval_drive_numpy on the host (EvaluatorBase)."""

    def __init__(self, lav_or_modules, precision=None, device=None, *, cfg=None, rules: DriveRules = None, nbins=NBINS):
        super().__init__(lav_or_modules, precision, device, cfg=cfg)
        self.rules = rules or DriveRules()
        self.nbins = int(nbins)
        self.layout = DriveLayout(self.nbins)
        self.acc = torch.zeros(len(self.layout), dtype=torch.int64, device=self.device)
        if max(self.rules.aim_point) >= self.num_plan:
            raise ValueError(f"aim_point {self.rules.aim_point} of {self.num_plan} waypoints")

    def upload(self, batch):
        """Evaluator.upload, and the expert's brake label, which stays on the host: it is an argument of the launch."""
        count = super().upload(batch)
        bras = batch[9]
        self._batch["bras"] = [int(b != 0) for b in (bras.tolist() if isinstance(bras, torch.Tensor) else bras)]
        return count

    def metrics(self, i, out):
        b = self._batch
        n = min(b["n"][i], b["locs"].shape[1])
        self._add("eval_drive", eval_drive_numpy, None, out["ego_plan"], out["ego_cast"], out["cmd"], b["bras"][i], b["ego_locs"][i], out["other_cast"],
                  out["other_cmds"], b["locs"][i], b["typs"][i], n, rules=self.rules, nbins=self.nbins)


# ------------------------------------------------------------------------------------------------------------ command line
def _rules(args) -> DriveRules:
    config = None
    if args.agent_config:
        import yaml
        with open(args.agent_config, "r") as f:
            config = yaml.safe_load(f) or {}
    return DriveRules.from_config(config, brake_speed=args.brake_speed, cmd_thresh=args.cmd_thresh, dist_static=args.dist_static,
                                  dist_moving=args.dist_moving, aim_point=args.aim_point)


TOOL = dict(
    name="eval_drive_v2", what="eval_drive", about="open-loop metrics of the agent's brake and aim rules on a LiDAR student + planner checkpoint",
    unit="frames", checkpoints=dict(lidar="lidar_model_dir", uniplanner="uniplanner_dir", bev="bev_model_dir"), precisions=PRECISIONS, batch_size=8,
    frames=8, synthetic="synthetic_lidar_batch samples",
    flags=[("--max-points", dict(type=int, default=None, help="--synthetic: points per cloud (default: the config's max_lidar_points)")),
           ("--agent-config", dict(default=None, metavar="YAML", help="the agent's config.yaml: brake_speed, cmd_thresh, aim_point and pixels_per_meter "
                                                                      "are read from it (flags given beside it win)")),
           ("--brake-speed", dict(type=float, default=None, help="metres per step below which a path brakes (default: the agent's, 0.2)")),
           ("--cmd-thresh", dict(type=float, default=None, help="score below which a forecast mode is ignored (default: the agent's, 0.2)")),
           ("--dist-static", dict(type=float, default=None, help="metres within which a standing forecast brakes (default: plan_collide's, 1.0)")),
           ("--dist-moving", dict(type=float, default=None, help="metres within which a moving forecast brakes (default: plan_collide's, 2.5)")),
           ("--aim-point", dict(type=int, nargs=NUM_CMDS, default=None, metavar="T", help="the aimed waypoint per command (default: the agent's, 4 4 4 3 6 6)")),
           ("--nbins", dict(type=int, default=NBINS, help="bins of the speed (1/64 m per step) and clearance (1/8 m) histograms"))],
    build=_build, batches=_batches,
    make_evaluator=lambda lav, name, args: DriveEvaluator(lav, precision=name, rules=_rules(args), nbins=args.nbins),
    line=lambda ev, acc, args, cfg: dict(rules=ev.rules.named(), camera_brake="not evaluated", summary=summarise(acc, cfg.num_plan)),
    keys=("what", "precision", "data", "frames_per_s", "rules", "camera_brake", "summary", "counters"))


def main(argv=None):
    """eval_drive_v2.py: one JSON line per precision - the rules in force, the summary, the raw counters and the frames per second."""
    return run_cli(TOOL, argv)


if __name__ == "__main__":
    main()
