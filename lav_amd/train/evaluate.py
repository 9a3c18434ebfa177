"""Open-loop evaluation of a LiDAR student + planner checkpoint on recorded routes (eval_full_v2.py).

The trainers print losses on augmented batches; this module measures a checkpoint on frames it never trained on: BEV segmentation IoU,
detection precision / recall / AP, the ego plan's displacement errors and the other vehicles' forecasts, per frame of the
'temporal_lidar_painted' loader with its augmentations switched off.  A frame runs the way InferModel.forward runs it; its metrics
are ADDED to one int64 accumulator in HBM by one launch (lav_eval_frame, lav_amd.ops.eval_frame) and the accumulator is read once, when
the route is done.  `eval_frame_numpy` below is that kernel's specification and the two agree in every bit (tests/test_gpu_eval.py).

The reference has no evaluator (its answer to "which epoch do I drive with" is closed-loop CARLA): the metric definitions are this
project's, and parity with a reference is UNPINNED because there is nothing to pin it to.  What is pinned: the kernel to this
specification, the specification to hand-derived counters, and the ground-truth pixel convention to the loader's own heat maps
(tests/test_eval_host.py).

Definitions (DESIGN 4.7g has the reasons):
  segmentation  per channel, inside mask > 0: tp = pred & label, fp = pred & ~label, fn = ~pred & label, pred = pred_bev > threshold.
  detection     per class: ground-truth pixel = float64(loc) * ppm + centre of frame 0 of the actors g < n of that class
                (detections_to_heatmap's and LAV._pixels' convention), ignored outside [0, W) x [0, H).  Rows in order; a row with
                float64(score) > min_score takes the nearest not-yet-taken actor (squared pixel distance, float64, ties to the lowest
                index) when it lies within the radius - a true positive -, else it is a false positive.  Both go to a score histogram,
                bin = min(nbins - 1, int(float32(score) * float32(nbins))), and to the pair of counters of float64(score) > det_score.
                The agent's size and range filters are NOT applied: this measures the detector.
  ego plan      q_t = rint(sqrt(dx^2 + dy^2) * 2^20) against ego_locs[t + 1], float64; per command: frames, sum of q_t, q_{T-1}.  A
                plan with a distance that is not below 2^32 m (NaN - the persistent plan kernel's time-out -, Inf) counts in
                plan_nonfinite only.
  others        forecast k came from row other_row[k] of class 1; if that row is a true positive of actor g: S_m = sum_t q_t of mode m
                against locs[g, t + 1], min_m S_m, and S and q_{T-1} of the first maximum of other_cmds[k]; else "unmatched".
Every term is an integer before it is added, so the sums do not depend on the order of frames or of workgroups.
"""
from __future__ import annotations

import numpy as np
import torch

from .eval_common import (FAR, NUM_CMDS, PRECISION_NAMES, QUANTA, AccLayout, EvaluatorBase, SeededFrames, _np, _quanta, _ratio,  # noqa: F401
                          average_precision, run_cli, synthetic_batches)                   # (re-exported: the tests and tools read them here)

NBINS = 256
MAX_DET = 20


class Layout(AccLayout):
    """The accumulator's named slices, in words of int64: lav_eval_frame's layout (csrc/eval_metrics.hip, include/lav_amd.h).
    seg [channel][tp, fp, fn]; det [class][tp, fp]; plan [cmd][frames, sum, final]; hist [class][tp, fp][bin]."""
    FIELDS = (("frames", ()), ("seg", (3, 3)), ("n_gt", (2,)), ("det", (2, 2)), ("plan", (NUM_CMDS, 3)), ("plan_nonfinite", ()),
              ("oth_matched", ()), ("oth_unmatched", ()), ("oth_nonfinite", ()), ("oth_min", ()), ("oth_top", ()), ("oth_top_final", ()))

    def __init__(self, nbins: int = NBINS):
        if not 1 <= int(nbins) <= 1024:
            raise ValueError(f"{nbins} score bins (1 .. 1024)")
        self.nbins = int(nbins)
        super().__init__(self.FIELDS + (("hist", (2, 2, self.nbins)),))

    @classmethod
    def of(cls, acc) -> "Layout":
        head = cls(1).words - 4
        if len(acc) <= head or (len(acc) - head) % 4:
            raise ValueError(f"an accumulator of {len(acc)} words")
        return cls((len(acc) - head) // 4)


ACC = Layout(NBINS)


def eval_frame_numpy(acc, pred_bev, bev, mask, rows, locs, typs, n, ego_plan, ego_locs, cmd, other_cast, other_cmds, other_row, *, ppm,
                     centre, radius_px, threshold=0.5, min_score=0.1, det_score=0.2, nbins=NBINS):
    """The specification of lav_amd.ops.eval_frame, same arguments (tensors or arrays), on the host: adds one frame's counters to
    `acc` (int64 array of len(Layout(nbins))) and returns it.  Written to be read: loops over rows and actors, float64 throughout."""
    lay = Layout(nbins)
    if not (isinstance(acc, np.ndarray) and acc.dtype == np.int64 and acc.shape == (lay.words,)):
        raise ValueError(f"acc must be an int64 array of {lay.words} words")
    pred_bev, bev, mask = _np(pred_bev, np.float32), _np(bev, np.uint8), _np(mask, np.uint8)
    rows, locs, typs = _np(rows, np.float32), _np(locs, np.float32), _np(typs, np.int32)
    ego_plan, ego_locs = _np(ego_plan, np.float32), _np(ego_locs, np.float32)
    H, W = pred_bev.shape[1:]
    T = ego_plan.shape[0]
    n, cmd, ppm, radius_px = int(n), int(cmd), float(ppm), float(radius_px)
    if not 0 <= cmd < NUM_CMDS:
        raise ValueError(f"command {cmd}")
    lay.view(acc, "frames")[...] += 1

    # BEV segmentation
    seg = lay.view(acc, "seg")
    inside = mask > 0
    for c in range(3):
        pred, label = pred_bev[c] > np.float32(threshold), bev[c] > 0
        seg[c, 0] += int((pred & label & inside).sum())
        seg[c, 1] += int((pred & ~label & inside).sum())
        seg[c, 2] += int((~pred & label & inside).sum())

    # detection: greedy matching in row order
    match = np.full((2, rows.shape[1]), -1, np.int64)
    hist, det, n_gt = lay.view(acc, "hist"), lay.view(acc, "det"), lay.view(acc, "n_gt")
    for c in range(2):
        gt = {}
        for g in range(n):
            if typs[g] != c:
                continue
            px = float(locs[g, 0, 0]) * ppm + float(centre[0])
            py = float(locs[g, 0, 1]) * ppm + float(centre[1])
            if 0.0 <= px < W and 0.0 <= py < H:
                gt[g] = (px, py)
        n_gt[c] += len(gt)
        taken = set()
        for r in range(rows.shape[1]):
            score = rows[c, r, 0]
            if not float(score) > min_score:          # (a NaN score is skipped)
                continue
            x, y = float(rows[c, r, 1]), float(rows[c, r, 2])
            best, best_g = np.inf, -1
            for g, (px, py) in gt.items():            # ascending g: a tie keeps the lowest index
                if g in taken:
                    continue
                d2 = (x - px) * (x - px) + (y - py) * (y - py)
                if d2 < best:
                    best, best_g = d2, g
            hit = best_g >= 0 and best <= radius_px * radius_px
            if hit:
                taken.add(best_g)
                match[c, r] = best_g
            scaled = np.float32(score) * np.float32(nbins)
            b = nbins - 1 if scaled >= np.float32(nbins - 1) else int(scaled)
            hist[c, 0 if hit else 1, b] += 1
            if float(score) > det_score:
                det[c, 0 if hit else 1] += 1

    # the ego plan
    q = _quanta(ego_plan, ego_locs[1:])
    if q is None:
        lay.view(acc, "plan_nonfinite")[...] += 1
    else:
        lay.view(acc, "plan")[cmd] += (1, int(q.sum()), int(q[-1]))

    # the others' forecasts
    N = 0 if other_cast is None else len(other_cast)
    if N:
        other_cast, other_cmds, other_row = _np(other_cast, np.float32), _np(other_cmds, np.float32), _np(other_row, np.int32)
    for k in range(N):
        r = int(other_row[k])
        g = int(match[1, r]) if 0 <= r < rows.shape[1] else -1
        if g < 0:
            lay.view(acc, "oth_unmatched")[...] += 1
            continue
        per_mode = [_quanta(other_cast[k, m], locs[g, 1:]) for m in range(NUM_CMDS)]
        if any(p is None for p in per_mode):
            lay.view(acc, "oth_nonfinite")[...] += 1
            continue
        sums = [int(p.sum()) for p in per_mode]
        top = int(np.argmax(other_cmds[k]))           # the first maximum; a NaN counts as one
        lay.view(acc, "oth_matched")[...] += 1
        lay.view(acc, "oth_min")[...] += min(sums)
        lay.view(acc, "oth_top")[...] += sums[top]
        lay.view(acc, "oth_top_final")[...] += int(per_mode[top][-1])
    return acc


def summarise(acc, num_plan: int = 20) -> dict:
    """Metrics from an accumulator (array or tensor); a zero denominator gives None, never a NaN.  Distances in metres:
    sum of q / (2^20 * num_plan * count) for the averages (ADE), final q / (2^20 * count) for the final displacement (FDE)."""
    acc = _np(acc, np.int64)
    lay = Layout.of(acc)
    v = lambda name: lay.view(acc, name)
    one = lambda name: int(v(name).reshape(-1)[0])
    T = int(num_plan)
    out = dict(frames=one("frames"))
    seg = v("seg")
    iou = [_ratio(seg[c, 0], seg[c].sum()) for c in range(3)]
    out["seg"] = dict(iou=iou, mean_iou=None if any(i is None for i in iou) else float(np.mean(iou)),
                      labelled=[int(seg[c, 0] + seg[c, 2]) for c in range(3)])
    det, hist, n_gt = v("det"), v("hist"), v("n_gt")
    out["det"] = []
    for c in range(2):
        tp, fp, gt = int(det[c, 0]), int(det[c, 1]), int(n_gt[c])
        out["det"].append(dict(n_gt=gt, tp=tp, fp=fp, fn=gt - tp, precision=_ratio(tp, tp + fp), recall=_ratio(tp, gt),
                               ap=average_precision(hist[c, 0], hist[c, 1], gt)))
    plan = v("plan")
    per_cmd = [dict(frames=int(plan[k, 0]), ade=_ratio(plan[k, 1], QUANTA * T * int(plan[k, 0])), fde=_ratio(plan[k, 2], QUANTA * int(plan[k, 0])))
               for k in range(NUM_CMDS)]
    cnt = int(plan[:, 0].sum())
    out["plan"] = dict(per_cmd=per_cmd, frames=cnt, ade=_ratio(plan[:, 1].sum(), QUANTA * T * cnt), fde=_ratio(plan[:, 2].sum(), QUANTA * cnt),
                       nonfinite=one("plan_nonfinite"))
    m = one("oth_matched")
    out["others"] = dict(matched=m, unmatched=one("oth_unmatched"), nonfinite=one("oth_nonfinite"), min_ade=_ratio(one("oth_min"), QUANTA * T * m),
                         top_ade=_ratio(one("oth_top"), QUANTA * T * m), top_fde=_ratio(one("oth_top_final"), QUANTA * m))
    return out


# ------------------------------------------------------------------------------------------------------------ the evaluator
PRECISIONS = ("f16x3", "bf16x6", "f32")


def forecast_rows(infer, rows: np.ndarray, dets1) -> np.ndarray:
    """For each forecast UniPlanner.infer_all makes of `dets1` (= det_decode_fast(rows)[0][1]) the row of rows[1] it came from.
    det_decode_fast keeps rows in order and others_from_detections drops the ego's own box, so the forecasts are the kept detections
    minus those, in row order; a kept detection is found again by its pixel (peaks of one class never share one)."""
    H, W = infer._bev_hw
    up = infer.uniplanner
    out, j = [], 0
    for det in dets1:
        while not (float(rows[1, j, 0]) > 0.2 and int(rows[1, j, 1]) == det[0] and int(rows[1, j, 2]) == det[1]):
            j += 1
        if len(up.others_from_detections([det], H, W)[0]):
            out.append(j)
        j += 1
    return np.asarray(out, np.int32)


class Evaluator(EvaluatorBase):
    """Runs frames of loader batches through the student and accumulates their metrics.

        ev = Evaluator(lav)                  # a lav_amd.train.LAV of stage "lidar", or (lidar_model, uniplanner)
        ev.run(loader, max_frames=None)      # -> frames evaluated
        ev.counters()                        # the accumulator, read once

    device "cpu": eval_frame_numpy on the host (EvaluatorBase)."""

    def __init__(self, lav_or_modules, precision=None, device=None, *, cfg=None, match_radius=2.0, threshold=0.5, min_score=0.1,
                 det_score=0.2, nbins=NBINS):
        from ..model_inference import InferModel
        from .lav import TrainConfig
        from .losses import build_seg_mask
        if isinstance(lav_or_modules, (tuple, list)):
            lidar_model, uniplanner = lav_or_modules
            cfg = cfg or TrainConfig()
        else:
            lidar_model, uniplanner, cfg = lav_or_modules.lidar_model, lav_or_modules.uniplanner, cfg or lav_or_modules.cfg
        self.nbins = int(nbins)
        super().__init__(lidar_model, Layout(self.nbins), precision, device)
        self.infer = InferModel(self.model, uniplanner.eval(), 1.5, 2.4, self.model_device, precision=self.code)
        self.ppm = float(cfg.pixels_per_meter)
        H, W = int((cfg.max_x - cfg.min_x) * cfg.pixels_per_meter), int((cfg.max_y - cfg.min_y) * cfg.pixels_per_meter)
        # LAV.bev_center
        self.centre = (W / 2 + (cfg.min_y + cfg.max_y) / 2 * cfg.pixels_per_meter, H / 2 + (cfg.min_x + cfg.max_x) / 2 * cfg.pixels_per_meter)
        self.mask = (build_seg_mask(h=H, w=W, cx=self.centre[0], cy=self.centre[1]) > 0).to(torch.uint8).to(self.model_device)
        self.num_plan = int(cfg.num_plan)
        self.kw = dict(ppm=self.ppm, centre=self.centre, radius_px=float(match_radius) * self.ppm, threshold=float(threshold),
                       min_score=float(min_score), det_score=float(det_score), nbins=self.nbins)
        self.frames = 0
        self._batch = None

    def upload(self, batch):
        """The ground truth of one loader batch (train_lidar's tuple), uploaded once; frames index into it.  `bev` stays uint8."""
        lidars, num_points, _, _, _, bev, ego_locs, cmds, nxps, _, locs, _, typs, num_objs = batch
        d = self.model_device
        as_list = lambda t: [int(v) for v in (t.tolist() if isinstance(t, torch.Tensor) else t)]
        self._batch = dict(lidars=lidars.to(d, torch.float32), num_points=as_list(num_points), bev=bev.to(d, torch.uint8).contiguous(),
                           ego_locs=ego_locs.to(d, torch.float32), cmds=as_list(cmds), nxps=nxps.to(d, torch.float32),
                           locs=locs.to(d, torch.float32), typs=typs.to(d, torch.int32), n=as_list(num_objs))
        return len(self._batch["cmds"])

    @torch.no_grad()
    def forward(self, i) -> dict:
        """Sample i of the uploaded batch through InferModel.forward's chain with the trainers' 20 peaks per class: what the metrics
        launches read, all of it in HBM but other_row (and the CPU zeros of a frame without forecasts)."""
        from .. import ops
        b, im = self._batch, self.infer
        lm, up = im.lidar_model, im.uniplanner
        pts = b["lidars"][i, :b["num_points"][i]]
        cmd = b["cmds"][i]
        with ops.precision(im.precision):
            features = lm.backbone(lm.point_pillar_net([pts], [len(pts)]))
            heat, size, ori, pred_bev = lm.heads(features)
            rows = ops.extract_peaks(heat[0], size[0], ori[0], max_det=MAX_DET, apply_sigmoid=True)
            rows_host = rows.cpu().numpy()              # the copy InferModel.forward makes: the others branch is sized on the host
            dets, _, _ = im.det_decode_fast(rows_host)
            other_row = forecast_rows(im, rows_host, dets[1])
            _, ego_plan, ego_cast, other_cast, other_cmds = up.infer_all(features[0], dets[1], cmd, b["nxps"][i], amax=ops.amax_of(features))
        return dict(pred_bev=pred_bev[0], rows=rows, cmd=cmd, ego_plan=ego_plan, ego_cast=ego_cast, other_cast=other_cast, other_cmds=other_cmds,
                    other_row=other_row)

    def metrics(self, i, out):
        """The metrics launch of sample i on what `forward` returned."""
        b = self._batch
        n = min(b["n"][i], b["locs"].shape[1])
        args = (out["pred_bev"], b["bev"][i], self.mask, out["rows"], b["locs"][i], b["typs"][i], n, out["ego_plan"], b["ego_locs"][i], out["cmd"],
                out["other_cast"], out["other_cmds"])
        self._add("eval_frame", eval_frame_numpy, None, *args, torch.from_numpy(out["other_row"]).to(self.device), **self.kw)

    @torch.no_grad()
    def frame(self, i):
        """Sample i of the uploaded batch: the forward chain, then the metrics launch."""
        self.metrics(i, self.forward(i))
        self.frames += 1

    def run(self, batches, max_frames=None) -> int:
        for batch, left in self._budget(batches, max_frames, lambda: self.frames):
            for i in range(self.upload(batch))[:left]:
                self.frame(i)
        return self.frames

    def precision(self) -> str:
        """The arithmetic asked for: InferModel runs every engine at it."""
        return PRECISION_NAMES.get(self.code, "default")


# ------------------------------------------------------------------------------------------------------------ command line
def held_out_frames(config_path, data_dir=None, seed=2021):
    """The 'temporal_lidar_painted' loader's dataset over `data_dir` (default: the config's) with every augmentation at 0, seeded
    per sample."""
    from ..data.datasets import TemporalLiDARPaintedDataset
    ds = TemporalLiDARPaintedDataset(config_path, seed=seed, overrides=dict(data_dir=data_dir) if data_dir else None)
    ds.angle_jitter = ds.stack_loc_jitter = ds.stack_ori_jitter = 0
    return SeededFrames(ds, seed)


def _build(args, cfg, device):
    from .lav import LAV
    ck = {k: torch.load(getattr(args, k), map_location="cpu") for k in TOOL["checkpoints"] if getattr(args, k)}
    lav = LAV(cfg, device, what="lidar", checkpoints=ck, distributed=False)       # (an evaluation is one process's own: no collective)
    lav.student.eval()
    return lav


def _batches(args, cfg):
    from .synthetic import synthetic_lidar_batch
    if args.synthetic:
        return synthetic_batches(synthetic_lidar_batch, args.frames, args.batch_size, args.seed, max_points=args.max_points or cfg.max_lidar_points)
    return held_out_frames(args.config_path, args.data_dir, args.seed)


TOOL = dict(
    name="eval_full_v2", what="eval_full", about="open-loop metrics of a LiDAR student + planner checkpoint on recorded routes", unit="frames",
    checkpoints=dict(lidar="lidar_model_dir", uniplanner="uniplanner_dir", bev="bev_model_dir"), precisions=PRECISIONS, batch_size=8, frames=8,
    synthetic="synthetic_lidar_batch samples",
    flags=[("--max-points", dict(type=int, default=None, help="--synthetic: points per cloud (default: the config's max_lidar_points)")),
           ("--match-radius", dict(type=float, default=2.0, help="metres within which a detection matches a ground-truth actor"))],
    build=_build, batches=_batches, make_evaluator=lambda lav, name, args: Evaluator(lav, precision=name, match_radius=args.match_radius),
    line=lambda ev, acc, args, cfg: dict(match_radius_m=args.match_radius, summary=summarise(acc, cfg.num_plan)),
    keys=("what", "precision", "data", "frames_per_s", "match_radius_m", "summary", "counters"))


def main(argv=None):
    """eval_full_v2.py: one JSON line per precision - the summary, the raw counters and the frames per second of the evaluation."""
    return run_cli(TOOL, argv)


if __name__ == "__main__":
    main()
