"""Rotated-box metrics of the detector's box and orientation heads on recorded routes (eval_det_v2.py).

eval_full_v2 scores a detection by its centre alone: lav_eval_frame reads (score, x, y) of a peak row and never (w, h, cos, sin) - the
numbers lav_det_decode turns into the heading every other vehicle's crop is rotated by, that decide through max(w, h) < min_box whether
the agent keeps a detection, and that the debug and log views draw.  This module measures them, per frame of the
'temporal_lidar_painted' loader with its augmentations switched off: pillars -> backbone -> LiDARModel.detect, then ONE launch
(lav_eval_det, lav_amd.ops.eval_det) that ADDS a frame's integers into an int64 accumulator in HBM; nothing of a frame is copied to the
host and the accumulator is read once.  `eval_det_numpy` below is that kernel's specification - the final word on the order of every
operation - and the two agree in every word (tests/test_gpu_eval_det.py).  The detector needs no planner.

The reference has no evaluator: the definitions are this project's, and parity with a reference is UNPINNED because there is nothing
to pin it to.  What is pinned: the kernel to this specification, the specification's IoU to exact rational clipping and to hand-derived
cases, its arm 0 to eval_frame_numpy, its corners to log_view.quad_corners, and the ground-truth boxes to the loader's own regression
targets (tests/test_eval_det_host.py).

Definitions (DESIGN 4.7l has the reasons).  Everything is float64 from the float32 inputs; only + - * /, sqrt and comparisons appear.
  ground truth  actor g < n of class typs[g]: pixel (px, py) = float64(locs[g, 0]) * ppm + centre, kept when it lies in [0, W) x [0, H)
                (eval_frame_numpy's rule).  Its box is read where the heads were trained to regress it: ix = min(W - 1, int(px + 0.5)),
                iy likewise; half extents size_map[:, iy, ix] in pixels, direction ori_map[:, iy, ix]; the centre is (px, py) itself.
                (The batch carries no bbox.  detections_to_heatmap writes every pixel within about 10 px of an actor with the box of the
                strongest Gaussian there, so an actor reads its own box unless another one is nearer to that pixel.)
  a valid box   (C, w, h, c, s): all finite, w > 0, h > 0, n = c c + s s finite and > 0.  r = sqrt(n), c^ = c / r, s^ = s / r; the
                heading in pixel axes is u = (s^, -c^) - the arrow log_view._boxes draws -, the side axis v = (c^, s^); corners
                counter-clockwise: C - w u - h v, C + w u - h v, C + w u + h v, C - w u + h v (each ((C - w u) - h v), left to right).
                For unit (cos, sin) these are log_view.quad_corners.  An invalid box has IoU 0 with everything.
  IoU           the prediction's quadrilateral clipped against the four edges of the ground truth's, Sutherland-Hodgman, edges in order:
                side(Q) = e.x (Q.y - G_k.y) - e.y (Q.x - G_k.x), e = G_{k+1} - G_k, inside when side >= 0.  One pass over the vertices
                V_i in order with S = V_i, E = V_{i+1 mod n}: S is kept when it is inside, and when exactly one of S, E is inside the
                crossing S + (dS / (dS - dE)) (E - S) follows.  At most 8 vertices (a ninth would be dropped).  A = 0.5 |sum_i cross(V_i - V_0, V_{i+1} - V_0)|
                in index order, iou = A / ((aP + aG) - A) with a = (2 w) (2 h); 0 when A or the union is not > 0 or the quotient is
                not finite.  iou_q = 2^20 when iou 2^20 >= 2^20, else llrint(iou 2^20).
  matching      per class, rows in order, over rows with float64(score) > min_score, four arms each with its own set of taken actors:
                arm 0 is eval_frame_numpy's centre rule word for word (the nearest free actor within radius_px, ties to the lowest
                index); arm 1 + k takes the free actor of the row's class with the largest iou_q, ties to the lowest index, if iou_q >=
                L_k and iou_q > 0; otherwise the row is a false positive.
  counters      per arm: the score histogram [class][tp, fp][bin] with eval_frame's float32 bin rule, and det [class][range bin][tp,
                fp] over float64(score) > det_score.  Range bin = the number of edges with d2 >= edge2, d2 the squared pixel distance
                from `centre` (the ego): a true positive's is its actor's, a false positive's the row's own (x, y).
  pairs         arm 0's true positives with score > det_score, by the actor's range bin: pairs += 1; if either box is invalid
                pair_invalid += 1 and nothing else; otherwise sum_centre += Q(sqrt(d2) / ppm) with d2 the matching distance, sum_dw +=
                Q(|w_p - w_g| / ppm), sum_dh likewise, sum_iou += iou_q, and with dot = c^_p c^_g + s^_p s^_g the heading bin is the
                number of edges with dot < cos(edge); a NaN dot goes to the last bin.  Q(x) = llrint(min(x, 2^32) 2^20).
The host passes heading edges as cosines, range edges as (e ppm) (e ppm) and IoU thresholds as L_k = llrint(t_k 2^20), computed once
(`thresholds`); kernel and specification receive the same arrays.  Every term is an integer before it is added, so the sums depend
on no order.  The agent's size and range filters are NOT applied: this measures the detector.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .eval_common import FAR, PRECISION_NAMES, QUANTA, AccLayout, EvaluatorBase, _np, _ratio, average_precision, run_cli, synthetic_batches

NBINS = 256
ARMS, MAX_IOU, MAX_RANGE, MAX_HEADING = 4, 3, 3, 7
IOU_THRESHOLDS = (0.3, 0.5, 0.7)
RANGE_EDGES_M = (15, 30, 50)
HEADING_EDGES_DEG = (5, 10, 20, 45, 90, 135, 175)
HEADS = ("peaks", "dense")
NOTE = ("the agent's size and range filters are NOT applied (this measures the detector); ground-truth boxes are read from the loader's "
        "size / orientation targets at the actor's pixel; parity with a reference is UNPINNED (there is none)")
SYNTHETIC_NOTE = ("--synthetic: the size / orientation maps are unrelated to locs, so most ground-truth boxes land in gt_invalid - a smoke "
                  "run, not a measurement")


class DetLayout(AccLayout):
    """lav_eval_det's accumulator, 135 + 16 nbins words of int64 (csrc/eval_det.hip, include/lav_amd.h): frames; n_gt [class][range
    bin]; gt_invalid, pred_invalid [class]; det [arm][class][range bin][tp, fp]; pairs [class][range bin]; pair_invalid [class];
    sum_centre, sum_dw, sum_dh, sum_iou [class][range bin]; heading [class][bin]; hist [arm][class][tp, fp][score bin]."""
    FIELDS = (("frames", ()), ("n_gt", (2, 4)), ("gt_invalid", (2,)), ("pred_invalid", (2,)), ("det", (ARMS, 2, 4, 2)), ("pairs", (2, 4)),
              ("pair_invalid", (2,)), ("sum_centre", (2, 4)), ("sum_dw", (2, 4)), ("sum_dh", (2, 4)), ("sum_iou", (2, 4)), ("heading", (2, 8)))

    def __init__(self, nbins: int = NBINS):
        if not 1 <= int(nbins) <= 1024:
            raise ValueError(f"{nbins} score bins (1 .. 1024)")
        self.nbins = int(nbins)
        super().__init__(self.FIELDS + (("hist", (ARMS, 2, 2, self.nbins)),))

    @classmethod
    def of(cls, acc) -> "DetLayout":
        head = cls(1).words - 16
        if len(acc) <= head or (len(acc) - head) % 16:
            raise ValueError(f"an accumulator of {len(acc)} words")
        return cls((len(acc) - head) // 16)


def det_layout(heads=("peaks",), nbins: int = NBINS) -> AccLayout:
    """One DetLayout section per head path that is run, in one sectioned layout."""
    one = DetLayout(nbins)
    return AccLayout(tuple((h, "det", tuple((name, shape) for name, (_, shape) in one.fields.items())) for h in heads), sectioned=True)


def thresholds(ppm, iou_thresholds=IOU_THRESHOLDS, range_edges_m=RANGE_EDGES_M, heading_edges_deg=HEADING_EDGES_DEG):
    """What the launch receives in place of the three tuples, computed once on the host: (L_k = llrint(t_k 2^20) int64, (e ppm) (e ppm)
    float64, cos(edge) float64).  IoU thresholds in (0, 1], range edges ascending and positive, heading edges ascending in (0, 180]."""
    iou, rng, hdg = [float(t) for t in iou_thresholds], [float(e) for e in range_edges_m], [float(e) for e in heading_edges_deg]
    if len(iou) > MAX_IOU or len(rng) > MAX_RANGE or len(hdg) > MAX_HEADING:
        raise ValueError(f"at most {MAX_IOU} IoU thresholds, {MAX_RANGE} range edges and {MAX_HEADING} heading edges")
    if not all(0.0 < t <= 1.0 for t in iou):
        raise ValueError(f"IoU thresholds {iou}: in (0, 1]")
    if not all(0.0 < e < 1e6 for e in rng) or sorted(rng) != rng:
        raise ValueError(f"range edges {rng}: positive metres, ascending")
    if not all(0.0 < e <= 180.0 for e in hdg) or sorted(hdg) != hdg:
        raise ValueError(f"heading edges {hdg}: degrees in (0, 180], ascending")
    ppm = float(ppm)
    return (np.array([int(np.rint(t * float(QUANTA))) for t in iou], np.int64), np.array([(e * ppm) * (e * ppm) for e in rng], np.float64),
            np.array([math.cos(math.radians(e)) for e in hdg], np.float64))


# ------------------------------------------------------------------------------------------------------------ geometry
def box_of(cx, cy, w, h, c, s):
    """The valid box (corners [(x, y)] * 4 counter-clockwise, w, h, c^, s^) of float64 values, or None."""
    cx, cy, w, h, c, s = float(cx), float(cy), float(w), float(h), float(c), float(s)
    if not (math.isfinite(cx) and math.isfinite(cy) and math.isfinite(w) and math.isfinite(h) and math.isfinite(c) and math.isfinite(s)):
        return None
    if not (w > 0.0 and h > 0.0):
        return None
    n = c * c + s * s
    if not (math.isfinite(n) and n > 0.0):
        return None
    r = math.sqrt(n)
    ch, sh = c / r, s / r
    ux, uy, vx, vy = sh, -ch, ch, sh
    corners = [(cx - w * ux - h * vx, cy - w * uy - h * vy), (cx + w * ux - h * vx, cy + w * uy - h * vy),
               (cx + w * ux + h * vx, cy + w * uy + h * vy), (cx - w * ux + h * vx, cy - w * uy + h * vy)]
    return corners, w, h, ch, sh


def clip(pred, gt):
    """The prediction's corners clipped against the ground truth's four edges in order (Sutherland-Hodgman): a list of at most 8 vertices."""
    poly = list(pred)
    for k in range(4):
        gx, gy = gt[k]
        ex, ey = gt[(k + 1) % 4][0] - gx, gt[(k + 1) % 4][1] - gy
        side = [ex * (qy - gy) - ey * (qx - gx) for qx, qy in poly]
        out = []
        for i in range(len(poly)):
            j = (i + 1) % len(poly)
            (sx, sy), (tx, ty), dS, dE = poly[i], poly[j], side[i], side[j]
            if dS >= 0.0 and len(out) < 8:
                out.append((sx, sy))
            if (dS >= 0.0) != (dE >= 0.0) and len(out) < 8:      # (rounding cannot make a ninth vertex: it would be dropped)
                t = dS / (dS - dE)
                out.append((sx + t * (tx - sx), sy + t * (ty - sy)))
        poly = out
        if not poly:
            break
    return poly


def area(poly):
    """0.5 |sum_i cross(V_i - V_0, V_{i+1} - V_0)|, in index order."""
    total = 0.0
    for i in range(1, len(poly) - 1):
        ax, ay = poly[i][0] - poly[0][0], poly[i][1] - poly[0][1]
        bx, by = poly[i + 1][0] - poly[0][0], poly[i + 1][1] - poly[0][1]
        total = total + (ax * by - ay * bx)
    return 0.5 * abs(total)


def iou(pred, gt):
    """IoU of two boxes of box_of (None: invalid), float64; 0 where it has no meaning."""
    if pred is None or gt is None:
        return 0.0
    a = area(clip(pred[0], gt[0]))
    union = ((2.0 * pred[1]) * (2.0 * pred[2]) + (2.0 * gt[1]) * (2.0 * gt[2])) - a
    if not (a > 0.0 and union > 0.0):
        return 0.0
    q = a / union
    return q if math.isfinite(q) else 0.0


def iou_quanta(pred, gt) -> int:
    x = iou(pred, gt) * float(QUANTA)
    return QUANTA if x >= float(QUANTA) else int(np.rint(x))


def _q(x) -> int:
    """llrint(min(x, 2^32) 2^20) of a non-negative finite float64."""
    return int(np.rint((x if x < FAR else FAR) * float(QUANTA)))


def _bins_at_or_above(value, edges) -> int:
    return sum(1 for e in edges if value >= e)


# ------------------------------------------------------------------------------------------------------------ the specification
def eval_det_numpy(acc, rows, locs, typs, n, size_map, ori_map, *, ppm, centre, radius_px, iou_thresholds=IOU_THRESHOLDS,
                   range_edges_m=RANGE_EDGES_M, heading_edges_deg=HEADING_EDGES_DEG, min_score=0.1, det_score=0.2, nbins=NBINS):
    """The specification of lav_amd.ops.eval_det, same arguments (tensors or arrays), on the host: adds one frame's counters to `acc`
    (int64 array of len(DetLayout(nbins))) and returns it.  Written to be read: loops, float64 throughout."""
    lay = DetLayout(nbins)
    if not (isinstance(acc, np.ndarray) and acc.dtype == np.int64 and acc.shape == (lay.words,)):
        raise ValueError(f"acc must be an int64 array of {lay.words} words")
    rows, locs, typs = _np(rows, np.float32), _np(locs, np.float32), _np(typs, np.int32)
    size_map, ori_map = _np(size_map, np.float32), _np(ori_map, np.float32)
    H, W = size_map.shape[1:]
    D = rows.shape[1]
    n, ppm, radius_px, min_score, det_score = int(n), float(ppm), float(radius_px), float(min_score), float(det_score)
    cx0, cy0 = float(centre[0]), float(centre[1])
    L, range2, hcos = thresholds(ppm, iou_thresholds, range_edges_m, heading_edges_deg)
    L, range2, hcos = [int(v) for v in L], [float(v) for v in range2], [float(v) for v in hcos]
    f = {name: lay.view(acc, name) for name in lay.fields}
    f["frames"][...] += 1

    for c in range(2):
        # the ground truth of class c: pixel, box, range bin
        gt = {}
        for g in range(n):
            if typs[g] != c:
                continue
            px = float(locs[g, 0, 0]) * ppm + cx0
            py = float(locs[g, 0, 1]) * ppm + cy0
            if not (0.0 <= px < W and 0.0 <= py < H):
                continue
            ix, iy = min(W - 1, int(px + 0.5)), min(H - 1, int(py + 0.5))
            box = box_of(px, py, size_map[0, iy, ix], size_map[1, iy, ix], ori_map[0, iy, ix], ori_map[1, iy, ix])
            dx, dy = px - cx0, py - cy0
            rb = _bins_at_or_above(dx * dx + dy * dy, range2)
            gt[g] = (px, py, box, rb)
            f["n_gt"][c, rb] += 1
            if box is None:
                f["gt_invalid"][c] += 1

        # the rows of class c that count, their boxes and the (row, actor) table of iou_q
        live = []
        for r in range(D):
            score = rows[c, r, 0]
            if not float(score) > min_score:              # (a NaN score is skipped)
                continue
            x, y = float(rows[c, r, 1]), float(rows[c, r, 2])
            box = box_of(x, y, *rows[c, r, 3:7])
            if box is None:
                f["pred_invalid"][c] += 1
            scaled = np.float32(score) * np.float32(nbins)
            b = nbins - 1 if scaled >= np.float32(nbins - 1) else int(scaled)
            dx, dy = x - cx0, y - cy0
            live.append((r, float(score), x, y, box, b, _bins_at_or_above(dx * dx + dy * dy, range2),
                         {g: iou_quanta(box, gbox) for g, (_, _, gbox, _) in gt.items()}))

        for arm in range(1 + len(L)):
            taken = set()
            for r, score, x, y, box, b, rb_row, table in live:
                best_g, d2 = -1, None
                if arm == 0:                              # eval_frame_numpy's centre rule
                    best = np.inf
                    for g, (px, py, _, _) in gt.items():  # ascending g: a tie keeps the lowest index
                        if g in taken:
                            continue
                        this = (x - px) * (x - px) + (y - py) * (y - py)
                        if this < best:
                            best, best_g = this, g
                    if not (best_g >= 0 and best <= radius_px * radius_px):
                        best_g = -1
                    d2 = best
                else:
                    best = -1
                    for g in gt:
                        if g not in taken and table[g] > best:
                            best, best_g = table[g], g
                    if not (best_g >= 0 and best >= L[arm - 1] and best > 0):
                        best_g = -1
                hit = best_g >= 0
                if hit:
                    taken.add(best_g)
                f["hist"][arm, c, 0 if hit else 1, b] += 1
                if not score > det_score:
                    continue
                rb = gt[best_g][3] if hit else rb_row
                f["det"][arm, c, rb, 0 if hit else 1] += 1
                if arm == 0 and hit:
                    gbox = gt[best_g][2]
                    f["pairs"][c, rb] += 1
                    if box is None or gbox is None:
                        f["pair_invalid"][c] += 1
                        continue
                    f["sum_centre"][c, rb] += _q(math.sqrt(d2) / ppm)
                    f["sum_dw"][c, rb] += _q(abs(box[1] - gbox[1]) / ppm)
                    f["sum_dh"][c, rb] += _q(abs(box[2] - gbox[2]) / ppm)
                    f["sum_iou"][c, rb] += table[best_g]
                    dot = box[3] * gbox[3] + box[4] * gbox[4]
                    f["heading"][c, len(hcos) if dot != dot else sum(1 for e in hcos if dot < e)] += 1
    return acc


def summarise(acc, iou_thresholds=IOU_THRESHOLDS, range_edges_m=RANGE_EDGES_M, heading_edges_deg=HEADING_EDGES_DEG) -> dict:
    """Metrics per class from an accumulator (array or tensor) of one DetLayout; a zero denominator gives None, never a NaN.  Errors in
    metres (quanta / 2^20), IoU as a fraction.  The edges name the bins; they must be those the accumulator was filled with."""
    acc = _np(acc, np.int64)
    lay = DetLayout.of(acc)
    f = {name: lay.view(acc, name) for name in lay.fields}
    arms = ["centre"] + [f"iou{t:g}" for t in iou_thresholds]
    redges, hedges = [float(e) for e in range_edges_m], [float(e) for e in heading_edges_deg]
    rbins, hbins = len(redges) + 1, len(hedges) + 1
    range_names = [f"{lo:g}-{hi:g} m" if hi is not None else f"{lo:g}+ m" for lo, hi in zip([0.0] + redges, redges + [None])]
    heading_names = [f"{lo:g}-{hi:g} deg" for lo, hi in zip([0.0] + hedges, hedges + [180.0])]
    share = lambda row, picks: None if picks is None else _ratio(int(sum(row[b] for b in picks)), int(row.sum()))
    within10 = [b for b in range(hbins) if (hedges + [180.0])[b] <= 10.0] if 10.0 in hedges else None
    flipped = [b for b in range(hbins) if ([0.0] + hedges)[b] >= 90.0] if 90.0 in hedges else None
    out = dict(frames=int(f["frames"].reshape(-1)[0]), arms=arms, range_bins=range_names, heading_bins=heading_names, classes=[])
    for c in range(2):
        gt = int(f["n_gt"][c].sum())
        good = int(f["pairs"][c].sum()) - int(f["pair_invalid"][c])
        per_arm = {}
        for a, name in enumerate(arms):
            tp, fp = f["det"][a, c, :, 0], f["det"][a, c, :, 1]
            per_arm[name] = dict(ap=average_precision(f["hist"][a, c, 0], f["hist"][a, c, 1], gt), tp=int(tp.sum()), fp=int(fp.sum()),
                                 precision=_ratio(int(tp.sum()), int(tp.sum() + fp.sum())), recall=_ratio(int(tp.sum()), gt),
                                 per_range=[dict(precision=_ratio(int(tp[b]), int(tp[b] + fp[b])), recall=_ratio(int(tp[b]), int(f["n_gt"][c, b])))
                                            for b in range(rbins)])
        out["classes"].append(dict(
            n_gt=gt, n_gt_per_range=[int(v) for v in f["n_gt"][c, :rbins]], gt_invalid=int(f["gt_invalid"][c]), pred_invalid=int(f["pred_invalid"][c]),
            arms=per_arm, pairs=int(f["pairs"][c].sum()), pair_invalid=int(f["pair_invalid"][c]),
            mean_iou=_ratio(int(f["sum_iou"][c].sum()), QUANTA * good), mean_centre_error=_ratio(int(f["sum_centre"][c].sum()), QUANTA * good),
            mean_dw=_ratio(int(f["sum_dw"][c].sum()), QUANTA * good), mean_dh=_ratio(int(f["sum_dh"][c].sum()), QUANTA * good),
            heading_within_10deg=share(f["heading"][c], within10), heading_flipped=share(f["heading"][c], flipped),
            heading_hist=[int(v) for v in f["heading"][c, :hbins]]))
    return out


# ------------------------------------------------------------------------------------------------------------ the evaluator
PRECISIONS = ("f16x3", "bf16x6", "f32")
_TAKEN = (0, 1, 3, 4, 10, 12, 13)      # of train_lidar's tuple: lidars, num_points, sizemaps, orimaps, locs, typs, num_objs


class DetEvaluator(EvaluatorBase):
    """Runs frames of loader batches (train_lidar's tuple) through the LiDAR model's detector and accumulates their box metrics.

        ev = DetEvaluator(lidar_model, heads="both")     # a LiDARModel (or a lav_amd.train.LAV of stage "lidar")
        ev.run(loader, max_frames=None)                  # -> frames evaluated
        ev.counters()                                    # the accumulator (det_layout: one section per head path), read once

    heads: "peaks" is LiDARModel.detect(at_peaks=True), what the frame runs; "dense" the four-head path; "both" runs each frame's
    features through both into two sections.  device "cpu": eval_det_numpy on the host (EvaluatorBase)."""

    def __init__(self, lidar_model, precision=None, device=None, *, cfg=None, heads="peaks", match_radius=2.0, iou_thresholds=IOU_THRESHOLDS,
                 range_edges_m=RANGE_EDGES_M, heading_edges_deg=HEADING_EDGES_DEG, min_score=0.1, det_score=0.2, nbins=NBINS):
        from .lav import TrainConfig
        if hasattr(lidar_model, "lidar_model"):
            lidar_model, cfg = lidar_model.lidar_model, cfg or lidar_model.cfg
        cfg = cfg or TrainConfig()
        if heads not in HEADS + ("both",):
            raise ValueError(f"heads={heads!r} (peaks, dense or both)")
        self.heads = HEADS if heads == "both" else (heads,)
        self.nbins = int(nbins)
        super().__init__(lidar_model, det_layout(self.heads, self.nbins), precision, device)
        self.ppm = float(cfg.pixels_per_meter)
        H, W = int((cfg.max_x - cfg.min_x) * cfg.pixels_per_meter), int((cfg.max_y - cfg.min_y) * cfg.pixels_per_meter)
        self.centre = (W / 2 + (cfg.min_y + cfg.max_y) / 2 * cfg.pixels_per_meter, H / 2 + (cfg.min_x + cfg.max_x) / 2 * cfg.pixels_per_meter)   # LAV.bev_center
        thresholds(self.ppm, iou_thresholds, range_edges_m, heading_edges_deg)          # (refuses bad ones here, not at the first frame)
        self.edges = dict(iou_thresholds=tuple(iou_thresholds), range_edges_m=tuple(range_edges_m), heading_edges_deg=tuple(heading_edges_deg))
        self.kw = dict(ppm=self.ppm, centre=self.centre, radius_px=float(match_radius) * self.ppm, min_score=float(min_score),
                       det_score=float(det_score), nbins=self.nbins, **self.edges)
        self.frames = 0
        self._batch = None

    def upload(self, batch):
        """The clouds and the ground truth of one loader batch, uploaded once; frames index into it."""
        lidars, num_points, size, ori, locs, typs, num_objs = [torch.as_tensor(batch[i]) for i in _TAKEN]
        d = self.model_device
        self._batch = dict(lidars=lidars.to(d, torch.float32), num_points=[int(v) for v in num_points.tolist()],
                           size=size.to(d, torch.float32).contiguous(), ori=ori.to(d, torch.float32).contiguous(),
                           locs=locs.to(d, torch.float32).contiguous(), typs=typs.to(d, torch.int32).contiguous(), n=[int(v) for v in num_objs.tolist()])
        return len(self._batch["n"])

    @torch.no_grad()
    def forward(self, i) -> dict:
        """Sample i of the uploaded batch through point_pillar_net -> backbone -> detect: {head path: rows (2, 15, 7)}, in HBM."""
        from .. import ops
        b, lm = self._batch, self.model
        pts = b["lidars"][i, :b["num_points"][i]]
        with ops.precision(self.code):
            features = lm.backbone(lm.point_pillar_net([pts], [len(pts)]))
            return {h: lm.detect(features, at_peaks=h == "peaks")[0] for h in self.heads}

    def metrics(self, i, out):
        """The metrics launches of sample i, one per head path, on the rows where `forward` left them."""
        b = self._batch
        n = min(b["n"][i], b["locs"].shape[1])
        for h, rows in out.items():
            self._add("eval_det", eval_det_numpy, h, rows, b["locs"][i], b["typs"][i], n, b["size"][i], b["ori"][i], **self.kw)

    @torch.no_grad()
    def frame(self, i):
        self.metrics(i, self.forward(i))
        self.frames += 1

    def run(self, batches, max_frames=None) -> int:
        for batch, left in self._budget(batches, max_frames, lambda: self.frames):
            for i in range(self.upload(batch))[:left]:
                self.frame(i)
        return self.frames

    def precision(self) -> str:
        """The arithmetic asked for: every engine of the chain runs at it."""
        return PRECISION_NAMES.get(self.code, "default")

    def summaries(self, acc) -> dict:
        """{head path: summarise(its section)}"""
        return {h: summarise(np.asarray(acc)[self.layout.sections[h]], **self.edges) for h in self.heads}


# ------------------------------------------------------------------------------------------------------------ command line
def _build(args, cfg, device):
    """The LiDAR model alone (LAV's construction of it): the detector needs no planner, so no planner checkpoint is asked for."""
    from .. import synth
    from ..lidar import LiDARModel
    num_input = (len(cfg.seg_channels) if cfg.point_painting else 0) + cfg.num_frame_stack + 10
    model = LiDARModel(num_input=num_input, num_features=cfg.num_features, backbone=cfg.backbone, min_x=cfg.min_x, max_x=cfg.max_x,
                       min_y=cfg.min_y, max_y=cfg.max_y, pixels_per_meter=cfg.pixels_per_meter)
    model.load_state_dict(torch.load(args.lidar, map_location="cpu") if args.lidar else synth.seeded_state_dict(model, prefix="lidar."))
    model.cfg = cfg
    return model.to(device).eval()


def _batches(args, cfg):
    from .evaluate import held_out_frames
    from .synthetic import synthetic_lidar_batch
    if args.synthetic:
        return synthetic_batches(synthetic_lidar_batch, args.frames, args.batch_size, args.seed, max_points=args.max_points or cfg.max_lidar_points,
                                 num_plan=cfg.num_plan)
    return held_out_frames(args.config_path, args.data_dir, args.seed)


def _make(model, name, args):
    return DetEvaluator(model, precision=name, cfg=model.cfg, heads=args.heads, match_radius=args.match_radius, iou_thresholds=tuple(args.iou),
                        range_edges_m=tuple(args.range_edges), nbins=args.nbins)


def _line(ev, acc, args, cfg):
    note = NOTE + ("; " + SYNTHETIC_NOTE if args.synthetic else "")
    return dict(heads=args.heads, measured=list(ev.heads), match_radius_m=args.match_radius, iou_thresholds=list(args.iou),
                range_edges_m=list(args.range_edges), heading_edges_deg=list(HEADING_EDGES_DEG), note=note, summary=ev.summaries(acc))


TOOL = dict(
    name="eval_det_v2", what="eval_det", about="rotated-box IoU metrics of a LiDAR checkpoint's box and orientation heads on recorded routes",
    unit="frames", checkpoints=dict(lidar="lidar_model_dir"), precisions=PRECISIONS, batch_size=8, frames=8, synthetic="synthetic_lidar_batch samples",
    epilog=NOTE,
    flags=[("--heads", dict(default="peaks", choices=HEADS + ("both",),
                            help="which path makes the rows: peaks (lav_heads_at_peaks, what the frame runs), dense (the four-head maps, "
                                 "gathered) or both (each frame's features through both, two sections)")),
           ("--max-points", dict(type=int, default=None, help="--synthetic: points per cloud (default: the config's max_lidar_points)")),
           ("--match-radius", dict(type=float, default=2.0, help="metres within which a detection matches an actor by its centre (arm 0)")),
           ("--iou", dict(type=float, nargs="+", default=list(IOU_THRESHOLDS), metavar="T", help="up to 3 IoU thresholds (arms 1 ..)")),
           ("--range-edges", dict(type=float, nargs="+", default=list(RANGE_EDGES_M), metavar="M", help="up to 3 range edges from the ego, metres")),
           ("--nbins", dict(type=int, default=NBINS, help="bins of the score histograms"))],
    build=_build, batches=_batches, make_evaluator=_make, line=_line, contrasts=(("dense", "peaks"),),      # (--bootstrap, --heads both: paired)
    keys=("what", "heads", "measured", "precision", "data", "frames_per_s", "match_radius_m", "iou_thresholds", "range_edges_m", "heading_edges_deg",
          "note", "summary", "counters"))


def main(argv=None):
    """eval_det_v2.py: one JSON line per precision - which head path(s) it measured, the summaries, the raw counters, frames per second."""
    return run_cli(TOOL, argv)


if __name__ == "__main__":
    main()
