"""Held-out metrics of the two camera checkpoints the agent loads (eval_seg.py, eval_bra_v2.py).

seg_{e}.th is the agent's `seg_model_dir` and what data_paint.py runs over every frame of every route; bra_{e}.th decides
`pred_bra > 0.1`, the emergency brake.  The trainers print a loss on (optionally augmented) training batches; this module measures a
checkpoint on routes it never trained on: the segmenter's confusion matrix (IoU, accuracy, precision / recall per class), the brake
net's precision / recall at the agent's threshold and its AP, and the confusion matrices of the brake net's two segmentation heads.
The nets run as the agent runs them (eval-mode engines under ops.precision); their outputs stay in HBM, where one launch per call
(lav_eval_seg, lav_eval_scores: lav_amd.ops.eval_seg / eval_scores) ADDS integer counters into a section of one int64 accumulator
that is read once, at the end.  `eval_seg_numpy` and `eval_scores_numpy` below are those kernels' specifications, and the kernels
equal them in every word (tests/test_gpu_eval_camera.py).

The reference has no evaluator (its answer to "which epoch do I drive with" is closed-loop CARLA): the metric definitions are this
project's, and parity of them with a reference is UNPINNED because there is nothing to pin it to.  What is pinned: the kernels to
these specifications, the specifications to hand-derived counters and to torch's own nearest up-sampling
(tests/test_eval_camera_host.py).

Definitions (DESIGN 4.7h has the reasons):
  segmentation  label pixel (y, x) of labels (n, h * scale, w * scale) is judged by logit pixel (y // scale, x // scale) of logits
                (n, k, h, w): F.interpolate(logits, scale_factor=scale) (nearest) followed by argmax - what train_bra's loss and its
                pred_sem1/2 mean - without the up-sampled logits.  The prediction is the FIRST maximum (p = 0; for c in 1 .. k - 1: if
                x[c] > x[p]: p = c; a NaN never wins).  A logit pixel with a channel that is not finite adds its scale^2 label pixels
                to `nonfinite` and to nothing else; otherwise a label >= k adds 1 to `ignored` and to nothing else; otherwise
                conf[label][prediction] += 1.  68 words whatever k is: images, pixels, ignored, nonfinite, conf [8][8].
  scores        per sample: samples += 1; a NaN or infinite score adds to `nonfinite` and to nothing else; otherwise
                at[flag != 0][float64(score) > threshold] += 1 and hist[flag != 0][bin] += 1 with
                bin = clamp(int(float32(score) * float32(nbins)), 0, nbins - 1), lav_eval_frame's rule.  6 + 2 nbins words.

Arithmetic.  ops.precision(...) switches the brake net's ResNet-18 trunk between f16x3, bf16x6 and exact fp32 inside one process.  Of the
ERFNet it switches the persistent runs of blocks only, between f16x3 and bf16x6 (and f16x3 needs a call the runs take: B * h within the
chip's workgroups, widths of 32 / 64 / 128 at the runs' strides - the agent's three 288 x 256 images are); its exact-fp32 path is chosen
by LAV_CONV_PRECISION=f32 in the environment, which the library reads once.  So `--precision` offers what it really switches, every
JSON line records the arithmetic that was IN FORCE, and the exact-fp32 evaluation of the segmenter is the same command under
LAV_CONV_PRECISION=f32.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .eval_common import AccLayout, EvaluatorBase, PRECISION_NAMES, _np, _ratio, average_precision, run_cli, synthetic_batches

SEG_WORDS = 68
MAX_CLASSES = 8
SCORE_HEAD = 6
NBINS = 256
SEG_FIELDS = (("images", ()), ("pixels", ()), ("ignored", ()), ("nonfinite", ()), ("conf", (MAX_CLASSES, MAX_CLASSES)))
SCORES = "scores"


def _score_fields(nbins):
    return (("samples", ()), ("nonfinite", ()), ("at", (2, 2)), ("hist", (2, int(nbins))))


def fields(section, kind) -> dict:
    """The named, shaped views of one section (array) of the given kind - "seg": a map's 68 words, SCORES: a score section's
    6 + 2 nbins -: adding to a view adds to the section.  The kind is always said, never guessed from the length: 68 words are
    also a score section of 31 bins."""
    n = len(section)
    if kind == "seg":
        if n != SEG_WORDS:
            raise ValueError(f"a map section of {n} words ({SEG_WORDS})")
        spec = SEG_FIELDS
    elif kind == SCORES:
        nbins = (n - SCORE_HEAD) // 2
        if n != SCORE_HEAD + 2 * nbins or not 1 <= nbins <= 1024:
            raise ValueError(f"a score section of {n} words (6 + 2 nbins, 1 .. 1024 bins)")
        spec = _score_fields(nbins)
    else:
        raise ValueError(f"section kind {kind!r}")
    return AccLayout(((kind, kind, spec),), sectioned=True).fields(section, kind)


class CameraLayout(AccLayout):
    """The sections of one int64 accumulator, in words: one 68-word section per name in `maps` (lav_eval_seg's, kind "seg") and, when
    `nbins` is given, one of 6 + 2 nbins words called "scores" (lav_eval_scores's, kind SCORES).  csrc/eval_camera.hip and
    include/lav_amd.h have the words."""

    def __init__(self, maps, nbins=NBINS):
        if nbins is not None and not 1 <= int(nbins) <= 1024:
            raise ValueError(f"{nbins} score bins (1 .. 1024)")
        self.maps = tuple(maps)
        self.nbins = None if nbins is None else int(nbins)
        if SCORES in self.maps or len(set(self.maps)) != len(self.maps):
            raise ValueError(f"section names {self.maps}")
        scores = () if self.nbins is None else ((SCORES, SCORES, _score_fields(self.nbins)),)
        super().__init__(tuple((name, "seg", SEG_FIELDS) for name in self.maps) + scores, sectioned=True)


SEG = CameraLayout(("seg",), nbins=None)
BRA = CameraLayout(("wide", "tele"), nbins=NBINS)


# ------------------------------------------------------------------------------------------------------------ the specifications
def eval_seg_numpy(section, logits, labels, scale=1):
    """The specification of lav_amd.ops.eval_seg, same arguments (tensors or arrays), on the host: adds the counters of one batch to
    `section` (int64 array of 68 words) and returns it."""
    if not (isinstance(section, np.ndarray) and section.dtype == np.int64 and section.shape == (SEG_WORDS,)):
        raise ValueError(f"the section must be an int64 array of {SEG_WORDS} words")
    logits, labels, scale = _np(logits, np.float32), _np(labels, np.uint8), int(scale)
    if logits.ndim != 4 or not 2 <= logits.shape[1] <= MAX_CLASSES or scale not in (1, 2, 4, 8):
        raise ValueError(f"logits {logits.shape} at scale {scale}")
    n, k, h, w = logits.shape
    if labels.shape != (n, h * scale, w * scale):
        raise ValueError(f"labels {labels.shape} for logits {logits.shape} at scale {scale}")
    f = fields(section, "seg")
    x = logits.astype(np.float64)
    # the first maximum: a later channel wins only where it is GREATER (a comparison with a NaN is false)
    pred, best = np.zeros((n, h, w), np.int64), x[:, 0].copy()
    for c in range(1, k):
        with np.errstate(invalid="ignore"):
            wins = x[:, c] > best
        pred[wins], best[wins] = c, x[:, c][wins]
    bad = ~np.isfinite(x).all(axis=1)
    up = lambda a: a.repeat(scale, axis=1).repeat(scale, axis=2)        # nearest: label pixel (y, x) <- logit pixel (y // scale, x // scale)
    pred, bad = up(pred), up(bad)
    f["images"][...] += n
    f["pixels"][...] += labels.size
    f["nonfinite"][...] += int(bad.sum())
    f["ignored"][...] += int((~bad & (labels >= k)).sum())
    for label in range(k):
        for p in range(k):
            f["conf"][label, p] += int((~bad & (labels == label) & (pred == p)).sum())
    return section


def score_bin(score, nbins):
    """clamp(int(float32(score) * float32(nbins)), 0, nbins - 1) of a finite score, the comparisons in float32 (no int() of an Inf)."""
    with np.errstate(over="ignore"):
        scaled = np.float32(score) * np.float32(nbins)
    if scaled >= np.float32(nbins - 1):
        return nbins - 1
    return 0 if scaled < np.float32(0) else int(scaled)


def eval_scores_numpy(section, scores, flags, threshold, nbins):
    """The specification of lav_amd.ops.eval_scores, same arguments, on the host: adds to `section` (int64 array of 6 + 2 nbins words)."""
    nbins = int(nbins)
    if not 1 <= nbins <= 1024:
        raise ValueError(f"{nbins} score bins (1 .. 1024)")
    if not (isinstance(section, np.ndarray) and section.dtype == np.int64 and section.shape == (SCORE_HEAD + 2 * nbins,)):
        raise ValueError(f"the section must be an int64 array of {SCORE_HEAD + 2 * nbins} words")
    scores, flags, threshold = _np(scores, np.float32), _np(flags, np.uint8), float(threshold)
    if scores.ndim != 1 or flags.shape != scores.shape or threshold != threshold:
        raise ValueError(f"scores {scores.shape}, flags {flags.shape}, threshold {threshold}")
    f = fields(section, SCORES)
    for score, flag in zip(scores, flags):
        f["samples"][...] += 1
        if not np.isfinite(score):
            f["nonfinite"][...] += 1
            continue
        positive = 1 if flag != 0 else 0
        f["at"][positive, 1 if float(score) > threshold else 0] += 1
        f["hist"][positive, score_bin(score, nbins)] += 1
    return section


# ------------------------------------------------------------------------------------------------------------ summaries
def summarise_seg(section, k: int) -> dict:
    """Metrics of one map section over its first k classes; a zero denominator gives None, never a NaN.  IoU of class c =
    conf[c, c] / (row c + column c - conf[c, c]); the mean is over the classes that have one."""
    f = fields(_np(section, np.int64), "seg")
    conf = f["conf"][:k, :k]
    rows, cols, diag = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    iou = [_ratio(diag[c], rows[c] + cols[c] - diag[c]) for c in range(k)]
    have = [i for i in iou if i is not None]
    return dict(images=int(f["images"]), pixels=int(f["pixels"]), iou=iou, mean_iou=float(np.mean(have)) if have else None,
                accuracy=_ratio(diag.sum(), conf.sum()), precision=[_ratio(diag[c], cols[c]) for c in range(k)],
                recall=[_ratio(diag[c], rows[c]) for c in range(k)], labelled=[int(r) for r in rows], ignored=int(f["ignored"]),
                nonfinite=int(f["nonfinite"]))


def summarise_scores(section) -> dict:
    """Metrics of a score section: the counts at the threshold, precision / recall / F1 / accuracy there, and the AP of the histogram
    (evaluate.average_precision: true positives = the positives' bins, false positives = the negatives')."""
    f = fields(_np(section, np.int64), SCORES)
    at, hist = f["at"], f["hist"]
    tn, fp, fn, tp = int(at[0, 0]), int(at[0, 1]), int(at[1, 0]), int(at[1, 1])
    positives, negatives = int(hist[1].sum()), int(hist[0].sum())
    return dict(samples=int(f["samples"]), positives=positives, negatives=negatives, tp=tp, fp=fp, fn=fn, tn=tn,
                precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn), f1=_ratio(2 * tp, 2 * tp + fp + fn),
                accuracy=_ratio(tp + tn, tp + tn + fp + fn), ap=average_precision(hist[1], hist[0], positives), nonfinite=int(f["nonfinite"]))


# ------------------------------------------------------------------------------------------------------------ arithmetic
SEG_PRECISIONS = ("f16x3", "bf16x6")
BRA_PRECISIONS = ("f16x3", "bf16x6", "f32")


def _env_f32():
    return os.environ.get("LAV_CONV_PRECISION", "") in ("f32", "fp32")


def trunk_arithmetic(resnet, code: int) -> str:
    """What the brake net's ResNet-18 ran at under ops.precision(code), read off the engine that call built
    (ResNet._engine: one engine per precision): the `precision` every packed layer's descriptor carries - 0 being the library's
    default, bf16x6 unless LAV_CONV_PRECISION=f32 -, and for f16x3 the engine's scale hand-off as well.  Layers that disagree are
    reported as such, joined by "/".  (f16x3 is the library's mode of that name: the layers whose plan is the split kernel run on two
    fp16 pieces, the others on their exact-fp32 kernels.)"""
    e = (getattr(resnet, "_eng", None) or {}).get(("trunk", int(code)))
    if e is None:
        raise RuntimeError(f"the trunk has no engine for precision code {code}: it did not run under it")
    layers = [e["stem"]] + [l for b in e["blocks"] for l in (b["c1"], b["c2"], b["down"]) if l is not None]
    default = "f32" if _env_f32() else "bf16x6"
    names = {PRECISION_NAMES.get(int(l.desc.precision), default) for l in layers}
    if names == {"f16x3"} and not e["f16"]:
        names = {"f16x3 without its scale hand-off"}
    return "/".join(sorted(names))


def erfnet_arithmetic(erfnet, code: int, shape) -> str:
    """What the ERFNet's runs of blocks ran at on a call of `shape` (B, 3, H, W) under ops.precision(code), read off the engine that call built: f16x3 only if
    every persistent run is the fp16 one AND takes the shape (else the blocks fall back to their own bf16x6 launches); f32 under
    LAV_CONV_PRECISION=f32, whatever ops.precision says."""
    if _env_f32():
        return "f32"
    B, _, H, W = shape
    device = next(erfnet.parameters()).device
    chains = erfnet.chains(int(code))
    stride = {16: 2, 64: 4, 128: 8}
    for c in chains:
        ch = c.pairs[0].ch
        like = torch.empty(1, device=device).expand(B, ch, H // stride[ch], W // stride[ch])      # (no memory: only its shape is read)
        if not (c.f16 and c.supported(like)):
            return "bf16x6"
    return "f16x3" if chains else "bf16x6"


# ------------------------------------------------------------------------------------------------------------ the evaluators
class SegEvaluator(EvaluatorBase):
    """Runs the 'seg' loader's batches (rgb (B, H, W, 3) uint8 RGB, sem (B, H, W) labels) through an RGBSegmentationModel and adds
    the confusion matrix of its logits.

        ev = SegEvaluator(seg_model)         # in HBM; precision: None (the frame's), "f16x3", "bf16x6" or a lav_conv precision code
        ev.run(loader, max_images=None)      # -> images evaluated
        ev.counters()                        # the accumulator (layout SEG), read once

    The net is called on `images_per_call` images at a time: the agent's call is its three cameras, and the persistent ERFNet runs
    need B * h within the chip's workgroups, which a training-size batch is not."""

    def __init__(self, seg_model, precision=None, device=None, images_per_call=3):
        super().__init__(seg_model, SEG, precision, device)
        self.images_per_call = max(1, int(images_per_call))
        self.images = 0
        self._ahead = 0

    def units(self) -> int:
        """The images of the calls before this one (EvaluatorBase.resample's rows: a call's images land in one row)."""
        return self.images + self._ahead

    @torch.no_grad()
    def batch(self, rgb, sem, limit=None):
        from .. import ops
        if limit is not None:
            rgb, sem = rgb[:limit], sem[:limit]
        d = self.model_device
        x = ops.image_u8_to_f32(torch.as_tensor(rgb).to(torch.uint8).to(d), reverse=False)        # (the loader already yields RGB)
        labels = torch.as_tensor(sem).to(torch.uint8).to(d).contiguous()
        for j in range(0, x.shape[0], self.images_per_call):
            part = x[j:j + self.images_per_call]
            with ops.precision(self.code):
                logits = self.model(part)
            self.in_force.add(erfnet_arithmetic(self.model.erfnet, self.code, part.shape))
            self._ahead = j
            self._add("eval_seg", eval_seg_numpy, "seg", logits, labels[j:j + self.images_per_call], 1)
        self._ahead = 0
        self.images += x.shape[0]

    def run(self, batches, max_images=None) -> int:
        for (rgb, sem), left in self._budget(batches, max_images, lambda: self.images):
            self.batch(rgb, sem, left)
        return self.images


class BrakeEvaluator(EvaluatorBase):
    """Runs the 'bra' loader's batches (rgb, tel_rgb uint8 HWC, sem, tel_sem uint8 labels, bra flags) through an
    RGBBrakePredictionModel, frame by frame at batch 1 as the frame pipeline does: x1 = trunk(wide), x2 = trunk(tele),
    pred = classify(x1, x2), and the two segmentation heads at stride 4.  The heads' confusion matrices go to the sections "wide" and
    "tele" (scale 4: the up-sampled logits of train_bra's loss never exist), the score against the frame's flag to "scores" at the
    agent's threshold (layout BRA)."""

    def __init__(self, bra_model, precision=None, device=None, threshold=0.1):
        super().__init__(bra_model, BRA, precision, device)
        self.threshold = float(threshold)
        self.frames = 0
        self._ahead = 0

    def units(self) -> int:
        """The frames before the one whose three launches are being added (EvaluatorBase.resample's rows)."""
        return self.frames + self._ahead

    @torch.no_grad()
    def batch(self, rgb, tel_rgb, sem, tel_sem, bra, limit=None):
        from .. import ops
        from .brake import SEG_SCALE
        d, m = self.model_device, self.model
        cut = (lambda t: torch.as_tensor(t)[:limit]) if limit is not None else torch.as_tensor
        wide = ops.image_u8_to_f32(cut(rgb).to(torch.uint8).to(d), reverse=False)
        tele = ops.image_u8_to_f32(cut(tel_rgb).to(torch.uint8).to(d), reverse=False)
        sem, tel_sem = cut(sem).to(torch.uint8).to(d).contiguous(), cut(tel_sem).to(torch.uint8).to(d).contiguous()   # uploaded once per batch
        flags = (cut(bra) != 0).to(torch.uint8).to(d)
        for i in range(wide.shape[0]):
            with ops.precision(self.code):
                x1, x2 = m.trunk(wide[i:i + 1]), m.trunk(tele[i:i + 1])
                pred = m.classify(x1, x2)
                logit1, logit2 = m.seg_head(x1).float().contiguous(), m.seg_head(x2).float().contiguous()
            if pred is None:
                raise RuntimeError("BrakeEvaluator: the brake net has no fused classifier path here (eval mode, in HBM, batch 1)")
            self.in_force.add(trunk_arithmetic(m.conv_backbone, self.code))
            self._ahead = i
            self._add("eval_seg", eval_seg_numpy, "wide", logit1, sem[i:i + 1], SEG_SCALE)
            self._add("eval_seg", eval_seg_numpy, "tele", logit2, tel_sem[i:i + 1], SEG_SCALE)
            self._add("eval_scores", eval_scores_numpy, SCORES, pred.contiguous(), flags[i:i + 1], self.threshold, self.layout.nbins)
        self._ahead = 0
        self.frames += wide.shape[0]

    def run(self, batches, max_frames=None) -> int:
        for batch, left in self._budget(batches, max_frames, lambda: self.frames):
            self.batch(*batch, limit=left)
        return self.frames


# ------------------------------------------------------------------------------------------------------------ command line
def _build(what):
    def build(args, cfg, device):
        from .. import synth
        from ..rgb import RGBBrakePredictionModel, RGBSegmentationModel
        from .brake import BRA_LABELS
        model = RGBSegmentationModel(cfg.seg_channels) if what == "seg" else RGBBrakePredictionModel(list(BRA_LABELS))
        path = getattr(args, what)
        model.load_state_dict(torch.load(path, map_location="cpu") if path else synth.seeded_state_dict(model, prefix=f"{what}."))
        return model.to(device).eval()
    return build


def _classes(what, cfg):
    from .brake import BRA_LABELS
    return len(cfg.seg_channels if what == "seg" else BRA_LABELS) + 1


def _batches(what):
    def batches(args, cfg):
        from . import synthetic
        from ..data.datasets import LOADERS
        if args.synthetic:
            return synthetic_batches(getattr(synthetic, f"synthetic_{what}_batch"), args.frames, args.batch_size, args.seed, num_classes=_classes(what, cfg))
        return LOADERS[what](args.config_path, seed=args.seed, overrides=dict(data_dir=args.data_dir) if args.data_dir else None)
    return batches


def _seg_line(ev, acc, args, cfg):
    return dict(summary=summarise_seg(SEG.view(acc, "seg"), _classes("seg", cfg)))


def _bra_line(ev, acc, args, cfg):
    k = _classes("bra", cfg)
    return dict(summary=dict(threshold=ev.threshold, brake=summarise_scores(BRA.view(acc, SCORES)), wide=summarise_seg(BRA.view(acc, "wide"), k),
                             tele=summarise_seg(BRA.view(acc, "tele"), k)))


def _tool(what, name, unit, **own):
    """What eval_seg and eval_bra_v2 have in common of eval_common.run_cli's description.  {unit}_per_s is the whole run's rate, set-up
    included: a precision's first call builds and packs its engines, the first line also starts the loader's workers.  On a short run it
    measures that set-up, and it is not comparable between the lines of --precision all; the forwards and the metrics launches alone
    are timed by tools/eval_camera_probe.py."""
    return dict(name=name, unit=unit, checkpoints={what: f"{what}_model_dir"}, frames=6, synthetic="synthetic images", dedupe=True,
                epilog=f"{unit}_per_s in the output is the whole run's rate, engine build, weight packing and loader start-up included: it says how "
                       "long an evaluation takes, not how fast an arithmetic is",
                build=_build(what), batches=_batches(what), keys=("what", "precision", "asked", "data", f"{unit}_per_s", "summary", "counters"), **own)


_PRECISION_HELP = ("arithmetic of the convolutions, of what ops.precision switches in this net (default: the frame's); all: the same {unit} "
                   "once per choice.")
_WHAT = dict(
    seg=_tool("seg", "eval_seg", "images", precisions=SEG_PRECISIONS, batch_size=24,
              about="held-out metrics of a camera segmenter checkpoint (seg_*.th) on recorded routes",
              help=dict(precision=_PRECISION_HELP.format(unit="images") + " Exact fp32: the same command under LAV_CONV_PRECISION=f32",
                        batch_size="loader batch; inference is per call of three images"),
              make_evaluator=lambda model, name, args: SegEvaluator(model, precision=name), line=_seg_line),
    bra=_tool("bra", "eval_bra_v2", "frames", precisions=BRA_PRECISIONS, batch_size=8,
              about="held-out metrics of a brake-net checkpoint (bra_*.th) on recorded routes", help=dict(precision=_PRECISION_HELP.format(unit="frames")),
              make_evaluator=lambda model, name, args: BrakeEvaluator(model, precision=name), line=_bra_line))


def main(what, argv=None):
    """eval_seg.py ("seg") / eval_bra_v2.py ("bra"): one JSON line per arithmetic that was in force (eval_common.run_cli)."""
    return run_cli(_WHAT[what], argv)
