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

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from .evaluate import _np, _ratio, average_precision

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
    out, at = {}, 0
    for name, shape in spec:
        size = int(np.prod(shape, dtype=np.int64))
        out[name] = section[at:at + size].reshape(shape)
        at += size
    return out


class CameraLayout:
    """The sections of one int64 accumulator, in words: one 68-word section per name in `maps` (lav_eval_seg's) and, when `nbins` is
    given, one of 6 + 2 nbins words called "scores" (lav_eval_scores's).  csrc/eval_camera.hip and include/lav_amd.h have the words."""

    def __init__(self, maps, nbins=NBINS):
        if nbins is not None and not 1 <= int(nbins) <= 1024:
            raise ValueError(f"{nbins} score bins (1 .. 1024)")
        self.maps = tuple(maps)
        self.nbins = None if nbins is None else int(nbins)
        if SCORES in self.maps or len(set(self.maps)) != len(self.maps):
            raise ValueError(f"section names {self.maps}")
        self.sections, at = {}, 0
        for name in self.maps:
            self.sections[name] = slice(at, at + SEG_WORDS)
            at += SEG_WORDS
        if self.nbins is not None:
            self.sections[SCORES] = slice(at, at + SCORE_HEAD + 2 * self.nbins)
            at += SCORE_HEAD + 2 * self.nbins
        self.words = at

    def __len__(self):
        return self.words

    def zeros(self) -> np.ndarray:
        return np.zeros(self.words, np.int64)

    def view(self, acc, name):
        """The named section of `acc` (array or tensor): a view, so that adding to it adds to `acc`."""
        return acc[self.sections[name]]

    def kind(self, name) -> str:
        """What `fields` is to make of the named section: SCORES for the score section, "seg" for a map's."""
        return SCORES if name == SCORES else "seg"

    def fields(self, acc, name) -> dict:
        """The named, shaped views of the named section of `acc` (array)."""
        return fields(self.view(acc, name), self.kind(name))

    def named(self, acc) -> dict:
        """The raw counters as nested lists per section (the JSON output)."""
        acc = np.asarray(acc)
        return {name: {k: v.tolist() for k, v in self.fields(acc, name).items()} for name in self.sections}

    def unnamed(self, counters: dict) -> np.ndarray:
        """The accumulator `named` was made from."""
        acc = self.zeros()
        for name in self.sections:
            for k, v in self.fields(acc, name).items():
                v[...] = np.asarray(counters[name][k], np.int64)
        return acc


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


def _precision_code(name):
    from .. import _lib, ops
    if name is None:
        return ops.frame_precision()
    if isinstance(name, int):
        return name
    return {"f16x3": _lib.CONV_F16X3, "bf16x6": _lib.CONV_BF16X6, "f32": _lib.CONV_F32}[name]


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
    names = {{3: "f16x3", 2: "bf16x6", 1: "f32"}.get(int(l.desc.precision), default) for l in layers}
    if names == {"f16x3"} and not e["f16"]:
        names = {"f16x3 without its scale hand-off"}
    return "/".join(sorted(names))


def erfnet_arithmetic(erfnet, shape) -> str:
    """What the ERFNet's runs of blocks ran at on a call of `shape` (B, 3, H, W), read off the engine that call built: f16x3 only if
    every persistent run is the fp16 one AND takes the shape (else the blocks fall back to their own bf16x6 launches); f32 under
    LAV_CONV_PRECISION=f32, whatever ops.precision says."""
    if _env_f32():
        return "f32"
    B, _, H, W = shape
    device = next(erfnet.parameters()).device
    chains = [s.chain for s in erfnet._eng[1] if getattr(s, "chain", None) is not None]
    stride = {16: 2, 64: 4, 128: 8}
    for c in chains:
        ch = c.pairs[0].ch
        like = torch.empty(1, device=device).expand(B, ch, H // stride[ch], W // stride[ch])      # (no memory: only its shape is read)
        if not (c.f16 and c.supported(like)):
            return "bf16x6"
    return "f16x3" if chains else "bf16x6"


# ------------------------------------------------------------------------------------------------------------ the evaluators
class _Evaluator:
    """What the two evaluators share: where the accumulator lives.  device "cpu" keeps it on the host and calls the NumPy
    specifications on copies of the tensors the kernels would have read (the models still run on the GPU: there is no CPU inference
    path); that is how the tests capture what the kernels saw."""

    def __init__(self, model, layout, precision, device):
        self.model = model.eval()
        self.model_device = next(model.parameters()).device
        self.device = torch.device(device) if device is not None else self.model_device
        self.code = _precision_code(precision)
        self.layout = layout
        self.acc = torch.zeros(len(layout), dtype=torch.int64, device=self.device)
        self.in_force = set()

    def _seg(self, name, logits, labels, scale):
        from .. import ops
        if self.device.type == "cpu":
            eval_seg_numpy(self.layout.view(self.acc.numpy(), name), logits, labels, scale)
        else:
            ops.eval_seg(self.layout.view(self.acc, name), logits, labels, scale)

    def precision(self) -> str:
        """The arithmetic that was in force over the calls so far."""
        return "+".join(sorted(self.in_force)) or "none"

    def counters(self) -> np.ndarray:
        return self.acc.cpu().numpy()


class SegEvaluator(_Evaluator):
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
            self.in_force.add(erfnet_arithmetic(self.model.erfnet, part.shape))
            self._seg("seg", logits, labels[j:j + self.images_per_call], 1)
        self.images += x.shape[0]

    def run(self, batches, max_images=None) -> int:
        for rgb, sem in batches:
            left = None if max_images is None else max_images - self.images
            if left is not None and left <= 0:
                break
            self.batch(rgb, sem, left)
        return self.images


class BrakeEvaluator(_Evaluator):
    """Runs the 'bra' loader's batches (rgb, tel_rgb uint8 HWC, sem, tel_sem uint8 labels, bra flags) through an
    RGBBrakePredictionModel, frame by frame at batch 1 as the frame pipeline does: x1 = trunk(wide), x2 = trunk(tele),
    pred = classify(x1, x2), and the two segmentation heads at stride 4.  The heads' confusion matrices go to the sections "wide" and
    "tele" (scale 4: the up-sampled logits of train_bra's loss never exist), the score against the frame's flag to "scores" at the
    agent's threshold (layout BRA)."""

    def __init__(self, bra_model, precision=None, device=None, threshold=0.1):
        super().__init__(bra_model, BRA, precision, device)
        self.threshold = float(threshold)
        self.frames = 0

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
            self._seg("wide", logit1, sem[i:i + 1], SEG_SCALE)
            self._seg("tele", logit2, tel_sem[i:i + 1], SEG_SCALE)
            if self.device.type == "cpu":
                eval_scores_numpy(self.layout.view(self.acc.numpy(), SCORES), pred, flags[i:i + 1], self.threshold, self.layout.nbins)
            else:
                ops.eval_scores(self.layout.view(self.acc, SCORES), pred.contiguous(), flags[i:i + 1], self.threshold, self.layout.nbins)
        self.frames += wide.shape[0]

    def run(self, batches, max_frames=None) -> int:
        for batch in batches:
            left = None if max_frames is None else max_frames - self.frames
            if left is not None and left <= 0:
                break
            self.batch(*batch, limit=left)
        return self.frames


# ------------------------------------------------------------------------------------------------------------ command line
_WHAT = dict(
    seg=dict(key="seg_model_dir", unit="images", precisions=SEG_PRECISIONS, batch=24,
             about="held-out metrics of a camera segmenter checkpoint (seg_*.th) on recorded routes"),
    bra=dict(key="bra_model_dir", unit="frames", precisions=BRA_PRECISIONS, batch=8,
             about="held-out metrics of a brake-net checkpoint (bra_*.th) on recorded routes"))


def _checkpoint(what, args):
    """The checkpoint file: the flag's, else the config's `seg_model_dir` / `bra_model_dir`; None for --synthetic without the flag
    (seeded weights).  A named file that does not exist is an error, never a silent fall back to seeded weights."""
    key, path = _WHAT[what]["key"], getattr(args, what)
    if path:
        if not os.path.isfile(path):
            raise SystemExit(f"--{what} {path}: no such file (the checkpoint the config calls `{key}`)")
        return path
    if args.synthetic:
        return None
    import yaml
    with open(args.config_path, "r") as f:
        rel = (yaml.safe_load(f) or {}).get(key)
    if not rel:
        raise SystemExit(f"{args.config_path} has no `{key}` and --{what} was not given")
    cands = [rel, os.path.join(os.path.dirname(os.path.abspath(args.config_path)), rel)]
    hit = next((c for c in cands if os.path.isfile(c)), None)
    if hit is None:
        raise SystemExit(f"checkpoint `{key}: {rel}` of {args.config_path} not found (tried {cands}); pass --{what} PATH, or --synthetic "
                         "for seeded random weights on synthetic images")
    return hit


def _synthetic_batches(what, frames, seed, batch_size, num_classes):
    from .synthetic import synthetic_bra_batch, synthetic_seg_batch
    done = 0
    while done < frames:
        b = min(batch_size, frames - done)
        yield (synthetic_seg_batch if what == "seg" else synthetic_bra_batch)(b, seed=seed + 1009 * done, num_classes=num_classes)
        done += b


def main(what, argv=None):
    """eval_seg.py ("seg") / eval_bra_v2.py ("bra"): one JSON line per precision - the summary, the raw counters and the images or
    frames per second of the evaluation.  Single process, no augmentation, the loader in order and to its last sample.  The rate is
    the whole run's, set-up included: a precision's first call builds and packs its engines, the first line also starts the loader's
    workers.  On a short run it measures that set-up, and it is not comparable between the lines of --precision all; the forwards
    and the metrics launches alone are timed by tools/eval_camera_probe.py."""
    from .. import synth
    from ..rgb import RGBBrakePredictionModel, RGBSegmentationModel
    from .brake import BRA_LABELS
    from .run import load_config
    w = _WHAT[what]
    unit = w["unit"]
    ap = argparse.ArgumentParser(description=w["about"], epilog=f"{unit}_per_s in the output is the whole run's rate, engine build, weight packing and "
                                 "loader start-up included: it says how long an evaluation takes, not how fast an arithmetic is")
    ap.add_argument("--config-path", default=None, help="the reference's config_v2.yaml; required unless --synthetic")
    ap.add_argument("--data-dir", default=None, help="held-out routes; overrides the config's data_dir")
    ap.add_argument(f"--{what}", default=None, help=f"{what}_*.th (default: the config's {w['key']})")
    ap.add_argument("--precision", default=None, choices=w["precisions"] + ("all",),
                    help="arithmetic of the convolutions, of what ops.precision switches in this net (default: the frame's); all: the same "
                         f"{unit} once per choice." + (" Exact fp32: the same command under LAV_CONV_PRECISION=f32" if what == "seg" else ""))
    ap.add_argument(f"--max-{unit}", type=int, default=None, dest="max_units")
    ap.add_argument("--batch-size", type=int, default=w["batch"], help="loader batch; inference is per "
                    + ("call of three images" if what == "seg" else "frame"))
    ap.add_argument("--num-workers", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2021)
    ap.add_argument("--synthetic", action="store_true", help="synthetic images and seeded random weights (smoke runs)")
    ap.add_argument("--frames", type=int, default=6, help=f"--synthetic: how many {unit}")
    ap.add_argument("--out", default=None, metavar="FILE", help="also write the JSON there")
    args = ap.parse_args(argv)
    tool = "eval_seg" if what == "seg" else "eval_bra_v2"
    if not args.synthetic and not args.config_path:
        raise SystemExit("recorded routes are read from --data-dir or the data_dir of --config-path (or pass --synthetic)")
    path = _checkpoint(what, args)
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: no GPU visible; the models have no CPU inference path")
    device = torch.device("cuda", torch.cuda.current_device())
    cfg = load_config(args.config_path, seed=args.seed)
    torch.manual_seed(cfg.seed)
    if what == "seg":
        model, k = RGBSegmentationModel(cfg.seg_channels), len(cfg.seg_channels) + 1
    else:
        model, k = RGBBrakePredictionModel(list(BRA_LABELS)), len(BRA_LABELS) + 1
    model.load_state_dict(torch.load(path, map_location="cpu") if path else synth.seeded_state_dict(model, prefix=f"{what}."))
    model.to(device).eval()
    if args.synthetic:
        data = f"{args.frames} synthetic {unit}"
        batches = lambda: _synthetic_batches(what, args.frames, args.seed, args.batch_size, k)
    else:
        from ..data.datasets import LOADERS
        ds = LOADERS[what](args.config_path, seed=args.seed, overrides=dict(data_dir=args.data_dir) if args.data_dir else None)
        if len(ds) == 0:
            raise SystemExit(f"no recorded {unit} under {args.data_dir or 'the data_dir of ' + args.config_path}")
        data = f"{len(ds)} recorded {unit}"
        batches = lambda: torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=False, drop_last=False, num_workers=args.num_workers)
    lines = []
    for name in (w["precisions"] if args.precision == "all" else (args.precision,)):
        ev = SegEvaluator(model, precision=name) if what == "seg" else BrakeEvaluator(model, precision=name)
        t0 = time.perf_counter()
        n = ev.run(batches(), args.max_units)
        acc = ev.counters()                      # (the one copy; it also waits for the last launch)
        dt = time.perf_counter() - t0
        ran = ev.precision()
        if any(line["precision"] == ran for line in lines):      # (e.g. a shape the fp16 runs do not take, LAV_CONV_PRECISION=f32)
            print(f"{tool}: --precision {name} ran at {ran}, which is already printed; no second line", file=sys.stderr)
            continue
        line = {"what": tool, "precision": ran, "asked": name, "data": data, f"{unit}_per_s": round(n / max(dt, 1e-9), 2)}
        if what == "seg":
            line["summary"] = summarise_seg(SEG.view(acc, "seg"), k)
        else:
            line["summary"] = dict(threshold=ev.threshold, brake=summarise_scores(BRA.view(acc, SCORES)),
                                   wide=summarise_seg(BRA.view(acc, "wide"), k), tele=summarise_seg(BRA.view(acc, "tele"), k))
        line["counters"] = ev.layout.named(acc)
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return lines
