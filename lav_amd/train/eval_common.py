"""What the evaluation tools share (eval_full_v2, eval_seg, eval_bra_v2, eval_bev_v2, eval_drive_v2, eval_distill_v2, eval_det_v2): the layout of an int64
accumulator, the evaluator base, the checkpoint rule and the command-line driver.  evaluate.py, evaluate_camera.py, evaluate_bev.py,
evaluate_drive.py, evaluate_distill.py and evaluate_det.py keep what is
their own: the metric definitions, the NumPy specification, the summaries, the model's upload / frame / batch code and one description
of their command line (run_cli's `tool`)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

QUANTA = 1 << 20            # quanta per metre of the distance sums
FAR = 2.0 ** 32             # metres; a distance that is not below it makes its plan / forecast "non-finite"
NUM_CMDS = 6


# ------------------------------------------------------------------------------------------------------------ the layout
class AccLayout:
    """One int64 accumulator as named, shaped slices, in words.  `spec` is ((name, shape), ...) in order - a flat layout, whose
    `fields` is the table name -> (slice, shape) and whose `view` gives a shaped field - or, sectioned, ((section, kind,
    ((name, shape), ...)), ...): `sections` is section -> slice, `view` gives a section's words and `fields(acc, section)` its shaped
    fields.  A section's kind is named in the spec and never read off its length: 68 words are a map section and also a score section
    of 31 bins."""

    def __init__(self, spec, sectioned=False):
        self.sections, self.kinds, self._table, at = {}, {}, {}, 0
        for section, kind, fields in (spec if sectioned else ((None, None, spec),)):
            start, table = at, {}
            for name, shape in fields:
                size = int(np.prod(shape, dtype=np.int64))
                table[name] = (slice(at - start, at - start + size), shape)       # within its section
                at += size
            self.sections[section], self.kinds[section], self._table[section] = slice(start, at), kind, table
        self.words = at
        if not sectioned:
            self.fields = self._table[None]

    def __len__(self):
        return self.words

    def zeros(self) -> np.ndarray:
        return np.zeros(self.words, np.int64)

    def _fields(self, acc, section=None) -> dict:
        if section is not None:
            acc = acc[self.sections[section]]
        return {name: acc[sl].reshape(shape) for name, (sl, shape) in self._table[section].items()}

    def view(self, acc, name):
        """The named field, shaped (flat), or the named section's words (sectioned), of `acc` (array or tensor): a view, so that
        adding to it adds to `acc`."""
        if None in self._table:
            sl, shape = self._table[None][name]
            return acc[sl].reshape(shape)
        return acc[self.sections[name]]

    def fields(self, acc, section) -> dict:
        """The named, shaped views of the named section of `acc`.  (A flat layout's `fields` is its table instead.)"""
        return self._fields(acc, section)

    def kind(self, section) -> str:
        return self.kinds[section]

    def named(self, acc) -> dict:
        """The raw counters as nested lists, per section where there are sections (the JSON output)."""
        acc = np.asarray(acc)
        per = {section: {k: v.tolist() for k, v in self._fields(acc, section).items()} for section in self._table}
        return per.get(None, per)

    def unnamed(self, counters: dict) -> np.ndarray:
        """The accumulator `named` was made from."""
        acc = self.zeros()
        for section in self._table:
            for k, v in self._fields(acc, section).items():
                v[...] = np.asarray((counters if section is None else counters[section])[k], np.int64)
        return acc


# ------------------------------------------------------------------------------------------------------------ the specifications' helpers
def _np(t, dtype):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t), dtype=dtype)


def _quanta(a, b):
    """q_t of (T, 2) float32 points against their targets, or None where a distance is not below FAR."""
    d = a.astype(np.float64) - b.astype(np.float64)
    with np.errstate(all="ignore"):
        dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        if not (dist < FAR).all():
            return None
        return np.rint(dist * float(QUANTA)).astype(np.int64)


def _ratio(a, b):
    return None if b == 0 else float(a) / float(b)


def average_precision(tp_hist, fp_hist, n_gt):
    """AP from the score histograms.  The rule: walk the bins from the highest score down, accumulating true and false positives; after
    every bin that holds a detection there is an operating point (recall = TP / n_gt, precision = TP / (TP + FP)); the precision at a
    point is replaced by the largest precision at that or any LOWER-score point (the monotone envelope); AP is the area under the
    resulting recall steps, sum over points of (recall - previous recall) * envelope precision, with recall 0 before the first point.
    None when there is no ground truth."""
    if n_gt == 0:
        return None
    tp = fp = 0
    points = []
    for b in range(len(tp_hist) - 1, -1, -1):
        if tp_hist[b] == 0 and fp_hist[b] == 0:
            continue
        tp, fp = tp + int(tp_hist[b]), fp + int(fp_hist[b])
        points.append((tp / n_gt, tp / (tp + fp)))
    env = 0.0
    for i in range(len(points) - 1, -1, -1):
        env = max(env, points[i][1])
        points[i] = (points[i][0], env)
    ap, prev = 0.0, 0.0
    for recall, prec in points:
        ap += (recall - prev) * prec
        prev = recall
    return ap


# ------------------------------------------------------------------------------------------------------------ the evaluator base
PRECISION_NAMES = {3: "f16x3", 2: "bf16x6", 1: "f32"}      # lav_conv.precision codes (_lib.CONV_*)


def precision_code(name):
    """The lav_conv precision code of a name, of a code, or of None (the frame's)."""
    from .. import _lib, ops
    if name is None:
        return ops.frame_precision()
    if isinstance(name, int):
        return name
    return {"f16x3": _lib.CONV_F16X3, "bf16x6": _lib.CONV_BF16X6, "f32": _lib.CONV_F32}[name]


class EvaluatorBase:
    """What the evaluators share: where the accumulator lives.  device "cpu" keeps it on the host and calls the NumPy specification
    on copies of the tensors the kernel would have read (the models still run on the GPU: there is no CPU inference path); that is
    how the tests capture what the kernels saw."""

    def __init__(self, model, layout, precision, device):
        self.model = model.eval()
        self.model_device = next(model.parameters()).device
        self.device = torch.device(device) if device is not None else self.model_device
        self.code = precision_code(precision)
        self.layout = layout
        self.acc = torch.zeros(len(layout), dtype=torch.int64, device=self.device)
        self.in_force = set()

    def _add(self, kernel, spec, section, *args, **kw):
        """One call's counters, added to the accumulator (section None) or to its named section: by lav_amd.ops.<kernel> where it is
        in HBM, by the specification `spec` on the host."""
        from .. import ops
        on_host = self.device.type == "cpu"
        acc = self.acc.numpy() if on_host else self.acc
        if section is not None:
            acc = self.layout.view(acc, section)
        (spec if on_host else getattr(ops, kernel))(acc, *args, **kw)

    def _budget(self, batches, most, done):
        """(batch, how many more units may be taken: None for no limit) for the loader's batches until done() reaches `most`."""
        for batch in batches:
            left = None if most is None else most - done()
            if left is not None and left <= 0:
                break
            yield batch, left

    def precision(self) -> str:
        """The arithmetic that was in force over the calls so far."""
        return "+".join(sorted(self.in_force)) or "none"

    def counters(self) -> np.ndarray:
        return self.acc.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ data
class SeededFrames(torch.utils.data.Dataset):
    """dataset[idx] with NumPy's and torch's generators seeded from (seed, idx) first: what a sample draws (the point shuffle, once the
    jitters are 0) then depends on the sample alone, not on which worker loads it or on what was loaded before."""

    def __init__(self, dataset, seed):
        self.dataset, self.seed = dataset, int(seed)

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        s = (self.seed * 1000003 + int(idx) * 7919 + 12345) % (1 << 32)
        np.random.seed(s)
        torch.manual_seed(s)
        return self.dataset[idx]


def synthetic_batches(make, frames, batch_size, seed, **kw):
    """`frames` samples of make(b, seed=..., **kw) (a lav_amd.train.synthetic.synthetic_*_batch) in batches of `batch_size`."""
    done = 0
    while done < frames:
        b = min(batch_size, frames - done)
        yield make(b, seed=seed + 1009 * done, **kw)
        done += b


# ------------------------------------------------------------------------------------------------------------ command line
def config_checkpoint(config_path, key, flag_name, given, synthetic, purpose, why=""):
    """The checkpoint file a run starts from: `given` (the flag's), else the config's `key`, as written or beside the config; None for
    --synthetic without the flag (seeded weights).  A named file that does not exist is an error, never a silent fall back to seeded
    weights.  `purpose` ends the sentence about --synthetic, `why` the one about a config without the key."""
    if given:
        if not os.path.isfile(given):
            raise SystemExit(f"--{flag_name} {given}: no such file (the checkpoint the config calls `{key}`)")
        return given
    if synthetic:
        return None
    import yaml
    with open(config_path, "r") as f:
        rel = (yaml.safe_load(f) or {}).get(key)
    if not rel:
        raise SystemExit(f"{config_path} has no `{key}` and --{flag_name} was not given{why}")
    cands = [rel, os.path.join(os.path.dirname(os.path.abspath(config_path)), rel)]
    hit = next((c for c in cands if os.path.isfile(c)), None)
    if hit is None:
        raise SystemExit(f"checkpoint `{key}: {rel}` of {config_path} not found (tried {cands}); pass --{flag_name} PATH, or --synthetic {purpose}")
    return hit


def parser(tool) -> argparse.ArgumentParser:
    """The command line of one tool: the shared flags, with the tool's defaults and help, and its own."""
    unit, h = tool["unit"], tool.get("help", {})
    ap = argparse.ArgumentParser(description=tool["about"], epilog=tool.get("epilog"))
    ap.add_argument("--config-path", default=None, help="the reference's config_v2.yaml; required unless --synthetic")
    ap.add_argument("--data-dir", default=None, help="held-out routes; overrides the config's data_dir")
    for flag, key in tool["checkpoints"].items():
        ap.add_argument(f"--{flag}", default=None, help=f"{flag}_*.th (default: the config's {key})")
    ap.add_argument("--precision", default=None, choices=tool["precisions"] + ("all",),
                    help=h.get("precision", f"arithmetic of the convolutions (default: the frame's); all: the same {unit} three times, three summaries"))
    ap.add_argument(f"--max-{unit}", type=int, default=None, dest="max_units")
    ap.add_argument("--batch-size", type=int, default=tool["batch_size"], help=h.get("batch_size", "loader batch; inference is per frame"))
    ap.add_argument("--num-workers", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2021)
    ap.add_argument("--synthetic", action="store_true", help=f"{tool['synthetic']} and seeded random weights (smoke runs)")
    ap.add_argument("--frames", type=int, default=tool["frames"], help=f"--synthetic: how many {unit}")
    for flag, kw in tool.get("flags", ()):
        ap.add_argument(flag, **kw)
    ap.add_argument("--out", default=None, metavar="FILE", help="also write the JSON there")
    return ap


def held_out_units(tool, config_path, data_dir, seed=2021):
    """How many of the tool's units (frames / images) its loader finds under `data_dir`, with the loaders' keys of `config_path`: what the
    trainers' --val-data-dir asks before the first step."""
    from .run import load_config
    args = argparse.Namespace(synthetic=False, config_path=config_path, data_dir=data_dir, seed=seed)
    return len(tool["batches"](args, load_config(config_path, seed=seed)))


def run_cli(tool, argv=None, optional=(), echo=True):
    """One evaluation tool's main: one JSON line per precision - the tool's summary, the raw counters and the frames (images) per
    second of the evaluation, the whole run's, engine build and loader start-up included.  Single process, no augmentation, the
    loader in order and to its last sample.  `tool` describes what is the tool's own:
        name, about, unit ("frames" / "images"), checkpoints {flag: config key}, precisions, batch_size, frames (defaults), synthetic
        (help), flags [(flag, add_argument keywords)], keys (the JSON line's, in order), dedupe (no second line for an arithmetic
        that was already in force)
        build(args, cfg, device) -> the model(s), from the checkpoint paths (or None: seeded weights) the driver left in args
        batches(args, cfg) -> the recorded dataset, or under --synthetic an iterator of batches
        make_evaluator(model, name, args), line(ev, acc, args, cfg) -> the tool's own keys of the line.
    optional: checkpoint flags that stay None when they are not given, the config is not asked (the trainers' validation: the teacher
    rides in uniplanner_*.th); echo False: the lines are returned and not printed."""
    from .run import load_config
    args = parser(tool).parse_args(argv)
    name, unit = tool["name"], tool["unit"]
    if not args.synthetic and not args.config_path:
        raise SystemExit("recorded routes are read from --data-dir or the data_dir of --config-path (or pass --synthetic)")
    if args.batch_size < 1:
        raise SystemExit(f"--batch-size {args.batch_size}")
    for flag, key in tool["checkpoints"].items():
        if flag in optional and not getattr(args, flag):
            continue
        setattr(args, flag, config_checkpoint(args.config_path, key, flag, getattr(args, flag), args.synthetic,
                                              f"for seeded random weights on {tool['synthetic']}"))
    if not torch.cuda.is_available():
        raise SystemExit(f"{name}: no GPU visible; the models have no CPU inference path")
    device = torch.device("cuda", torch.cuda.current_device())
    cfg = load_config(args.config_path, seed=args.seed)
    torch.manual_seed(cfg.seed)
    model = tool["build"](args, cfg, device)
    if args.synthetic:
        data = f"{args.frames} synthetic {unit}"
        batches = lambda: tool["batches"](args, cfg)
    else:
        ds = tool["batches"](args, cfg)
        if len(ds) == 0:
            raise SystemExit(f"no recorded {unit} under {args.data_dir or 'the data_dir of ' + args.config_path}")
        data = f"{len(ds)} recorded {unit}"
        batches = lambda: torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=False, drop_last=False, num_workers=args.num_workers)
    lines = []
    for asked in (tool["precisions"] if args.precision == "all" else (args.precision,)):
        ev = tool["make_evaluator"](model, asked, args)
        t0 = time.perf_counter()
        n = ev.run(batches(), args.max_units)
        acc = ev.counters()                      # (the one copy; it also waits for the last launch)
        dt = time.perf_counter() - t0
        ran = ev.precision()
        if tool.get("dedupe") and any(line["precision"] == ran for line in lines):      # (e.g. a shape the fp16 runs do not take, LAV_CONV_PRECISION=f32)
            print(f"{name}: --precision {asked} ran at {ran}, which is already printed; no second line", file=sys.stderr)
            continue
        have = {"what": tool.get("what", name), "precision": ran, "asked": asked, "data": data, "batch_size": args.batch_size,
                f"{unit}_per_s": round(n / max(dt, 1e-9), 2), "counters": ev.layout.named(acc), **tool["line"](ev, acc, args, cfg)}
        line = {k: have[k] for k in tool["keys"]}
        lines.append(line)
        if echo:
            print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.writelines(json.dumps(one) + "\n" for one in lines)
    return lines
