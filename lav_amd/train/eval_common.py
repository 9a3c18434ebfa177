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


# ------------------------------------------------------------------------------------------------------------ resampling
RESAMPLE_TAG = 0x52534D50          # "RSMP": counter word 2 of the draws
RESAMPLE_MAX_ROWS = 1 << 20        # lav_eval_resample's cap (ops.EVAL_RESAMPLE_MAX_ROWS)
RESAMPLE_MAX_BYTES = 4 << 30       # of a row table


def eval_resample_numpy(rows, B, seed) -> np.ndarray:
    """The specification of lav_eval_resample (lav_amd.ops.eval_resample): block-bootstrap replicates of a row table.  rows (R, W)
    int64, one row of counters per block of consecutive units -> (B + 1, W) int64:
        out[0] = rows.sum(0)                                      the identity replicate, no draws: the run's own accumulator
        out[b] = sum over j < R of rows[idx(b, j)]                b = 1 .. B
        idx(b, j) = (u * R) >> 32 as a 64-bit product, u = word j & 3 of Philox4x32-10 (lav_amd.data.augment.philox4x32) at counter
                    (j >> 2, b, 0x52534D50, 0) and key (seed low word, seed high word).
    The multiply-high map is not exactly uniform: 2^32 words fall into R bins of floor(2^32 / R) or one more, so a row's probability is off
    by at most R / 2^32 of itself - below 2.5e-4 at the cap of 2^20 rows.  All sums are int64 sums modulo 2^64: integer addition is
    associative, so the kernel's split of the work gives these bits, and overflow is excluded as it is for the accumulators themselves."""
    rows = np.ascontiguousarray(_np(rows, np.int64))
    if rows.ndim != 2 or not 1 <= rows.shape[0] <= RESAMPLE_MAX_ROWS or rows.shape[1] < 1:
        raise ValueError(f"eval_resample: rows of shape {rows.shape} (1 .. 2^20 rows of at least one word)")
    R, W = rows.shape
    B, seed = int(B), int(seed) & 0xFFFFFFFFFFFFFFFF
    out = np.empty((B + 1, W), np.int64)
    out[0] = rows.sum(axis=0)
    step = max(1, (1 << 22) // (R * W))          # replicates per gather: at most 2^22 words at a time
    for b0 in range(1, B + 1, step):
        b = np.arange(b0, min(b0 + step, B + 1), dtype=np.int64)
        out[b] = rows[resample_indices(R, b, seed)].sum(axis=1)
    return out


def resample_indices(R, b, seed) -> np.ndarray:
    """idx(b, j) of eval_resample_numpy for the replicates `b` (an array of numbers >= 1) and j < R: (len(b), R) int64."""
    from ..data.augment import philox4x32
    j, b = np.arange(int(R), dtype=np.int64), np.asarray(b, np.int64)
    words = np.stack(philox4x32((j >> 2)[None, :], b[:, None], RESAMPLE_TAG, 0, int(seed) & 0xFFFFFFFFFFFFFFFF))       # (4, replicates, R)
    u = np.take_along_axis(words, np.broadcast_to((j & 3)[None, None, :], (1,) + words.shape[1:]), axis=0)[0]
    return ((u.astype(np.uint64) * np.uint64(R)) >> np.uint64(32)).astype(np.int64)


def interval(values, B, level):
    """The percentile interval of one leaf over the replicates where it is defined: `values` sorted ascending as v, n of them,
    lo = v[floor((1 - P) / 2 (n - 1))], hi = v[ceil((1 + P) / 2 (n - 1))] - order statistics, no interpolation, the positions computed
    exactly (P as the decimal it was written as).  None for n < B / 2 (or none at all), [lo, hi, n] for n < B, [lo, hi] otherwise."""
    from fractions import Fraction
    import math
    v = sorted(float(x) for x in values)
    n = len(v)
    if n == 0 or 2 * n < B:
        return None
    P = Fraction(str(level))
    lo, hi = v[math.floor((1 - P) / 2 * (n - 1))], v[math.ceil((1 + P) / 2 * (n - 1))]
    return [lo, hi, n] if n < B else [lo, hi]


def _float_leaves(tree, path=()):
    """The paths of a summary's leaves that are a float or None (ints, bools and strings are left out); lists are walked by index."""
    if isinstance(tree, dict):
        for k, v in tree.items():
            yield from _float_leaves(v, path + (k,))
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from _float_leaves(v, path + (i,))
    elif tree is None or isinstance(tree, float):
        yield path


def _leaf(tree, path):
    """The number at `path` of a replicate's summary, or None where it is not defined there."""
    for k in path:
        if isinstance(tree, dict):
            tree = tree.get(k)
        elif isinstance(tree, (list, tuple)) and isinstance(k, int) and k < len(tree):
            tree = tree[k]
        else:
            return None
    return float(tree) if isinstance(tree, (int, float)) and not isinstance(tree, bool) else None


def _grow(entries, like):
    """{path: entry} as a tree in the shape of `like`: dicts stay dicts, a list stays a list where every position has an entry and
    becomes {index: entry} where some have not; what has no entry at all is left out."""
    def walk(node, path):
        if path in entries:
            return True, entries[path]
        if isinstance(node, dict):
            kids = {k: walk(v, path + (k,)) for k, v in node.items()}
            kept = {k: e for k, (has, e) in kids.items() if has}
            return bool(kept), kept
        if isinstance(node, (list, tuple)):
            kids = [walk(v, path + (i,)) for i, v in enumerate(node)]
            if kids and all(has for has, _ in kids):
                return True, [e for _, e in kids]
            kept = {str(i): e for i, (has, e) in enumerate(kids) if has}
            return bool(kept), kept
        return False, None
    return walk(like, ())[1]


def interval_tree(point, replicates, B, level, minus=None):
    """The intervals of every float-or-None leaf of the summary `point` over `replicates` (the summaries of replicates 1 .. B), as a
    tree in the shape of `point`.  minus = (point', replicates'): the intervals of point - point' instead, over the float-or-None leaves
    the two have in common, replicate b of the one against replicate b of the other - a paired difference."""
    paths = list(_float_leaves(point))
    if minus is not None:
        theirs = set(_float_leaves(minus[0]))
        paths = [p for p in paths if p in theirs]
    entries = {}
    for p in paths:
        if minus is None:
            vals = [_leaf(r, p) for r in replicates]
        else:
            vals = [None if a is None or b is None else a - b for a, b in ((_leaf(r, p), _leaf(s, p)) for r, s in zip(replicates, minus[1]))]
        entries[p] = interval([v for v in vals if v is not None], B, level)
    return _grow(entries, point)


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
        self.table = None

    def resample(self, block, units):
        """Opt in, before run(): the accumulator becomes a zeroed (ceil(units / block), W) int64 table on self.device, one row per block
        of consecutive units, and self.acc the row in use (a contiguous view: the metric kernels and specifications see an accumulator).
        The row rule, _add's: with u = units() finished before the call, the next row is opened at u once u - (the u at which the row in
        use was opened) >= block.  Every launch of one frame lands in one row; a launch over a group of 8 frames lands whole in the row of
        its first frame, so rows hold block .. block + (group - 1) units, the last one possibly fewer, and none is empty.  `units`: how
        many run() will be given at most (the table's size)."""
        L, N, W = int(block), int(units), len(self.layout)
        if L < 1 or N < 1:
            raise ValueError(f"resample: blocks of {L} units over {N} units (--block and the units must be at least 1)")
        rows = -(-N // L)
        if rows > RESAMPLE_MAX_ROWS:
            raise ValueError(f"resample: {N} units in blocks of {L} are {rows} rows, more than 2^20 (the draws' index rule): raise --block")
        if rows * W * 8 > RESAMPLE_MAX_BYTES:
            raise ValueError(f"resample: {rows} rows of {W} words are more than 4 GiB: raise --block")
        self.table = torch.zeros((rows, W), dtype=torch.int64, device=self.device)
        self.block, self._opened = L, []
        self.acc = self.table[0]

    def units(self) -> int:
        """The units (frames, images: what run() returns) finished before the call that asks."""
        return self.frames

    def _row(self):
        u = self.units()
        if self._opened and u - self._opened[-1] < self.block:
            return
        if len(self._opened) == self.table.shape[0]:
            raise RuntimeError(f"resample: more than the {self.table.shape[0]} x {self.block} units resample() was told of")
        self.acc = self.table[len(self._opened)]
        self._opened.append(u)

    def row_table(self):
        """(the used rows of the table, the units each holds) of resample mode."""
        used = len(self._opened)
        return self.table[:used], np.diff(np.asarray(self._opened + [self.units()], np.int64))

    def replicates(self, B, seed) -> np.ndarray:
        """(B + 1, W) on the host: eval_resample_numpy's replicates of the used rows, by lav_amd.ops.eval_resample where the table is in
        HBM."""
        from .. import ops
        table = self.row_table()[0]
        if self.device.type == "cpu":
            return eval_resample_numpy(table.numpy(), B, seed)
        return ops.eval_resample(table, B, seed).cpu().numpy()

    def _add(self, kernel, spec, section, *args, **kw):
        """One call's counters, added to the accumulator (section None) or to its named section: by lav_amd.ops.<kernel> where it is
        in HBM, by the specification `spec` on the host.  In resample mode the accumulator is the row the call belongs to."""
        from .. import ops
        if self.table is not None:
            self._row()
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
        """The run's accumulator on the host; in resample mode the column sums of the used rows, the same bits."""
        if self.table is not None:
            return self.row_table()[0].sum(dim=0).cpu().numpy()
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


def _resample_flags(ap, unit):
    """run_cli's own flags, the same for every tool (parser(tool) keeps the tool's)."""
    ap.add_argument("--bootstrap", type=int, default=0, metavar="B",
                    help="B block-bootstrap replicates: every line gains `resample`, a percentile interval for each float of its summary "
                         "(default 0: off, the lines are what they are without it)")
    ap.add_argument("--block", type=int, default=32, metavar="L",
                    help=f"--bootstrap: {unit} per resampled block (default 32, a choice and not a measurement); blocks should span the "
                         "correlation length of the drive - consecutive 20 Hz frames are not independent, and blocks shorter than "
                         "their correlation give intervals that are too narrow")
    ap.add_argument("--level", type=float, default=0.95, metavar="P", help="--bootstrap: the intervals' nominal coverage (default 0.95)")
    ap.add_argument("--rows-out", default=None, metavar="FILE.npz",
                    help="--bootstrap: also write the per-block record there (table, row_units, block, words): what the worst blocks of a route "
                         "are found from offline")


def _resample_entry(tool, ev, reps, summary, ran, first, args, cfg):
    """(a line's `resample` entry, what a later line of --precision all is compared with).  The replicates' summaries are the tool's own
    line() of their accumulators; `contrasts` are paired differences inside the line (the tool names the pairs of summary keys), `vs` the
    paired difference to the first line, replicate b against replicate b: the same seed and the same row_units draw the same blocks."""
    B = args.bootstrap
    row_units = ev.row_table()[1]
    summaries = [tool["line"](ev, reps[b], args, cfg)["summary"] for b in range(1, B + 1)]
    entry = dict(replicates=B, block=args.block, blocks=len(row_units), units_per_block=[int(row_units.min()), int(row_units.max())],
                 seed=args.seed, level=args.level, ci=interval_tree(summary, summaries, B, args.level))
    pairs = [(a, b) for a, b in tool.get("contrasts", ()) if a in summary and b in summary]
    if pairs:
        entry["contrasts"] = {f"{a} − {b}": interval_tree(summary[a], [s[a] for s in summaries], B, args.level,
                                                                 minus=(summary[b], [s[b] for s in summaries])) for a, b in pairs}
    if first is None:
        return entry, (ran, row_units, summary, summaries)
    if np.array_equal(row_units, first[1]):
        entry["vs"] = dict(precision=first[0], diff=interval_tree(summary, summaries, B, args.level, minus=(first[2], first[3])))
    else:
        entry["vs"] = dict(precision=first[0], note=f"not paired: this run filled {len(row_units)} blocks of {int(row_units.sum())} {tool['unit']}, the "
                                                    f"first line's {len(first[1])} of {int(first[1].sum())}, or cut them elsewhere")
    return entry, first


def run_cli(tool, argv=None, optional=(), echo=True):
    """One evaluation tool's main: one JSON line per precision - the tool's summary, the raw counters and the frames (images) per
    second of the evaluation, the whole run's, engine build and loader start-up included.  Single process, no augmentation, the
    loader in order and to its last sample.  `tool` describes what is the tool's own:
        name, about, unit ("frames" / "images"), checkpoints {flag: config key}, precisions, batch_size, frames (defaults), synthetic
        (help), flags [(flag, add_argument keywords)], keys (the JSON line's, in order), dedupe (no second line for an arithmetic
        that was already in force)
        build(args, cfg, device) -> the model(s), from the checkpoint paths (or None: seeded weights) the driver left in args
        batches(args, cfg) -> the recorded dataset, or under --synthetic an iterator of batches
        make_evaluator(model, name, args), line(ev, acc, args, cfg) -> the tool's own keys of the line
        contrasts ((a, b), ...): pairs of summary keys whose paired difference --bootstrap reports.
    --bootstrap B, --block L, --level P, --rows-out FILE (added here, the same for every tool): the evaluator runs in resample mode
    (EvaluatorBase.resample), lav_eval_resample draws B block-bootstrap replicates of its row table, and every line gains `resample` =
    {replicates, block, blocks, units_per_block [min, max], seed, level, ci, contrasts, vs} with `ci` a tree of [lo, hi] in the shape of
    the summary (interval_tree: percentile block-bootstrap intervals of ratio-of-sums estimators, nothing more); summary and counters
    are those of replicate 0, the bits they have without the flag.
    optional: checkpoint flags that stay None when they are not given, the config is not asked (the trainers' validation: the teacher
    rides in uniplanner_*.th); echo False: the lines are returned and not printed."""
    from .run import load_config
    ap = parser(tool)
    _resample_flags(ap, tool["unit"])
    args = ap.parse_args(argv)
    name, unit = tool["name"], tool["unit"]
    if args.bootstrap < 0 or args.block < 1 or not 0.0 < args.level < 1.0:
        raise SystemExit(f"--bootstrap {args.bootstrap} --block {args.block} --level {args.level}: replicates >= 0, blocks of >= 1 {unit}, 0 < level < 1")
    if args.rows_out and not args.bootstrap:
        raise SystemExit("--rows-out writes the row table of --bootstrap B (B > 0)")
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
    most = args.frames if args.synthetic else len(ds)
    most = most if args.max_units is None else min(most, args.max_units)
    lines, first, tables = [], None, {}
    for asked in (tool["precisions"] if args.precision == "all" else (args.precision,)):
        ev = tool["make_evaluator"](model, asked, args)
        if args.bootstrap:
            try:
                ev.resample(args.block, most)
            except ValueError as e:
                raise SystemExit(f"{name}: {e}")
        t0 = time.perf_counter()
        n = ev.run(batches(), args.max_units)
        acc = ev.counters()                      # (the one copy; it also waits for the last launch)
        dt = time.perf_counter() - t0
        ran = ev.precision()
        if tool.get("dedupe") and any(line["precision"] == ran for line in lines):      # (e.g. a shape the fp16 runs do not take, LAV_CONV_PRECISION=f32)
            print(f"{name}: --precision {asked} ran at {ran}, which is already printed; no second line", file=sys.stderr)
            continue
        if args.bootstrap:
            reps = ev.replicates(args.bootstrap, args.seed)
            acc = reps[0]                        # (the identity replicate: the column sums, the bits `acc` had)
        have = {"what": tool.get("what", name), "precision": ran, "asked": asked, "data": data, "batch_size": args.batch_size,
                f"{unit}_per_s": round(n / max(dt, 1e-9), 2), "counters": ev.layout.named(acc), **tool["line"](ev, acc, args, cfg)}
        line = {k: have[k] for k in tool["keys"]}
        if args.bootstrap:
            line["resample"], first = _resample_entry(tool, ev, reps, have["summary"], ran, first, args, cfg)
            table, row_units = ev.row_table()
            suffix = "" if not tables else f"_{ran}"
            tables.update({"table" + suffix: table.cpu().numpy(), "row_units" + suffix: row_units})
        lines.append(line)
        if echo:
            print(json.dumps(line), flush=True)
    if args.rows_out:
        with open(args.rows_out, "wb") as f:          # (np.savez would add .npz to a name without it)
            np.savez(f, block=np.int64(args.block), words=np.int64(len(ev.layout)), **tables)
    if args.out:
        with open(args.out, "w") as f:
            f.writelines(json.dumps(one) + "\n" for one in lines)
    return lines
