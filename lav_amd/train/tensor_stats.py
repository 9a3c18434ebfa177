"""--tensor-stats N of the four trainers: SAVE_DIR/tensor_stats.jsonl, and its reader.

`TensorStatsLog` is what the trainers' main drives on rank 0: behind every N-th optimiser step it takes the per-tensor rows of that step
(FusedAdam.tensor_stats(): two launches and a non-blocking copy, nothing waits) and writes them one watched step late - when the next
ones arrive, and at the end - as one JSON line:

    {"global_it", "applied", "grad_norm", "clip",
     "tensors": {name: {"numel", "grad_norm", "grad_maxabs", "grad_nonfinite", "grad_zero_frac", "weight_norm", "weight_maxabs",
                        "update_norm", "update_ratio" (= update_norm / weight_norm), "grad_hist": {"first": k, "bins": [...]}}},
     "buffers": {name: {"maxabs", "nonfinite"}}}

grad_hist holds the exponent bins (lav_amd.train.optim: bin k of 1 .. 62 is [2^(k-41), 2^(k-40))) from the first to the last one that is
not empty.  A step that was skipped becomes a line {"global_it", "skipped": [{"name", "nonfinite"}, ...], "buffers": [...]} from the
optimiser's blame ring.  A name is "{checkpoint stem}/{state_dict key}".  The file is only ever appended to: --resume goes on in it.

    python -m lav_amd.train.tensor_stats FILE.jsonl [--top K]

reads such a file on the host: per tensor the median and the last update_ratio, the tensors whose gradient was all zero in every line,
the exponent range that holds 99 % of each gradient, and every blamed step."""
from __future__ import annotations

import argparse
import json
import math
import os

import numpy as np

FILE = "tensor_stats.jsonl"


def _hist(bins):
    nz = np.flatnonzero(bins)
    if nz.size == 0:
        return dict(first=0, bins=[])
    return dict(first=int(nz[0]), bins=[int(x) for x in bins[nz[0]:nz[-1] + 1]])


def line_of(result, global_it):
    """The JSON line of one watched step from PendingTensorStats.result()."""
    names, numels, rows, wnames, wrows, glob = result
    tensors = {}
    for name, numel, r in zip(names, numels, rows):
        wn, un = math.sqrt(float(r["p_sumsq"])), math.sqrt(float(r["u_sumsq"]))
        tensors[name] = dict(numel=numel, grad_norm=math.sqrt(float(r["g_sumsq"])), grad_maxabs=float(r["g_maxabs"]), grad_nonfinite=int(r["g_nonfinite"]),
                             grad_zero_frac=int(r["g_zeros"]) / numel, weight_norm=wn, weight_maxabs=float(r["p_maxabs"]), update_norm=un,
                             update_ratio=un / wn if wn > 0 else None, grad_hist=_hist(r["hist"]))
    buffers = {name: dict(maxabs=float(r["maxabs"]), nonfinite=int(r["nonfinite"])) for name, r in zip(wnames, wrows)}
    return dict(global_it=int(global_it), applied=bool(glob["apply"]), grad_norm=math.sqrt(float(glob["sumsq"])), clip=float(glob["clip"]),
                tensors=tensors, buffers=buffers)


def digest_of(line):
    """The trainers' one-line digest of a watched step."""
    ratios = sorted((t["update_ratio"], name) for name, t in line["tensors"].items() if t["update_ratio"] is not None)
    dead = sum(1 for t in line["tensors"].values() if t["grad_zero_frac"] == 1.0)
    if not ratios:
        return f"tensor stats it {line['global_it']}: no update yet, {dead} of {len(line['tensors'])} gradients all zero"
    (lo, lo_name), (hi, hi_name) = ratios[0], ratios[-1]
    return (f"tensor stats it {line['global_it']}: update_ratio max {hi:.3e} {hi_name}, min {lo:.3e} {lo_name}; "
            f"{dead} of {len(line['tensors'])} gradients all zero")


class TensorStatsLog:
    """SAVE_DIR/tensor_stats.jsonl of one run (rank 0).  first_it: the iteration of the optimiser's first step in this process, which
    turns the blame ring's step ordinals (1, 2, ... since the optimiser was built) into iterations."""

    def __init__(self, save_dir, every, first_it=0):
        if every < 1:
            raise ValueError(f"--tensor-stats {every}: every N-th iteration, N >= 1")
        os.makedirs(save_dir, exist_ok=True)
        self.path, self.every, self.first_it = os.path.join(save_dir, FILE), int(every), int(first_it)
        self._pending = None            # (PendingTensorStats, global_it): written when the next arrives
        self._blamed = [0, 0]           # records of the two rings already written
        self._digested = None
        open(self.path, "a").close()

    def _append(self, line):
        with open(self.path, "a") as f:
            f.write(json.dumps(line) + "\n")

    def flush(self):
        if self._pending is not None:
            pending, it = self._pending
            self._pending = None
            self._append(line_of(pending.result(), it))

    def after_step(self, optimizer, global_it):
        """Behind the optimiser step of iteration global_it: at every N-th one, enqueue its rows and write the ones before."""
        if global_it % self.every:
            return
        pending = optimizer.tensor_stats()
        self.flush()
        self._pending = (pending, global_it)

    def digest(self):
        """Of the newest watched step, once (waits for its rows: called where the trainers read health() anyway); None without a new one."""
        if self._pending is None or self._pending[1] == self._digested:
            return None
        pending, it = self._pending
        self._digested = it
        return digest_of(line_of(pending.result(), it))

    def blamed(self, blame):
        """The records of FusedAdam.blame() that are new since the last call, as one line per skipped step; returns blame with every
        record's step turned into its iteration."""
        out, lines = ([], []), {}
        for k, recs in enumerate(blame):
            for rec in recs:
                rec = dict(rec, global_it=self.first_it + rec["step"] - 1)
                out[k].append(rec)
                if rec["ordinal"] >= self._blamed[k]:
                    line = lines.setdefault(rec["global_it"], dict(global_it=rec["global_it"], skipped=[], buffers=[]))
                    line["skipped" if k == 0 else "buffers"].append(dict(name=rec["name"], nonfinite=rec["nonfinite"]))
            if recs:
                lost = recs[0]["ordinal"] - self._blamed[k]
                if lost > 0:
                    self._append(dict(blame_records_lost=lost, ring="skipped" if k == 0 else "buffers"))
                self._blamed[k] = recs[-1]["ordinal"] + 1
        for it in sorted(lines):
            self._append(lines[it])
        return out

    def close(self):
        self.flush()


# ------------------------------------------------------------------------------------------------------------ the reader
def exponent_range(hist, mass=0.99):
    """(lo, hi): the narrowest run of bins first + lo .. first + hi, as exponents of two, that holds `mass` of the finite elements -
    [2^lo, 2^hi) for bins 1 .. 62; bin 0 reaches down to zero and bin 63 up to FLT_MAX."""
    bins, first = np.asarray(hist["bins"], np.int64), hist["first"]
    total = int(bins.sum())
    if total == 0:
        return None
    need, best = math.ceil(mass * total), None
    cum = np.concatenate([[0], np.cumsum(bins)])
    for a in range(len(bins)):
        b = int(np.searchsorted(cum, cum[a] + need, side="left"))
        if b <= len(bins) and (best is None or b - a < best[1] - best[0]):
            best = (a, b)
    a, b = best
    return first + a - 41, first + b - 41


def read(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def report(lines, top=10):
    steps = [ln for ln in lines if "tensors" in ln]
    blamed = [ln for ln in lines if "skipped" in ln]
    out = [f"{len(steps)} watched steps, iterations {steps[0]['global_it']} .. {steps[-1]['global_it']}" if steps else "no watched step"]
    names = list(steps[-1]["tensors"]) if steps else []
    table = []
    for name in names:
        ratios = [ln["tensors"][name]["update_ratio"] for ln in steps if name in ln["tensors"] and ln["tensors"][name]["update_ratio"] is not None]
        if ratios:
            table.append((float(np.median(ratios)), ratios[-1], name))
    table.sort(reverse=True)
    shown = table if top <= 0 or len(table) <= 2 * top else table[:top] + table[-top:]
    out.append(f"update_ratio (median, last) of {len(shown)} of {len(table)} tensors, largest median first:")
    out += [f"  {med:.3e} {last:.3e} {name}" for med, last, name in shown]
    dead = [name for name in names if all(ln["tensors"][name]["grad_zero_frac"] == 1.0 for ln in steps if name in ln["tensors"])]
    out.append(f"gradient all zero in every line: {len(dead)}")
    out += [f"  {name}" for name in dead]
    out.append("exponent range [2^lo, 2^hi) holding 99 % of each gradient (last line):")
    for name in names:
        rng = exponent_range(steps[-1]["tensors"][name]["grad_hist"])
        out.append(f"  {name}: " + ("no finite element" if rng is None else
                                   ("0" if rng[0] <= -41 else f"2^{rng[0]}") + " .. " + ("FLT_MAX" if rng[1] >= 23 else f"2^{rng[1]}")))
    out.append(f"blamed steps: {len(blamed)}")
    for ln in blamed:
        what = ", ".join(f"{r['name']} ({r['nonfinite']})" for r in ln["skipped"]) or "-"
        bufs = ", ".join(f"{r['name']} ({r['nonfinite']})" for r in ln.get("buffers", []))
        out.append(f"  it {ln['global_it']}: {what}" + (f"; buffers: {bufs}" if bufs else ""))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="read a trainer's tensor_stats.jsonl (--tensor-stats N)")
    ap.add_argument("file")
    ap.add_argument("--top", type=int, default=10, help="tensors shown at either end of the update_ratio table; 0: all")
    args = ap.parse_args(argv)
    print("\n".join(report(read(args.file), args.top)))


if __name__ == "__main__":
    main()
