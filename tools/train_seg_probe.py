#!/usr/bin/env python3
"""train_seg step time: LAV(what="seg").train_seg on 288 x 256 synthetic images at batch 32 and 256, the training kernels
(default) against LAV_TRAIN_CONV=torch (every block on torch / MIOpen), interleaved A B A B ..., plus GPU kernels per step
(torch.profiler).  Prints one line per measurement and a JSON summary; writes it to the path given with --out.

    python tools/train_seg_probe.py [--batches 32,256] [--rounds 3] [--steps 3] [--out profiles/train_seg_probe.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lav_amd.train import TrainConfig  # noqa: E402
from lav_amd.train.lav import LAV  # noqa: E402
from lav_amd.train.synthetic import synthetic_seg_batch  # noqa: E402

PATHS = {"hip": "hip", "torch": "torch"}


def set_path(name):
    os.environ["LAV_TRAIN_CONV"] = PATHS[name]


def timed(lav, batch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        lav.train_seg(*batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernels_per_step(lav, batch):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            lav.train_seg(*batch)
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.device_type.name == "CUDA")
    except Exception as e:      # (the count is informative only)
        print("kernel count unavailable:", e, flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = dict(device=torch.cuda.get_device_name(0), image="288x256", results={})
    for B in [int(b) for b in a.batches.split(",")]:
        lav = LAV(TrainConfig(), dev, what="seg")
        batch = synthetic_seg_batch(B, seed=2021, device=dev)
        res = {n: [] for n in PATHS}
        for n in PATHS:              # warm-up of each path (MIOpen's solver search, the library's first launches)
            set_path(n)
            timed(lav, batch, 1)
        for r in range(a.rounds):
            for n in PATHS:
                set_path(n)
                ms = timed(lav, batch, a.steps)
                res[n].append(round(ms, 2))
                print(f"batch {B} round {r} {n}: {ms:.2f} ms/step", flush=True)
        launches = {}
        for n in PATHS:
            set_path(n)
            launches[n] = kernels_per_step(lav, batch)
        out["results"][str(B)] = dict(ms_per_step=res, median_ms={n: sorted(v)[len(v) // 2] for n, v in res.items()}, kernels_per_step=launches,
                                      peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
        del lav, batch
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    os.environ.pop("LAV_TRAIN_CONV", None)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
