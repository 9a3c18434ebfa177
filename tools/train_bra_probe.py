#!/usr/bin/env python3
"""train_bra step time: BrakeTrainer.train_bra on 288 x 768 + 192 x 480 synthetic images at batch 52 and 8, the configurations
below interleaved A B C ... per round, plus peak memory and GPU kernels per step (torch.profiler); and, with --ops, the two new
operations alone (forward + backward) against the torch ops they replace at the step's batch-52 shapes.  Prints one line per
measurement and a JSON summary; writes it to the path given with --out.

    python tools/train_bra_probe.py [--batches 52,8] [--rounds 3] [--steps 3] [--ops] [--out profiles/train_bra_probe.json]

Configurations (environment of hipnn.brake_piece_on):
    default      nothing set: the measured defaults
    torch        LAV_TRAIN_CONV=torch: the all-torch step
    hip_bf16x6   LAV_TRAIN_CONV=hip: trunk, attention and loss on liblav_amd, convolutions in bf16x6
    hip_f16x3    the same with LAV_TRAIN_PRECISION=f16x3
    kernels      LAV_TRAIN_BRA=attn,xent: attention and loss on liblav_amd, the trunk on torch
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lav_amd.train import BrakeTrainer, TrainConfig, hipnn, synthetic_bra_batch  # noqa: E402

CONFIGS = {"default": {}, "torch": {"LAV_TRAIN_CONV": "torch"}, "hip_bf16x6": {"LAV_TRAIN_CONV": "hip", "LAV_TRAIN_PRECISION": "bf16x6"},
           "hip_f16x3": {"LAV_TRAIN_CONV": "hip", "LAV_TRAIN_PRECISION": "f16x3"}, "kernels": {"LAV_TRAIN_BRA": "attn,xent"}}
KEYS = ("LAV_TRAIN_CONV", "LAV_TRAIN_PRECISION", "LAV_TRAIN_BRA")


def set_config(name):
    for k in KEYS:
        os.environ.pop(k, None)
    os.environ.update(CONFIGS[name])


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernels_per_step(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.device_type.name == "CUDA")
    except Exception as e:      # (the count is informative only)
        print("kernel count unavailable:", e, flush=True)
        return None


def op_times(dev, rounds, steps):
    """The attention pooling and the upsampled loss alone, forward + backward, at the batch-52 shapes: liblav_amd vs torch."""
    from lav_amd.rgb import Attention
    out = {}
    B = 52
    attn = Attention(512, num_heads=8).to(dev).train()
    for name, (h, w) in (("attn_wide_216", (9, 24)), ("attn_tel_90", (6, 15))):
        x = torch.relu(torch.randn(B, 512, h, w, device=dev)).requires_grad_(True)
        dout = torch.randn(B, 512, device=dev)
        fns = {"hip": lambda: hipnn.attn_pool_train(attn, x).backward(dout), "torch": lambda: attn(x).backward(dout)}
        out[name] = _ab(fns, rounds, steps, name)
    for name, (h, w) in (("xent_up_wide_72x192", (72, 192)), ("xent_up_tel_48x120", (48, 120))):
        lg = torch.randn(B, 4, h, w, device=dev).requires_grad_(True)
        lab8 = torch.randint(0, 4, (B, 4 * h, 4 * w), device=dev, dtype=torch.uint8)
        lab64 = lab8.long()
        fns = {"hip": lambda: hipnn.seg_cross_entropy_up(lg, lab8, 4).backward(),
               "torch": lambda: F.cross_entropy(F.interpolate(lg, scale_factor=4), lab64).backward()}
        out[name] = _ab(fns, rounds, steps, name)
    return out


def _ab(fns, rounds, steps, what):
    os.environ.pop("LAV_TRAIN_CONV", None)
    for f in fns.values():
        timed(f, 2)
    res = {n: [] for n in fns}
    for r in range(rounds):
        for n, f in fns.items():
            ms = timed(f, steps * 10)
            res[n].append(round(ms, 4))
            print(f"{what} round {r} {n}: {ms:.4f} ms", flush=True)
    return dict(ms=res, median_ms={n: sorted(v)[len(v) // 2] for n, v in res.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="52,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--ops", action="store_true", help="also time the two new operations alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    names = a.configs.split(",")
    out = dict(device=torch.cuda.get_device_name(0), images="288x768 + 192x480", defaults={p: hipnn.brake_piece_on(p) for p in hipnn.BRAKE_PIECES},
               results={})
    for B in [int(b) for b in a.batches.split(",") if b]:
        tr = BrakeTrainer(TrainConfig(), dev)
        batch = synthetic_bra_batch(B, seed=2021, device=dev)
        step = lambda: tr.train_bra(*batch)
        res, peak, launches = {n: [] for n in names}, {}, {}
        for n in names:              # warm-up of each configuration (MIOpen's solver search, the library's first launches), peak memory
            set_config(n)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            timed(step, 2)
            peak[n] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        for r in range(a.rounds):
            for n in names:
                set_config(n)
                ms = timed(step, a.steps)
                res[n].append(round(ms, 2))
                print(f"batch {B} round {r} {n}: {ms:.2f} ms/step", flush=True)
        for n in names:
            set_config(n)
            launches[n] = kernels_per_step(step)
        med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
        out["results"][str(B)] = dict(ms_per_step=res, median_ms=med, samples_per_s={n: round(B * 1e3 / v, 1) for n, v in med.items()},
                                      kernels_per_step=launches, peak_mem_gb=peak)
        del tr, batch
        torch.cuda.empty_cache()
    set_config("default")
    if a.ops:
        out["ops_batch52_fwd_bwd"] = op_times(dev, a.rounds, a.steps)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
