#!/usr/bin/env python3
"""lav_augment_u8 device time and what --augment 0.5 costs a training step.

Kernel: HIP events around 20 launches after warm-up, at train_seg's default batch (256 of 288 x 256) and train_bra's (52 of
288 x 768 plus 52 of 192 x 480), for the records Augmenter(0.5) draws and for all seven ops active; beside a plain device copy of
the same bytes on the same box (the floor: the kernel reads and writes every byte once).  Steps: LAV.train_seg (batch 32) and
BrakeTrainer.train_bra (batch 52) on host-resident synthetic uint8 batches as the trainers feed them, with and without the uint8
upload + augmentation in front, interleaved A B A B.  Fails without a GPU.  Prints one line per measurement; writes the JSON summary
to --out.

    python tools/augment_probe.py [--launches 20] [--rounds 3] [--steps 5] [--no-steps] [--out profiles/augment_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lav_amd import ops  # noqa: E402
from lav_amd.data import augment as A  # noqa: E402

SEED = 2021


def event_ms(fn, launches):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def kernel_case(name, shapes, launches, rounds):
    """shapes: [(batch, h, w), ...] launched one after the other (train_bra: wide, then tele)."""
    rng = np.random.default_rng(0)
    imgs = [torch.from_numpy(rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)).cuda() for b, h, w in shapes]
    nbytes = sum(t.numel() for t in imgs)
    res = dict(shapes=[list(s) for s in shapes], bytes=nbytes)
    tables = {"drawn_p0.5": [A.Augmenter(0.5, SEED, stream_tag=k).draw(t.shape[0]) for k, t in enumerate(imgs)],
              "all_seven_ops": [A.make_params(t.shape[0], active=range(7), per_channel=["noise", "dropout"], blur_sigma=0.5, noise_scale=12.75,
                                              dropout_p=0.1, multiply=1.2, contrast=1.2, gray_alpha=0.5, elastic_alpha=3.5) for t in imgs]}
    dsts = [torch.empty_like(t) for t in imgs]
    runs = {"copy": lambda: [d.copy_(t) for d, t in zip(dsts, imgs)]}
    for tname, tabs in tables.items():
        dev_tabs = [torch.from_numpy(p.view(np.uint8).reshape(len(p), -1)).cuda() for p in tabs]
        # the launch alone (ops.augment_u8 also uploads the 128-byte records and allocates the output: in the step times below)
        from lav_amd import _lib
        lib = _lib.load()

        def launch(dev_tabs=dev_tabs):
            for t, d, p in zip(imgs, dsts, dev_tabs):
                _lib.check(lib.lav_augment_u8(t.data_ptr(), d.data_ptr(), *t.shape[:3], p.data_ptr(), SEED, torch.cuda.current_stream().cuda_stream),
                           "lav_augment_u8")
        runs[tname] = launch
        runs[tname + "_with_upload"] = lambda tabs=tabs: [ops.augment_u8(t, p, SEED) for t, p in zip(imgs, tabs)]
    for rname, fn in runs.items():
        ms = [round(event_ms(fn, launches), 4) for _ in range(rounds)]
        res[rname] = dict(ms=ms, median_ms=sorted(ms)[len(ms) // 2], gb_per_s=round(2 * nbytes / sorted(ms)[len(ms) // 2] / 1e6, 1))
        print(f"{name} {rname}: {ms} ms  ({res[rname]['gb_per_s']} GB/s read + written)", flush=True)
    res["active_share_drawn"] = {A.OP_NAMES[o]: round(float(np.mean(np.concatenate(tables['drawn_p0.5'])["active"] >> o & 1)), 3) for o in range(7)}
    return res


def step_case(name, make_trainer, make_batch, nimg, rounds, steps):
    dev = torch.device("cuda")
    trainer, step = make_trainer(dev)
    batch = make_batch()
    augs = [A.Augmenter(0.5, SEED, stream_tag=k) for k in range(nimg)]

    def run(augment):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            b = list(batch)
            if augment:
                for k in range(nimg):
                    b[k] = augs[k](b[k].to(dev))
            step(trainer, b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for flag in (False, True):
        run(flag)
    res = {"plain": [], "augment_0.5": []}
    for r in range(rounds):
        for key, flag in (("plain", False), ("augment_0.5", True)):
            res[key].append(round(run(flag), 2))
            print(f"{name} round {r} {key}: {res[key][-1]} ms/step", flush=True)
    return dict(ms_per_step=res, median_ms={k: sorted(v)[len(v) // 2] for k, v in res.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true", help="the kernel only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    out = dict(device=torch.cuda.get_device_name(0), launches=a.launches, kernel={}, step={})
    out["kernel"]["train_seg_256x288x256"] = kernel_case("seg", [(256, 288, 256)], a.launches, a.rounds)
    out["kernel"]["train_bra_52x288x768+52x192x480"] = kernel_case("bra", [(52, 288, 768), (52, 192, 480)], a.launches, a.rounds)
    if not a.no_steps:
        from lav_amd.train import TrainConfig
        from lav_amd.train.brake import BRA_LABELS, BrakeTrainer
        from lav_amd.train.lav import LAV
        from lav_amd.train.synthetic import synthetic_bra_batch, synthetic_seg_batch
        out["step"]["train_seg_batch32"] = step_case(
            "train_seg b32", lambda d: (LAV(TrainConfig(), d, what="seg"), lambda t, b: t.train_seg(*b)),
            lambda: synthetic_seg_batch(32, seed=SEED), 1, a.rounds, a.steps)
        out["step"]["train_bra_batch52"] = step_case(
            "train_bra b52", lambda d: (BrakeTrainer(TrainConfig(), d), lambda t, b: t.train_bra(*b)),
            lambda: synthetic_bra_batch(52, seed=SEED, num_classes=len(BRA_LABELS) + 1), 2, a.rounds, a.steps)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
