#!/usr/bin/env python3
"""What the box-metric evaluation costs on an MI355X.

(a) Launch: one HIP event pair around EACH of --launches calls of ops.eval_det after warm-up, at 15 rows per class and 20 actors on a
    seeded frame (tests/eval_det_util.py) resident in HBM: median, quartiles, minimum and maximum in microseconds.  The window of one
    call holds the wrapper's argument checks too, so the median is an upper bound of the kernel's time; the same calls back to back
    between one event pair give the per-call time of a full queue.
(b) Frames: evaluated frames per second over --frames synthetic frames of lav_amd.train.evaluate_det.DetEvaluator (heads "peaks", what
    the tool runs by default) beside the same pillar -> backbone -> detect chain WITHOUT the metrics launch, on the same clouds in the
    same process, interleaved, --rounds medians.

Reports; asserts no threshold.  Fails without a GPU: a time measured elsewhere says nothing about the MI355X.

    python tools/eval_det_probe.py [--launches 200] [--frames 50] [--rounds 3] [--out profiles/eval_det_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lav_amd import ops  # noqa: E402
from lav_amd.train import evaluate_det as E  # noqa: E402
from tests import eval_det_util as U  # noqa: E402


def launch_case(launches):
    f = U.random_scene(1, D=15, G=20, used=15)
    args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if isinstance(a, np.ndarray) else a for a in U.positional(f)]
    acc = torch.zeros(len(E.DetLayout(E.NBINS)), dtype=torch.int64, device="cuda")
    for _ in range(20):
        ops.eval_det(acc, *args, **f["kw"])
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in pairs:
        e0.record()
        ops.eval_det(acc, *args, **f["kw"])
        e1.record()
    torch.cuda.synchronize()
    us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        ops.eval_det(acc, *args, **f["kw"])
    e1.record()
    torch.cuda.synchronize()
    q = lambda p: float(np.percentile(us, p))
    return {"geometry": dict(rows_per_class=15, actors=20, nbins=E.NBINS), "launches": launches, "median_us": q(50), "p25_us": q(25),
            "p75_us": q(75), "min_us": float(us.min()), "max_us": float(us.max()), "back_to_back_us": e0.elapsed_time(e1) * 1e3 / launches}


def frames_case(frames, rounds):
    from lav_amd.train import LAV, TrainConfig
    from lav_amd.train.synthetic import synthetic_lidar_batch
    cfg = TrainConfig()
    torch.manual_seed(cfg.seed)
    lav = LAV(cfg, torch.device("cuda"), what="lidar")
    lav.student.eval()
    batch = synthetic_lidar_batch(min(frames, 10), seed=3, max_points=cfg.max_lidar_points)
    ev = E.DetEvaluator(lav)
    B = ev.upload(batch)
    runs = {"eval_det": ev.frame, "chain_only": ev.forward}
    times = {what: [] for what in runs}
    for r in range(rounds + 1):                     # round 0 warms up
        for what, one in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(frames):
                one(k % B)
            if what == "eval_det":
                ev.counters()
            torch.cuda.synchronize()
            if r:
                times[what].append(frames / (time.perf_counter() - t0))
    return {"frames": frames, "rounds": rounds, "points": cfg.max_lidar_points, "heads": "peaks",
            "eval_det_frames_per_s": float(np.median(times["eval_det"])), "chain_only_frames_per_s": float(np.median(times["chain_only"])),
            "all_eval_det": times["eval_det"], "all_chain_only": times["chain_only"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_det_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_det_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    res = {"device": torch.cuda.get_device_name(0), "launch": launch_case(args.launches), "frames": frames_case(args.frames, args.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
