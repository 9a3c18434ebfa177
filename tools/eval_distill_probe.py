#!/usr/bin/env python3
"""What the student-beside-teacher evaluation costs on an MI355X.

(a) Launch: one HIP event pair around EACH of --launches calls of ops.eval_distill after 20 warm-ups, at a group's geometry - B = 8
    frames, K = 20 forecasts, T = 20 waypoints, I = 5 plan iterations - on a seeded batch (tests/eval_distill_util.py) resident in HBM:
    median, quartiles, minimum and maximum in microseconds.  The window of one call holds the wrapper's argument checks too, so the
    median is an upper bound of the kernel's time; the same calls back to back between one event pair give the per-call time of a full
    queue.
(b) Frames: evaluated frames per second over --frames synthetic frames in batches of 8, in one process, interleaved, --rounds medians:
    lav_amd.train.evaluate_distill.DistillEvaluator (the LiDAR trunk on 8 clouds, both infer_batch, three metrics launches) beside
    lav_amd.train.evaluate.Evaluator (eval_full_v2: the student frame by frame, the way the agent runs it) on the same clouds and
    lav_amd.train.evaluate_bev.BevEvaluator (eval_bev_v2: the teacher alone) on the same frames' BEV stacks.

Reports; asserts no threshold.  Fails without a GPU: a time measured elsewhere says nothing about the MI355X.

    python tools/eval_distill_probe.py [--launches 200] [--frames 32] [--rounds 3] [--out profiles/eval_distill_probe.json]
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
from lav_amd.train import evaluate as EF  # noqa: E402
from lav_amd.train import evaluate_bev as EB  # noqa: E402
from lav_amd.train import evaluate_distill as E  # noqa: E402
from tests import eval_distill_util as U  # noqa: E402

B, K, T, I = 8, 20, 20, 5


def launch_case(launches):
    s = U.random_batch(1, Bn=B, K=K, T=T, I=I)
    args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in U.positional(s)]
    acc = torch.zeros(len(E.PairLayout(I)), dtype=torch.int64, device="cuda")
    for _ in range(20):
        ops.eval_distill(acc, *args)
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in pairs:
        e0.record()
        ops.eval_distill(acc, *args)
        e1.record()
    torch.cuda.synchronize()
    us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        ops.eval_distill(acc, *args)
    e1.record()
    torch.cuda.synchronize()
    q = lambda p: float(np.percentile(us, p))
    return {"geometry": dict(frames=B, forecasts=K, waypoints=T, iterations=I), "launches": launches, "median_us": q(50), "p25_us": q(25),
            "p75_us": q(75), "min_us": float(us.min()), "max_us": float(us.max()), "back_to_back_us": e0.elapsed_time(e1) * 1e3 / launches}


def frames_case(frames, rounds, max_points):
    from lav_amd.train import LAV, TrainConfig
    from lav_amd.train.synthetic import synthetic_lidar_batch
    cfg = TrainConfig()
    torch.manual_seed(cfg.seed)
    lav = LAV(cfg, torch.device("cuda"), what="lidar")
    lav.student.eval()
    batches = [synthetic_lidar_batch(B, seed=3 + 1009 * i, max_points=max_points, num_plan=cfg.num_plan) for i in range(max(1, frames // B))]
    make = {"distill": lambda: E.DistillEvaluator(lav), "eval_full": lambda: EF.Evaluator(lav), "eval_bev": lambda: EB.BevEvaluator(lav.bev_planner)}
    feed = {"distill": batches, "eval_full": batches, "eval_bev": [b[5:] for b in batches]}
    times = {k: [] for k in make}
    in_force, forecasts = {}, 0
    for r in range(rounds + 1):                     # round 0 warms up
        for what in make:
            ev = make[what]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = ev.run(feed[what])
            acc = ev.counters()
            torch.cuda.synchronize()
            if r:
                times[what].append(n / (time.perf_counter() - t0))
            in_force[what] = ev.precision()
            if what == "distill":
                pair = ev.layout.fields(acc, "pair")
                forecasts = int(pair["others"].item() + pair["oth_nonfinite"].item())
    out = {"frames": len(batches) * B, "batch": B, "points_per_cloud": max_points, "forecasts": forecasts, "rounds": rounds, "precision": in_force}
    for what, v in times.items():
        out[what + "_frames_per_s"] = float(np.median(v))
        out["all_" + what] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-points", type=int, default=120000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_distill_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_distill_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    res = {"device": torch.cuda.get_device_name(0), "launch": launch_case(args.launches), "frames": frames_case(args.frames, args.rounds, args.max_points)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
