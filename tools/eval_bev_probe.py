#!/usr/bin/env python3
"""What the teacher's evaluation costs on an MI355X.

(a) Launch: one HIP event pair around EACH of --launches calls of ops.eval_plans after warm-up, at a loader batch's geometry - B = 8
    frames, K = 20 forecasts, T = 20 waypoints, I = 5 plan iterations - on a seeded batch (tests/eval_bev_util.py) resident in HBM:
    median, quartiles, minimum and maximum in microseconds.  The window of one call holds the wrapper's argument checks too, so the
    median is an upper bound of the kernel's time; the same calls back to back between one event pair give the per-call time of a full
    queue.
(b) Frames: evaluated frames per second over --frames synthetic frames in batches of 8 (lav_amd.train.evaluate_bev.BevEvaluator at the
    frame's precision: upload, infer_batch, the metrics launch) beside BevEvaluator.infer - infer_batch alone - on the same uploaded
    batches, interleaved, --rounds medians.

Reports; asserts no threshold.  Fails without a GPU: a time measured elsewhere says nothing about the MI355X.

    python tools/eval_bev_probe.py [--launches 200] [--frames 64] [--rounds 3] [--out profiles/eval_bev_probe.json]
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
from lav_amd.train import evaluate_bev as E  # noqa: E402
from tests import eval_bev_util as U  # noqa: E402

B, K, T, I = 8, 20, 20, 5


def launch_case(launches):
    s = U.random_batch(1, B=B, K=K, T=T, I=I)
    args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in U.positional(s)]
    acc = torch.zeros(len(E.PlanLayout(I)), dtype=torch.int64, device="cuda")
    for _ in range(20):
        ops.eval_plans(acc, *args)
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in pairs:
        e0.record()
        ops.eval_plans(acc, *args)
        e1.record()
    torch.cuda.synchronize()
    us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        ops.eval_plans(acc, *args)
    e1.record()
    torch.cuda.synchronize()
    q = lambda p: float(np.percentile(us, p))
    return {"geometry": dict(frames=B, forecasts=K, waypoints=T, iterations=I), "launches": launches, "median_us": q(50), "p25_us": q(25),
            "p75_us": q(75), "min_us": float(us.min()), "max_us": float(us.max()), "back_to_back_us": e0.elapsed_time(e1) * 1e3 / launches}


def frames_case(frames, rounds):
    from lav_amd.train import LAV, TrainConfig
    from lav_amd.train.synthetic import synthetic_bev_batch
    cfg = TrainConfig()
    torch.manual_seed(cfg.seed)
    lav = LAV(cfg, torch.device("cuda"), what="bev")
    batches = [synthetic_bev_batch(B, seed=3 + 1009 * i, num_plan=cfg.num_plan) for i in range(max(1, frames // B))]
    ev = E.BevEvaluator(lav)
    times = {"evaluate": [], "infer": []}
    forecasts = 0
    for r in range(rounds + 1):                     # round 0 warms up
        for what in ("infer", "evaluate"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for batch in batches:
                ev.upload(batch)
                if what == "infer":
                    out = ev.infer()
                    if r == 0:
                        forecasts += int(out.other_locs.shape[0])
                else:
                    ev.batch()
            if what == "evaluate":
                ev.counters()
            torch.cuda.synchronize()
            if r:
                times[what].append(len(batches) * B / (time.perf_counter() - t0))
    return {"frames": len(batches) * B, "batch": B, "forecasts": forecasts, "rounds": rounds, "precision": ev.precision(),
            "evaluate_frames_per_s": float(np.median(times["evaluate"])), "infer_batch_frames_per_s": float(np.median(times["infer"])),
            "all_evaluate": times["evaluate"], "all_infer_batch": times["infer"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_bev_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bev_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    res = {"device": torch.cuda.get_device_name(0), "launch": launch_case(args.launches), "frames": frames_case(args.frames, args.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
