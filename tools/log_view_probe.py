#!/usr/bin/env python3
"""What the trainers' visual log costs on an MI355X.

(a) Launch: HIP events around --launches calls of ops.log_view (one upload of the tables, the zeroing, the minimum / maximum and the
    compose launches) after warm-up, at the four trainers' geometries - bev 320 x 320, lidar 332 x 640 with 0 and 7 detections, seg
    288 x 768, bra 360 x 1248 - from seeded views (tests/log_view_util.py), the sources resident.
(b) Step: seconds per train_seg step (synthetic batch of --batch images) with the view switched on - the step returns its sources,
    the frame is built, composed and handed to the writer - against the same step with it off, interleaved, --rounds medians.

Reports; asserts no threshold.  Fails without a GPU: a time measured elsewhere says nothing about the MI355X.

    python tools/log_view_probe.py [--launches 50] [--steps 10] [--rounds 3] [--batch 8] [--out profiles/log_view_probe.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lav_amd.train import log_view as V  # noqa: E402
from tests.log_view_util import seeded_view  # noqa: E402


def launch_case(launches):
    res = {}
    for what, ndet in (("bev", 0), ("lidar", 0), ("lidar", 7), ("seg", 0), ("bra", 0)):
        frame = V.build_frame(what, seeded_view(what, ndet))
        frame = frame._replace(sources=[torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in frame.sources])
        out = torch.empty(frame.size + (3,), dtype=torch.uint8, device="cuda")
        for _ in range(5):
            V.render(frame, out=out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            V.render(frame, out=out)
        e1.record()
        torch.cuda.synchronize()
        res[f"{what}_{ndet}"] = {"frame": list(frame.size), "records": int(len(frame.prims)), "with_upload_ms": e0.elapsed_time(e1) / launches}
    return res


def step_case(steps, rounds, batch):
    from lav_amd.train import LAV, TrainConfig, synthetic_seg_batch
    cfg = TrainConfig()
    lav = LAV(cfg, torch.device("cuda"), what="seg")
    data = synthetic_seg_batch(batch, seed=1, num_classes=len(cfg.seg_channels) + 1, device="cuda")
    times = {False: [], True: []}
    with tempfile.TemporaryDirectory() as root:
        writer = V.FrameWriter(root, "seg")
        for r in range(rounds + 1):                 # round 0 warms up
            for on in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(steps):
                    lav.log_view = on
                    info = lav.train_seg(*data)
                    if on:
                        writer.add(V.render(V.build_frame("seg", info.pop("view"), cfg)), i)
                torch.cuda.synchronize()
                if r:
                    times[on].append((time.perf_counter() - t0) / steps)
        writer.close()
    return {"batch": batch, "steps": steps, "rounds": rounds, "s_per_step_unlogged": float(np.median(times[False])),
            "s_per_step_logged": float(np.median(times[True])), "all_unlogged": times[False], "all_logged": times[True]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "log_view_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("log_view_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    res = {"device": torch.cuda.get_device_name(0), "launch": launch_case(args.launches), "step": step_case(args.steps, args.rounds, args.batch)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
