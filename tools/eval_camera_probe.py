#!/usr/bin/env python3
"""What the camera evaluation costs on an MI355X.

(a) Launches: one HIP event pair around EACH of --launches calls after 20 warm-ups, on seeded cases (tests/eval_camera_util.py)
    resident in HBM: ops.eval_seg at 3 x 5 x 288 x 256 (scale 1, the agent's call), 1 x 4 x 72 x 192 against 288 x 768 labels and
    1 x 4 x 48 x 120 against 192 x 480 labels (scale 4, the brake net's two heads), ops.eval_scores at n = 1.  Median, quartiles,
    minimum and maximum in microseconds; the bytes a launch reads over its median as a fraction of the 8 TB/s HBM figure DESIGN uses.
    The window of one call holds the wrapper's argument checks too, so the median is an upper bound of the kernel's time.  These are
    1 - 5 MB: expect latency, not bandwidth.
(b) Evaluators: images / frames per second of SegEvaluator and BrakeEvaluator on synthetic data with seeded weights, beside the models'
    forwards alone on the same uploaded inputs, interleaved, --rounds medians.  That is the comparison that matters.

Reports; asserts no threshold.  Fails without a GPU: a time measured elsewhere says nothing about the MI355X.

    python tools/eval_camera_probe.py [--launches 200] [--images 48] [--frames 16] [--rounds 3] [--out profiles/eval_camera_probe.json]
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
from lav_amd import ops, synth  # noqa: E402
from lav_amd.train import evaluate_camera as C  # noqa: E402
from tests import eval_camera_util as U  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def timed(call, launches, nbytes):
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in pairs:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    torch.cuda.synchronize()
    q = lambda p: float(np.percentile(us, p))
    return {"launches": launches, "bytes_read": nbytes, "median_us": q(50), "p25_us": q(25), "p75_us": q(75), "min_us": float(us.min()),
            "max_us": float(us.max()), "back_to_back_us": e0.elapsed_time(e1) * 1e3 / launches,
            "fraction_of_hbm_at_median": nbytes / (q(50) * 1e-6) / HBM_BYTES_PER_S}


def launch_cases(launches):
    out = {}
    for name, (n, k, h, w, scale) in (("seg_3x5x288x256_scale1", (3, 5, 288, 256, 1)), ("seg_1x4x72x192_scale4", (1, 4, 72, 192, 4)),
                                      ("seg_1x4x48x120_scale4", (1, 4, 48, 120, 4))):
        case = U.seg_case(11, n, k, h, w, scale)
        logits, labels = torch.from_numpy(case["logits"]).cuda(), torch.from_numpy(case["labels"]).cuda()
        section = torch.zeros(68, dtype=torch.int64, device="cuda")
        out[name] = timed(lambda: ops.eval_seg(section, logits, labels, scale), launches, logits.numel() * 4 + labels.numel())
    scores, flags = torch.full((1,), 0.3, device="cuda"), torch.ones(1, dtype=torch.uint8, device="cuda")
    section = torch.zeros(6 + 2 * 256, dtype=torch.int64, device="cuda")
    out["scores_n1"] = timed(lambda: ops.eval_scores(section, scores, flags, 0.1, 256), launches, 5)
    return out


def seeded(model, prefix):
    model.load_state_dict(synth.seeded_state_dict(model, prefix=prefix))
    return model.cuda().eval()


def rate(rounds, units, forward, evaluate):
    times = {"evaluate": [], "forward": []}
    for r in range(rounds + 1):                     # round 0 warms up
        for what, fn in (("forward", forward), ("evaluate", evaluate)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times[what].append(units / (time.perf_counter() - t0))
    return {"rounds": rounds, "evaluate_per_s": float(np.median(times["evaluate"])), "forward_per_s": float(np.median(times["forward"])),
            "all_evaluate": times["evaluate"], "all_forward": times["forward"]}


@torch.no_grad()
def seg_rate(images, rounds):
    from lav_amd.rgb import RGBSegmentationModel
    from lav_amd.train.synthetic import synthetic_seg_batch
    model = seeded(RGBSegmentationModel([4, 6, 7, 10]), "seg.")
    rgb, sem = synthetic_seg_batch(images, seed=3)
    ev = C.SegEvaluator(model)

    def forward():      # the evaluator's loop without the metrics launch: the same upload, conversion and calls of three images
        x = ops.image_u8_to_f32(rgb.cuda(), reverse=False)
        sem.to(torch.uint8).cuda()
        for j in range(0, images, ev.images_per_call):
            with ops.precision(ev.code):
                model(x[j:j + ev.images_per_call])

    def evaluate():
        ev.batch(rgb, sem)
        ev.counters()
    return dict(images=images, images_per_call=ev.images_per_call, **rate(rounds, images, forward, evaluate), precision=ev.precision())


@torch.no_grad()
def bra_rate(frames, rounds):
    from lav_amd.rgb import RGBBrakePredictionModel
    from lav_amd.train.synthetic import synthetic_bra_batch
    model = seeded(RGBBrakePredictionModel([4, 10, 18]), "bra.")
    batch = synthetic_bra_batch(frames, seed=3)
    ev = C.BrakeEvaluator(model)

    def forward():      # the same uploads and per-frame calls, the heads included, without the three metrics launches
        wide, tele = ops.image_u8_to_f32(batch[0].cuda(), reverse=False), ops.image_u8_to_f32(batch[1].cuda(), reverse=False)
        batch[2].cuda(), batch[3].cuda(), batch[4].cuda()
        for i in range(frames):
            with ops.precision(ev.code):
                x1, x2 = model.trunk(wide[i:i + 1]), model.trunk(tele[i:i + 1])
                model.classify(x1, x2)
                model.seg_head(x1), model.seg_head(x2)

    def evaluate():
        ev.batch(*batch)
        ev.counters()
    return dict(frames=frames, **rate(rounds, frames, forward, evaluate), precision=ev.precision())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_camera_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_camera_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    res = {"device": torch.cuda.get_device_name(0), "launch": launch_cases(args.launches), "seg": seg_rate(args.images, args.rounds),
           "bra": bra_rate(args.frames, args.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
