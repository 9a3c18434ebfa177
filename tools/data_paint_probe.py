#!/usr/bin/env python3
"""Throughput of the offline point painter (data_paint.py) on a synthetic data set of 2 routes with 5 cameras of 288 x 256 and
40 000 points per sweep (config.yaml's max_lidar_points), seeded segmenter weights:

  * frames/s of paint_dataset at frames_per_batch 1, 4, 16 (stages not synchronised);
  * the per-frame time split at each of them - decode (in the loader processes), upload + convert, ERFNet, paint_frames
    (upload of the clouds, the launch, the download), commit - from a second pass that synchronises between the stages;
  * lav_paint_frames alone (device time, events around 20 launches) against paint_from_cameras on the host for the same batch.

    python tools/data_paint_probe.py [--frames 16] [--num-workers 8] [--out profiles/data_paint_probe.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from lav_amd import ops, synth  # noqa: E402
from lav_amd.data import synthetic_route  # noqa: E402
from lav_amd.data.paint import PointPaintDataset, PointPainter, host_paint, paint_dataset  # noqa: E402
from lav_amd.rgb import RGBSegmentationModel  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16, help="indexed frames per route")
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--num-workers", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "data_paint_probe.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), routes=2, cameras=5, image="288x256", points_per_sweep=a.points,
               indexed_frames=2 * a.frames, num_workers=a.num_workers, runs={})
    with tempfile.TemporaryDirectory() as root:
        with open(os.path.join(REPO, "tests", "golden", "dataset_config.yaml")) as f:
            cfg = yaml.safe_load(f)
        cfg.update(num_plan=4, data_dir=os.path.join(root, "data"), seg_model_dir=os.path.join(root, "seg.th"))
        synthetic_route.make_dataset(cfg["data_dir"], routes=2, frames=a.frames + cfg["num_plan"], seed=0, points=a.points, cameras=5,
                                     camera_hw=(288, 256))
        seg = RGBSegmentationModel(cfg["seg_channels"])
        torch.save(synth.seeded_state_dict(seg, prefix="seg."), cfg["seg_model_dir"])
        config_path = os.path.join(root, "config.yaml")
        with open(config_path, "w") as f:
            yaml.safe_dump(cfg, f)
        painter = PointPainter(config_path, dev)
        paint_dataset(config_path, dev, frames_per_batch=4, num_workers=a.num_workers, num_per_log=0, painter=painter)      # warm-up
        for fpb in (1, 4, 16):
            painter.timed = False
            s = paint_dataset(config_path, dev, frames_per_batch=fpb, num_workers=a.num_workers, num_per_log=0, painter=painter)
            run = dict(frames_per_s=round(s["frames"] / s["seconds"], 2))
            painter.timed = True
            painter.seconds = dict(upload_convert=0.0, erfnet=0.0, paint_frames=0.0)
            s = paint_dataset(config_path, dev, frames_per_batch=fpb, num_workers=a.num_workers, num_per_log=0, painter=painter)
            run["frames_per_s_synchronised"] = round(s["frames"] / s["seconds"], 2)
            run["ms_per_frame"] = {k: round(1e3 * s[k] / s["frames"], 3) for k in ("decode", "upload_convert", "erfnet", "paint_frames", "commit")}
            res["runs"][str(fpb)] = run
            print(fpb, run, flush=True)
        # ERFNet frame by frame (what the painter does) against one run over a batch's images: time, and how far the maps differ
        ds = PointPaintDataset(config_path)
        imgs = np.concatenate([ds.raw(i)[1] for i in range(16)])
        with torch.no_grad():
            x = ops.image_u8_to_f32(torch.from_numpy(imgs).to(dev), reverse=True)

            def timed(fn, reps=3):
                fn()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(reps):
                    out = fn()
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t) / reps, out
            per_frame_ms, a5 = timed(lambda: torch.cat([painter.seg_model.probs(x[at:at + 5]).clone() for at in range(0, 80, 5)]))
            res["erfnet_16_frames"] = dict(per_frame_runs_ms=round(per_frame_ms, 2), max_abs_diff_vs_per_frame={})
            for rows in (20, 80):
                ms, b = timed(lambda: torch.cat([painter.seg_model.probs(x[at:at + rows]).clone() for at in range(0, 80, rows)]))
                res["erfnet_16_frames"][f"runs_of_{rows}_images_ms"] = round(ms, 2)
                res["erfnet_16_frames"]["max_abs_diff_vs_per_frame"][str(rows)] = float((a5 - b).abs().max())
            del a5, b
        print(res["erfnet_16_frames"], flush=True)
        # the painting kernel alone, on a batch of 16 frames
        lidars = [ds.raw(i)[0] for i in range(16)]
        offsets = np.zeros(17, np.int32)
        offsets[1:] = np.cumsum([len(l) for l in lidars])
        lidar = np.concatenate(lidars)
        r = np.random.Generator(np.random.PCG64(1))
        e = r.exponential(1.0, (16, 5, 5, 288, 256)).astype(np.float32)
        sem = e / e.sum(axis=2, keepdims=True)
        d_l, d_o, d_s = torch.from_numpy(lidar).to(dev), torch.from_numpy(offsets).to(dev), torch.from_numpy(sem).to(dev)
        cams = ops.make_cameras_f64(painter.cameras)
        for _ in range(3):
            out = ops.paint_frames(d_l, d_o, d_s, cams)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(20):
            out = ops.paint_frames(d_l, d_o, d_s, cams)
        t1.record()
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        want = host_paint(lidar, offsets, sem, painter.cameras)
        host_ms = 1e3 * (time.perf_counter() - h0)
        res["paint_frames_batch16"] = dict(points=int(len(lidar)), kernel_ms=round(t0.elapsed_time(t1) / 20, 4), host_paint_from_cameras_ms=round(host_ms, 1),
                                           rows_equal=int((out.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all(1).sum()))
        print(res["paint_frames_batch16"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
