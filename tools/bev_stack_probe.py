#!/usr/bin/env python3
"""What --bev-on-device moves, and what it costs on the device.

(a) Loader: ms per sample of 'temporal_bev' and 'temporal_lidar_painted' in this process (one worker's view), default against
    bev_on_device=True, over one synthetic route (40 frames, 30 000 points per sweep, max_lidar_points 120 000, the other keys of
    tests/golden/dataset_config.yaml); the same sample indices in the same order, interleaved A B.  Needs no GPU.
(b) Kernel: HIP events around --launches launches of lav_bev_stack_u8 after warm-up at train_bev's and train_full's per-GPU batches
    (64 and 32 samples of 9 planes of 320 x 320), for records drawn like the temporal loaders' (angle jitter +-20 degrees, relative
    headings of a few degrees, the current frame's five planes with W1 = identity) and for the worst rotations (45 degrees twice on
    every plane); beside a plain device copy of the same bytes (the floor: every byte read and written once).  Fails without a GPU
    unless --no-kernel.

    python tools/bev_stack_probe.py [--samples 8] [--launches 20] [--rounds 3] [--no-loader] [--no-kernel] [--out profiles/bev_stack_probe.json]
"""
import argparse
import json
import os
import platform
import sys
import tempfile
import time

import numpy as np
import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lav_amd.data import bev_stack as S  # noqa: E402
from lav_amd.data import datasets, image, synthetic_route  # noqa: E402


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            return next(ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name"))
    except (OSError, StopIteration):
        return platform.processor() or "unknown"


def loader_case(samples, rounds):
    res = {}
    with tempfile.TemporaryDirectory() as root:
        synthetic_route.make_dataset(os.path.join(root, "data"), routes=1, frames=40, seed=0, points=30000)
        with open(os.path.join(REPO, "tests", "golden", "dataset_config.yaml")) as f:
            cfg = yaml.safe_load(f)
        cfg.update(data_dir=os.path.join(root, "data"), max_lidar_points=120000)
        path = os.path.join(root, "config.yaml")
        with open(path, "w") as f:
            yaml.safe_dump(cfg, f)
        for name in ("temporal_bev", "temporal_lidar_painted"):
            sets = {False: datasets.LOADERS[name](path), True: datasets.LOADERS[name](path)}
            sets[True].bev_on_device = True
            picks = np.linspace(2, len(sets[False]) - 1, samples).astype(int)
            ms = {False: [], True: []}
            for r in range(rounds + 1):            # round 0 warms the page cache and the imports
                for deferred in (False, True):
                    torch.manual_seed(r)
                    np.random.seed(r)
                    t0 = time.perf_counter()
                    for i in picks:
                        sets[deferred][int(i)]
                    if r:
                        ms[deferred].append(round((time.perf_counter() - t0) * 1e3 / len(picks), 2))
            med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
            res[name] = dict(samples=len(picks), default_ms_per_sample=ms[False], deferred_ms_per_sample=ms[True],
                             median_default_ms=med[False], median_deferred_ms=med[True], median_saved_ms=round(med[False] - med[True], 2))
            print(f"loader {name}: default {ms[False]} ms/sample, deferred {ms[True]} ms/sample", flush=True)
    return res


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


def records(batch, kind, rng):
    """coef (batch, 9, 12), shift (batch, 9, 2)."""
    rot = lambda deg: image.inverse_map(image.rotation_matrix_2d(datasets.BEV_CENTER, deg, 1.0))
    coef, shift = np.empty((batch, 9, 12)), np.zeros((batch, 9, 2), np.int32)
    for b in range(batch):
        jitter, off = rng.uniform(-20, 20), int(rng.integers(-10, 11))
        for k, planes in enumerate(((0, 1, 2), (3, 4), (5, 6), (7, 8))):
            w1 = 0.0 if k == 0 or k == 1 else rng.uniform(-3, 3) * (k - 1)
            if kind == "worst_rotations":
                w1, jitter = 45.0, 45.0
            for p in planes:
                coef[b, p] = np.concatenate([rot(w1) if w1 else S.IDENTITY, rot(jitter)])
                shift[b, p] = (0 if k < 2 else int(rng.integers(-6, 1)) * (k - 1), off)
    return coef, shift


def kernel_case(batch, launches, rounds):
    from lav_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(batch)
    blocks = rng.random((batch, 9, 41, 41)) < 1 / 6
    planes = torch.from_numpy((np.kron(blocks, np.ones((8, 8), np.uint8))[..., :320, :320] * 255).astype(np.uint8)).cuda()
    dst = torch.empty_like(planes)
    res = dict(shape=list(planes.shape), bytes=planes.numel())
    runs = {"copy": lambda: dst.copy_(planes)}
    for kind in ("drawn_like_the_loaders", "worst_rotations"):
        coef, shift = records(batch, kind, rng)
        cd, sd = torch.from_numpy(coef.reshape(-1, 12)).cuda(), torch.from_numpy(shift.reshape(-1, 2)).cuda()
        paths = np.sum([ops.bev_stack_tile_paths(c, s, 320, 320) for c, s in zip(coef.reshape(-1, 12), shift.reshape(-1, 2))], axis=0)
        res[kind + "_tiles_zero_staged_direct"] = [int(v) for v in paths]

        def launch(cd=cd, sd=sd):
            _lib.check(lib.lav_bev_stack_u8(planes.data_ptr(), cd.data_ptr(), sd.data_ptr(), dst.data_ptr(), batch * 9, 320, 320, 1,
                                            torch.cuda.current_stream().cuda_stream), "lav_bev_stack_u8")
        runs[kind] = launch
        runs[kind + "_with_upload"] = lambda coef=coef, shift=shift: ops.bev_stack_u8(planes, coef, shift)
    for name, fn in runs.items():
        ms = [round(event_ms(fn, launches), 4) for _ in range(rounds)]
        med = sorted(ms)[len(ms) // 2]
        res[name] = dict(ms=ms, median_ms=med, gb_per_s=round(2 * planes.numel() / med / 1e6, 1))
        print(f"kernel batch {batch} {name}: {ms} ms  ({res[name]['gb_per_s']} GB/s read + written)", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-loader", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(host_cpu=cpu_name())
    if not a.no_kernel:
        if not torch.cuda.is_available():
            raise SystemExit("bev_stack_probe: no GPU; a kernel time measured elsewhere says nothing about the MI355X (--no-kernel: loaders only)")
        out["device"] = torch.cuda.get_device_name(0)
        out["kernel"] = {"train_bev_64x9x320x320": kernel_case(64, a.launches, a.rounds), "train_full_32x9x320x320": kernel_case(32, a.launches, a.rounds)}
    if not a.no_loader:
        out["loader"] = loader_case(a.samples, a.rounds)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
