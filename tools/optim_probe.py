#!/usr/bin/env python3
"""What the optimiser step costs on an MI355X: FusedAdam.step() (lav_optim_adam_step: statistics, finalise, update) against
torch.optim.Adam.step() (torch's multi-tensor path) on the parameter shapes of LAV(what="lidar") and LAV(what="bev").

Both optimisers step their own copies of the trained parameters on fixed random gradients.  A sample is the time between two HIP
events around --burst back-to-back steps, divided by the burst; reported is the median of --samples samples after a warm-up, and the
host time one step takes to enqueue; lav_optim_grad_stats (the first two launches) the same way.  The update launch alone is timed by
the library's own HIP events around it (lav_profile_enable) over --samples further steps; its bytes are 28 per element (p, g, m, v read,
p, m, v written), against the 6.3 TB/s of HBM that are achievable.

Reports; asserts no threshold.  Fails without a GPU: a time measured elsewhere says nothing about the MI355X.

    python tools/optim_probe.py [--samples 200] [--burst 20] [--out profiles/optim_probe.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lav_amd import _lib, ops  # noqa: E402
from lav_amd.train import LAV, TrainConfig  # noqa: E402
from lav_amd.train.optim import FusedAdam  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def timed(fn, samples, burst):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    ms, host = [], []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(burst):
            fn()
        host.append((time.perf_counter() - t0) * 1e3 / burst)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / burst)
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "p90_ms": float(np.percentile(ms, 90)),
            "host_enqueue_median_ms": float(np.median(host))}


def case(what, samples, burst):
    torch.manual_seed(0)
    lav = LAV(TrainConfig(log_inference=False), "cuda", what=what)
    shapes = [tuple(p.shape) for g in getattr(lav, f"{what}_optim").param_groups for p in g["params"]]
    del lav
    gen = torch.Generator(device="cuda").manual_seed(1)
    sets = []
    for _ in range(2):
        ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen)) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-2
        sets.append(ps)
    fused, adam = FusedAdam(sets[0], lr=3e-4), torch.optim.Adam(sets[1], lr=3e-4)
    numel = sum(p.numel() for p in sets[0])
    res = {"tensors": len(shapes), "elements": numel, "largest": max(p.numel() for p in sets[0]), "samples": samples, "burst": burst,
           "torch_adam": timed(adam.step, samples, burst), "fused_adam": timed(fused.step, samples, burst)}
    n, chunks, nw, wchunks = fused._counts
    stats = lambda: ops.optim_grad_stats(fused._table, n, chunks, fused._watch_table, nw, wchunks, fused._global, None)
    res["grad_stats"] = timed(stats, samples, burst)
    h = fused.health()
    assert h["skipped"] == 0 and h["applied"] > 0, h
    # the launches themselves: the library's HIP-event timers around them (lav_profile_enable), over --samples further steps
    lib = _lib.load()
    lib.lav_profile_enable(4096)
    lib.lav_profile_reset()
    for _ in range(samples):
        fused.step()
    torch.cuda.synchronize()
    launches = {}
    for name in ("optim_stats", "optim_update"):
        ms, n = ctypes.c_double(), ctypes.c_int()
        lib.lav_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(n))
        launches[name] = {"calls": n.value, "mean_ms": ms.value / max(n.value, 1)}
    lib.lav_profile_enable(0)
    update_ms, stats_ms = launches["optim_update"]["mean_ms"], launches["optim_stats"]["mean_ms"]
    res["chunks"] = chunks
    res["launches"] = launches
    res["stats_bytes"] = 4 * numel
    res["stats_bytes_per_s"] = 4 * numel / (stats_ms * 1e-3)
    res["update_bytes"] = 28 * numel
    res["update_bytes_per_s"] = 28 * numel / (update_ms * 1e-3)
    res["update_fraction_of_hbm"] = res["update_bytes_per_s"] / HBM_ACHIEVABLE
    res["fused_over_torch"] = res["fused_adam"]["median_ms"] / res["torch_adam"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optim_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    res = {"device": torch.cuda.get_device_name(0), "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
           "lidar": case("lidar", args.samples, args.burst), "bev": case("bev", args.samples, args.burst)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
