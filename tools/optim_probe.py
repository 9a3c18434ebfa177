#!/usr/bin/env python3
"""What the optimiser step costs on an MI355X: FusedAdam.step() (lav_optim_adam_step: statistics, finalise, update) against
torch.optim.Adam.step() (torch's multi-tensor path) on the parameter shapes of LAV(what="lidar") and LAV(what="bev").

Both optimisers step their own copies of the trained parameters on fixed random gradients.  A sample is the time between two HIP
events around --burst back-to-back steps, divided by the burst; reported is the median of --samples samples after a warm-up, and the
host time one step takes to enqueue; lav_optim_grad_stats (the first two launches) the same way.  The update launch alone is timed by
the library's own HIP events around it (lav_profile_enable) over --samples further steps; its bytes are 28 per element (p, g, m, v read,
p, m, v written), against the 6.3 TB/s of HBM that are achievable.

--ema adds, per trainer, the moving average of the weights (lav_optim_adam_ema_step, FusedAdam(ema_decay=)): three variants over their own
copies of the same tensors ALTERNATE in one process, round after round - the fused step, the fused step with the shadow inside its update
launch, and the fused step followed by torch._foreach_lerp_ over the same tensors (the separate-launch alternative) - each timed as
above per round, and the update launch alone by the library's timers in both of its instantiations.  Reported are the medians over
the rounds, the spread (min, max) of the per-round ratios, and the ratio against bytes alone, 36 / 28.  With --only-ema the file's
other keys are kept as they are.

Reports; asserts no threshold.  Fails without a GPU: a time measured elsewhere says nothing about the MI355X.

    python tools/optim_probe.py [--samples 200] [--burst 20] [--ema] [--only-ema] [--rounds 9] [--out profiles/optim_probe.json]
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


def _update_launch_ms(lib, step, steps):
    """The mean time of the update launch over `steps` steps, by the library's HIP events around it."""
    lib.lav_profile_reset()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms, n = ctypes.c_double(), ctypes.c_int()
    lib.lav_profile_read(b"optim_update", ctypes.byref(ms), ctypes.byref(n))
    assert n.value == steps, (n.value, steps)
    return ms.value / steps


def _spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def ema_case(what, rounds, burst, decay=0.999):
    torch.manual_seed(0)
    lav = LAV(TrainConfig(log_inference=False), "cuda", what=what)
    shapes = [tuple(p.shape) for g in getattr(lav, f"{what}_optim").param_groups for p in g["params"]]
    del lav
    gen = torch.Generator(device="cuda").manual_seed(1)
    sets = []
    for _ in range(3):
        ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen)) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-2
        sets.append(ps)
    plain, ema, sep = FusedAdam(sets[0], lr=3e-4), FusedAdam(sets[1], lr=3e-4, ema_decay=decay), FusedAdam(sets[2], lr=3e-4)
    shadows = [p.detach().clone() for p in sets[2]]
    live = [p.detach() for p in sets[2]]

    def separate():
        sep.step()
        torch._foreach_lerp_(shadows, live, 1.0 - decay)

    variants = {"fused": plain.step, "fused_ema": ema.step, "fused_plus_foreach_lerp": separate}
    for fn in variants.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    lib = _lib.load()
    step_ms = {k: [] for k in variants}
    host_ms = {k: [] for k in variants}
    launch_ms = {"fused": [], "fused_ema": []}
    for _ in range(rounds):
        for name, fn in variants.items():       # the variants alternate: a drift of the clocks meets all of them
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(burst):
                fn()
            host_ms[name].append((time.perf_counter() - t0) * 1e3 / burst)
            e1.record()
            e1.synchronize()
            step_ms[name].append(e0.elapsed_time(e1) / burst)
        lib.lav_profile_enable(4096)
        for name in launch_ms:
            launch_ms[name].append(_update_launch_ms(lib, variants[name], burst))
        lib.lav_profile_enable(0)
    numel = sum(p.numel() for p in sets[0])
    a = lambda k, table: np.asarray(table[k])
    res = {"tensors": len(shapes), "elements": numel, "rounds": rounds, "burst": burst, "ema_decay": decay,
           "step_ms": {k: _spread(v) for k, v in step_ms.items()}, "host_enqueue_ms": {k: _spread(v) for k, v in host_ms.items()},
           "update_launch_ms": {k: _spread(v) for k, v in launch_ms.items()},
           "update_launch_ema_over_plain": _spread(a("fused_ema", launch_ms) / a("fused", launch_ms)), "bytes_alone_ratio": 36 / 28,
           "update_ema_bytes_per_s": 36 * numel / (float(np.median(launch_ms["fused_ema"])) * 1e-3),
           "step_ema_over_plain": _spread(a("fused_ema", step_ms) / a("fused", step_ms)),
           "step_ema_over_separate_lerp": _spread(a("fused_ema", step_ms) / a("fused_plus_foreach_lerp", step_ms))}
    res["update_ema_fraction_of_hbm"] = res["update_ema_bytes_per_s"] / HBM_ACHIEVABLE
    assert ema.health()["skipped"] == 0 and plain.health()["skipped"] == 0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--ema", action="store_true", help="also the moving average: keys ema_lidar / ema_bev")
    ap.add_argument("--only-ema", action="store_true", help="the EMA cases alone; the other keys of --out stay as they are")
    ap.add_argument("--rounds", type=int, default=9, help="--ema: rounds in which the variants alternate")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optim_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    if args.only_ema:
        with open(args.out) as f:
            res = json.load(f)
    else:
        res = {"device": torch.cuda.get_device_name(0), "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
               "lidar": case("lidar", args.samples, args.burst), "bev": case("bev", args.samples, args.burst)}
    if args.ema or args.only_ema:
        res["ema_lidar"] = ema_case("lidar", args.rounds, args.burst)
        res["ema_bev"] = ema_case("bev", args.rounds, args.burst)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
