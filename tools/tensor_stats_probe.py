#!/usr/bin/env python3
"""What --tensor-stats costs on an MI355X: the two launches of lav_optim_tensor_stats, the launch of lav_optim_blame, and
FusedAdam.step() with the flag at N = 1 and N = 100 against FusedAdam.step() without it (the code path of a run that never asked), on
the parameter shapes of LAV(what="lidar") (train_full) and LAV(what="bev") (train_bev).

The variants step their own copies of the trained parameters on fixed random gradients and ALTERNATE in one process, round after
round: a sample is the time between two HIP events around --burst back-to-back calls, divided by the burst; reported are the median and
[min, max] over --rounds rounds.  The N = 100 variant takes its rows at every 100th of its own steps, so over a burst of 20 it mostly
measures the blame launch that every step carries.  The stats pass reads 16 bytes per element (g, p, m, v) where the update launch moves
28; the update launch alone is timed by the library's own HIP events (lav_profile_enable) for that comparison.

--stats-only times the two stats launches alone: with LAV_AMD_LIB pointing at another build of the library it compares two forms of
the kernel (a process per build, alternating in the caller's loop).

Reports; asserts no threshold.  Fails without a GPU: a time measured elsewhere says nothing about the MI355X.

    python tools/tensor_stats_probe.py [--rounds 9] [--burst 20] [--stats-only] [--out profiles/tensor_stats_probe.json]
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


def _spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def _optimiser(shapes, gen, names):
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen)) for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-2
    watch = [torch.ones(64, device="cuda") for _ in range(40)]        # BatchNorm-sized buffers
    kw = dict(names=([f"p{i}" for i in range(len(ps))], [f"b{i}" for i in range(len(watch))])) if names else {}
    return FusedAdam(ps, lr=3e-4, watch=watch, **kw)


def case(what, rounds, burst, stats_only):
    torch.manual_seed(0)
    lav = LAV(TrainConfig(log_inference=False), "cuda", what=what)
    shapes = [tuple(p.shape) for g in getattr(lav, f"{what}_optim").param_groups for p in g["params"]]
    del lav
    gen = torch.Generator(device="cuda").manual_seed(1)
    off, every, sparse = _optimiser(shapes, gen, False), _optimiser(shapes, gen, True), _optimiser(shapes, gen, True)
    count = [0]

    def step_n1():
        every.step()
        every.tensor_stats()

    def step_n100():
        sparse.step()
        if count[0] % 100 == 0:
            sparse.tensor_stats()
        count[0] += 1

    every.step()
    n, chunks, nw, wchunks = every._counts
    rows = torch.zeros(n * 576 + nw * 16, dtype=torch.uint8, device="cuda")
    stats = lambda: ops.optim_tensor_stats(every._table, n, chunks, every._watch_table, nw, wchunks, every._words, rows[:n * 576], rows[n * 576:])
    blame = lambda: ops.optim_blame(every._table, n, chunks, every._watch_table, nw, wchunks, every._global, every._blame)
    variants = {"tensor_stats_launches": stats}
    if not stats_only:
        variants.update({"blame_launch": blame, "step_flag_off": off.step, "step_tensor_stats_1": step_n1, "step_tensor_stats_100": step_n100})
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    host = {k: [] for k in variants}
    update_ms = []
    lib = _lib.load()
    for _ in range(rounds):
        for name, fn in variants.items():       # the variants alternate: a drift of the clocks meets all of them
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(burst):
                fn()
            host[name].append((time.perf_counter() - t0) * 1e3 / burst)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / burst)
        if not stats_only:
            lib.lav_profile_enable(4096)
            lib.lav_profile_reset()
            for _ in range(burst):
                off.step()
            torch.cuda.synchronize()
            t, k = ctypes.c_double(), ctypes.c_int()
            lib.lav_profile_read(b"optim_update", ctypes.byref(t), ctypes.byref(k))
            update_ms.append(t.value / max(k.value, 1))
            lib.lav_profile_enable(0)
    extra = {}
    # the two stats launches apart, by the library's HIP events; then the same on gradients that are all zero: every element of a wave
    # in one bin, the worst case of a histogram in LDS
    for key in ("launches", "launches_zero_gradients"):
        lib.lav_profile_enable(4096)
        lib.lav_profile_reset()
        for _ in range(burst):
            stats()
        torch.cuda.synchronize()
        extra[key] = {}
        for name in ("optim_tensor_stats", "optim_tensor_reduce"):
            t, k = ctypes.c_double(), ctypes.c_int()
            lib.lav_profile_read(name.encode(), ctypes.byref(t), ctypes.byref(k))
            extra[key][name] = {"calls": k.value, "mean_ms": t.value / max(k.value, 1)}
        lib.lav_profile_enable(0)
        for group in every.param_groups:
            for p in group["params"]:
                p.grad.zero_()
    numel = sum(int(np.prod(s)) for s in shapes)
    res = {"tensors": len(shapes), "elements": numel, "chunks": chunks, "watched": nw, "rounds": rounds, "burst": burst,
           "ms": {k: _spread(v) for k, v in ms.items()}, "host_enqueue_ms": {k: _spread(v) for k, v in host.items()},
           "stats_bytes": 16 * numel, "stats_bytes_per_s": 16 * numel / (float(np.median(ms["tensor_stats_launches"])) * 1e-3)}
    res["stats_fraction_of_hbm"] = res["stats_bytes_per_s"] / HBM_ACHIEVABLE
    res.update(extra)
    res["largest"] = max(int(np.prod(s)) for s in shapes)
    if not stats_only:
        a = lambda k: np.asarray(ms[k])
        res["update_launch_ms"] = _spread(update_ms)
        res["stats_over_update_launch"] = _spread(a("tensor_stats_launches") / np.asarray(update_ms))
        res["step_1_over_off"] = _spread(a("step_tensor_stats_1") / a("step_flag_off"))
        res["step_100_over_off"] = _spread(a("step_tensor_stats_100") / a("step_flag_off"))
        assert off.health()["skipped"] == 0 and every.health()["skipped"] == 0 and every.blame() == ([], [])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--stats-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tensor_stats_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tensor_stats_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
           "lidar": case("lidar", args.rounds, args.burst, args.stats_only), "bev": case("bev", args.rounds, args.burst, args.stats_only)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
