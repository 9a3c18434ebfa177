#!/usr/bin/env python3
"""What the eval tools' --bootstrap resampling costs on an MI355X.

For (R blocks, W words, B replicates) = (1 000, 279, 1 000), (10 000, 512, 1 000) and (1 000, 8 462, 1 000), on a seeded int64 table
resident in HBM:
  kernel   one HIP event pair around EACH of --launches calls of ops.eval_resample after warm-up: median, quartiles, minimum, maximum.
           The window of one call holds the wrapper's checks and the allocation of the output.
  torch    the same sums by rows[idx].sum(1) on the device, in replicate chunks of at most 1 GiB of gathered rows, with the indices
           (eval_common.resample_indices) already in HBM: their generation is NOT in the window.  Median of --torch-rounds.
  numpy    eval_resample_numpy on the host over the first --host-replicates replicates, in seconds, and that time scaled by
           B / host-replicates: the work is linear in B, and the scaled figure is an extrapolation, named as one.
  copy     a device-to-device copy of B R W 8 bytes (a 1 GiB buffer copied as often as that takes): what moving the gathered bytes
           once costs at the copy's bandwidth, the yardstick for the kernel's B-fold re-read of the table.
The kernel's and torch's outputs are compared word by word.  Reports; asserts no threshold.  Fails without a GPU: a time measured
elsewhere says nothing about the MI355X.

    python tools/eval_resample_probe.py [--launches 50] [--torch-rounds 5] [--host-replicates 100] [--out profiles/eval_resample_probe.json]
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
from lav_amd.train import eval_common as C  # noqa: E402

SHAPES = ((1000, 279, 1000), (10000, 512, 1000), (1000, 8462, 1000))
SEED = 2021
GIB = 1 << 30


def _timed(fn, rounds):
    """Milliseconds of each of `rounds` calls of fn, one event pair per call."""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)]
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return np.array([e0.elapsed_time(e1) for e0, e1 in pairs])


def case(R, W, B, launches, torch_rounds, host_replicates):
    rows_host = np.random.default_rng(R + W).integers(-(1 << 40), 1 << 40, (R, W), dtype=np.int64)
    rows = torch.from_numpy(rows_host).cuda()
    gathered = B * R * W * 8
    for _ in range(5):
        out = ops.eval_resample(rows, B, SEED)
    torch.cuda.synchronize()
    ms = _timed(lambda: ops.eval_resample(rows, B, SEED), launches)
    q = lambda p: float(np.percentile(ms, p))
    res = {"R": R, "W": W, "B": B, "table_bytes": R * W * 8, "gathered_bytes": gathered,
           "kernel": {"launches": launches, "median_ms": q(50), "p25_ms": q(25), "p75_ms": q(75), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                      "gathered_TB_per_s_at_median": gathered / (q(50) * 1e-3) / 1e12}}

    per = max(1, GIB // (R * W * 8))                                # replicates per gather
    idx = torch.from_numpy(C.resample_indices(R, np.arange(1, B + 1), SEED)).cuda()
    by_torch = torch.empty((B + 1, W), dtype=torch.int64, device="cuda")

    def torch_sums():
        by_torch[0] = rows.sum(dim=0)
        for b0 in range(0, B, per):
            by_torch[1 + b0:1 + b0 + per] = rows[idx[b0:b0 + per]].sum(dim=1)
    torch_sums()
    torch.cuda.synchronize()
    res["kernel_equals_torch"] = bool(torch.equal(out, by_torch))
    tms = _timed(torch_sums, torch_rounds)
    res["torch"] = {"rounds": torch_rounds, "replicates_per_gather": per, "median_ms": float(np.median(tms)), "min_ms": float(tms.min()),
                    "max_ms": float(tms.max()), "indices": "in HBM before the window"}

    n = min(B, host_replicates)
    t0 = time.perf_counter()
    by_numpy = C.eval_resample_numpy(rows_host, n, SEED)
    dt = time.perf_counter() - t0
    res["numpy"] = {"replicates": n, "seconds": dt, "seconds_scaled_to_B": dt * B / n, "scaled": "extrapolated, linear in B; not measured" if n < B else "measured",
                    "equals_kernel": bool(np.array_equal(by_numpy, out[:n + 1].cpu().numpy()))}

    src = torch.empty(min(gathered, GIB), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    times = -(-gathered // src.numel())

    def copies():
        for _ in range(times):
            dst.copy_(src)
    copies()
    torch.cuda.synchronize()
    cms = _timed(copies, 5)
    moved = times * src.numel()
    res["copy"] = {"bytes": moved, "buffer_bytes": src.numel(), "copies": times, "median_ms": float(np.median(cms)),
                   "TB_per_s_read_plus_written": 2 * moved / (float(np.median(cms)) * 1e-3) / 1e12}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--torch-rounds", type=int, default=5)
    ap.add_argument("--host-replicates", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_resample_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_resample_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    res = {"device": torch.cuda.get_device_name(0), "chunk": ops.eval_resample_chunk(), "seed": SEED,
           "cases": [case(R, W, B, args.launches, args.torch_rounds, args.host_replicates) for R, W, B in SHAPES]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
