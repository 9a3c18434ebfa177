"""One side of the LAV_HEADS_AT_PEAKS A/B (the knob is read at import: one process per side, alternated by the caller): bench.py's
frame loop, `--rounds` rounds of `--steps` frames after 20 + 6 warm-up frames, every graph replayed alone (heads: best of 3 x 200
replays), the frame with the others branch forced to 0 and to 4 fixed poses (one round each), and the health counters over all of it.
Prints one JSON line.

    LAV_HEADS_AT_PEAKS=0 python tools/heads_peaks_ab.py; LAV_HEADS_AT_PEAKS=1 python tools/heads_peaks_ab.py; ..."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from lav_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
device = torch.device("cuda", 0)
pipe, sds, _ = bench.build_pipeline(device)
host, dev = bench.synthetic_inputs(device)
nt = len(dev["ticks"])
i = 0


def step():
    global i
    loc, ori = bench.pose(i)
    out = pipe.step(dev["ticks"][i % nt], dev["all_rgbs"], dev["rgbs"], dev["tel_rgbs"], loc, ori, dev["nxp"], 3)
    i += 1
    return out


def timed(steps):
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / steps * 1e3, 4)


pipe.precapture(cmds=[3], max_others=8)
for _ in range(20):
    step()
torch.cuda.synchronize()
h0 = pipe.health()
frame_ms = [timed(a.steps) for _ in range(a.rounds)]
graphs = {}
for key, g in pipe.graphs.items():
    name = key if isinstance(key, str) else "_".join(str(k) for k in key)
    state = (pipe.ring.clone(), pipe.b_prev.clone())
    best = None
    for _ in range(3 if name == "heads" else 1):
        for _ in range(5):
            g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            g.replay()
        torch.cuda.synchronize()
        t = (time.perf_counter() - t0) / 200 * 1e6
        best = t if best is None else min(best, t)
    graphs[name] = round(best, 1)
    pipe.ring.copy_(state[0]); pipe.b_prev.copy_(state[1])
forced = {}
for n in (0, 4):   # bench.py's forced_frames poses
    pipe.set_forced_others([[4.0 + 3.0 * k, -8.0 - 4.0 * k] for k in range(n)], [0.2 * k - 0.3 for k in range(n)])
    forced[n] = timed(a.steps)
pipe.set_forced_others(None)
h1 = pipe.health()
print(json.dumps(dict(LAV_HEADS_AT_PEAKS=os.environ.get("LAV_HEADS_AT_PEAKS", "default " + str(int(ops.frame_heads_at_peaks()))),
                      frame_ms=frame_ms, heads_us=graphs.pop("heads"), other_graphs_us=graphs, forced0_ms=forced[0], forced4_ms=forced[4],
                      nonfinite_outputs=h1["nonfinite_outputs"] - h0["nonfinite_outputs"], decode_mismatches=pipe.decode_mismatches,
                      timeouts=h1["pair_chain_timeouts"] - h0["pair_chain_timeouts"] + h1["plan_aborts"] - h0["plan_aborts"] + ops.bev_run_status(device)[0])))
