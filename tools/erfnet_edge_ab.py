"""One side of the LAV_ERFNET_ENTRY A/B (the knob is read when the engine is built: one process per side, alternated by the caller):
bench.py's frame loop, `--rounds` rounds of `--steps` frames after 20 + 6 warm-up frames, the lidar graph replayed alone (best of
3 x 200 replays), and the health counters over all of it.  Prints one JSON line.

    LAV_ERFNET_ENTRY=0 python tools/erfnet_edge_ab.py; LAV_ERFNET_ENTRY=1 python tools/erfnet_edge_ab.py; ..."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from lav_amd import erfnet, ops  # noqa: E402

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


pipe.precapture(cmds=[3], max_others=8)
for _ in range(20):
    step()
torch.cuda.synchronize()
h0 = pipe.health()
frame_ms = []
for _ in range(a.rounds):
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    frame_ms.append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
h1 = pipe.health()
graphs = {}
for key, g in pipe.graphs.items():
    name = key if isinstance(key, str) else "_".join(str(k) for k in key)
    state = (pipe.ring.clone(), pipe.b_prev.clone())
    best = None
    for _ in range(3 if name == "lidar" else 1):
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
print(json.dumps(dict(LAV_ERFNET_ENTRY=os.environ.get("LAV_ERFNET_ENTRY", "default " + erfnet.ERFNET_ENTRY_DEFAULT), frame_ms=frame_ms, lidar_us=graphs.pop("lidar"),
                      other_graphs_us=graphs, nonfinite_outputs=h1["nonfinite_outputs"] - h0["nonfinite_outputs"],
                      timeouts=h1["pair_chain_timeouts"] - h0["pair_chain_timeouts"] + h1["plan_aborts"] - h0["plan_aborts"] + ops.bev_run_status(device)[0])))
