#!/usr/bin/env python3
"""What the agent's MJPEG recording costs on an MI355X.

(a) Encoder: ops.jpeg_encode (the wrapper and lav_jpeg_encode's three launches) at the agent's 160 x 1146 frame, one frame and a
    batch of 8, quality 90, the default restart interval: every call between two HIP events of its own, the median of --launches
    calls after warm-up; and the host time a call takes to enqueue.
(b) Agent: ticks per second of LAVAgent.run_step over synth.agent_scenario() with `debug_view` on in the npy and in the mjpeg format
    and off (synthetic weights, HIP graphs, the inputs of --ticks ticks prepared beforehand and replayed --rounds times, the three
    agents interleaved; the ring never fills, so this is the steady state between two flushes).  The npy agent is the recorder as it
    was before the mjpeg format existed.
(c) Bytes: mean bytes per frame (header, scan, EOI) of the mjpeg agent's drive - its cameras are the scenario's synthetic images - and
    of the rendered frame of tests/mjpeg_util.debug_frame, against the 550 080 bytes of a raw frame.

Reports; asserts no threshold.  Fails without a GPU: a time measured elsewhere says nothing about the MI355X.

    python tools/mjpeg_probe.py [--launches 200] [--ticks 40] [--rounds 3] [--out profiles/mjpeg_probe.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lav_amd import ops, synth  # noqa: E402
from lav_amd.agent import RoadOption  # noqa: E402
from lav_amd.agent import mjpeg as M  # noqa: E402


def encoder_case(launches, frame):
    res = {}
    for n in (1, 8):
        frames = torch.from_numpy(np.ascontiguousarray(np.stack([np.roll(frame, 7 * i, axis=1) for i in range(n)]))).cuda()
        out = torch.empty((n, M.scan_capacity(*frame.shape[:2])), dtype=torch.uint8, device="cuda")
        lengths = torch.empty((n,), dtype=torch.int32, device="cuda")
        for _ in range(20):
            ops.jpeg_encode(frames, 90, out=out, lengths=lengths)
        torch.cuda.synchronize()
        ms, host = [], []
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            ops.jpeg_encode(frames, 90, out=out, lengths=lengths)
            host.append((time.perf_counter() - t0) * 1e3)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        got = lengths.cpu().numpy()
        assert out[0, :got[0]].cpu().numpy().tobytes() == M.scan_numpy(frame, 90)
        res[f"batch_{n}"] = {"launches": launches, "median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "p90_ms": float(np.percentile(ms, 90)),
                             "host_enqueue_median_ms": float(np.median(host)), "scan_bytes": [int(v) for v in got]}
    return res


def agent_case(ticks, rounds):
    from lav_amd.lav_agent import LAVAgent
    sc = synth.agent_scenario()
    data = [synth.agent_inputs(i, sc) for i in range(ticks)]
    modes = {"off": dict(debug_view=False), "npy": dict(debug_view=True, debug_view_format="npy"), "mjpeg": dict(debug_view=True, debug_view_format="mjpeg")}
    with tempfile.TemporaryDirectory() as root:
        agents = {}
        for name, over in modes.items():
            path = os.path.join(root, f"cfg_{name}.yaml")
            with open(path, "w") as f:
                yaml.safe_dump(dict(synthetic_weights=True, points_per_tick=8192, debug_view_dir=os.path.join(root, name), debug_view_flush=ticks + 1, **over), f)
            a = LAVAgent(path)
            a.set_global_plan([({"lat": la, "lon": lo, "z": 0.0}, RoadOption(int(c))) for la, lo, c in zip(sc["lat"], sc["lon"], sc["cmds"])])
            agents[name] = a
        rates = {name: [] for name in modes}
        sizes = []
        for r in range(rounds + 1):                 # round 0 warms up
            for name, a in agents.items():
                a.num_frames = 1 if r else 0        # (the first tick of a drive only stashes its sweep)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i, d in enumerate(data):
                    a.run_step(d, i * 0.05)
                torch.cuda.synchronize()
                if r:
                    rates[name].append(len(data) / (time.perf_counter() - t0))
                if name == "mjpeg" and r == rounds:
                    sizes = [len(j) for j in a.vizs.frames_jpeg()]
                a.vizs.clear()                      # (outside the timed window; waits for the frames still in flight)
        for a in agents.values():
            a.destroy()
    res = {"ticks": ticks, "rounds": rounds}
    for name in modes:
        res[f"ticks_per_s_{name}"] = float(np.median(rates[name]))
        res[f"all_{name}"] = rates[name]
    res["mjpeg_over_npy"] = res["ticks_per_s_mjpeg"] / res["ticks_per_s_npy"]
    res["drive_frames"] = len(sizes)
    res["drive_mean_bytes_per_frame"] = float(np.mean(sizes)) if sizes else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mjpeg_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mjpeg_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    from tests.mjpeg_util import debug_frame
    frame = debug_frame()
    res = {"device": torch.cuda.get_device_name(0), "frame": list(frame.shape), "raw_frame_bytes": int(frame.size), "quality": 90,
           "restart_mcus": M.DEFAULT_RESTART_MCUS, "scan_capacity": M.scan_capacity(*frame.shape[:2]),
           "rendered_frame_bytes": len(M.jpeg_encode_numpy(frame, 90)), "encoder": encoder_case(args.launches, frame), "agent": agent_case(args.ticks, args.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
