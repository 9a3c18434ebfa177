#!/usr/bin/env python3
"""What the agent's debug view costs on an MI355X.

(a) Kernel: HIP events around --launches calls of lav_debug_view (zeroing, histogram and compose launches) after warm-up at the
    agent's geometry - 288 x 768 and 192 x 480 images, a 196 608-row cloud, the 320 x 320 grid, a 160 x 1146 frame - for 0, 7 and
    15 vehicles (20 + 120 n + 4 n + 1 records), the records resident; and the same through ops.debug_view, which uploads the
    records and the text with every call.
(b) Agent: ticks per second of LAVAgent.run_step over synth.agent_scenario() with `debug_view` on and off (synthetic weights,
    HIP graphs, the inputs of --ticks ticks prepared beforehand and replayed --rounds times, the two agents interleaved).

Reports; asserts no threshold.  Fails without a GPU: a time measured elsewhere says nothing about the MI355X.

    python tools/debug_view_probe.py [--launches 50] [--ticks 40] [--rounds 3] [--out profiles/debug_view_probe.json]
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
from lav_amd import _lib, ops, synth  # noqa: E402
from lav_amd.agent import RoadOption  # noqa: E402
from lav_amd.agent import debug_view as V  # noqa: E402

GRID = (-10, 70, -40, 40, 4)


def scene(n, rng):
    f32 = np.float32
    plan = np.stack([rng.normal(0, 0.3, 20), -np.arange(20) * 0.5], 1).astype(f32)
    starts = rng.uniform((-30, -60), (30, 5), (n, 1, 1, 2))
    locs = (starts + np.cumsum(rng.normal(0, 0.3, (n, 6, 20, 2)), axis=2)).astype(f32)
    cmds = rng.uniform(0.2, 1.0, (n, 6)).astype(f32)
    det = [[], [(float(160 + 4 * s[0, 0, 0]), float(280 + 4 * s[0, 0, 1]), 4.0, 9.0, 1.0, 0.0) for s in starts]]
    return V.primitives(plan, locs, cmds, det, [1.0, -20.0], ppm=GRID[4], cmd_thresh=0.2)


def kernel_case(launches):
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    rgb = torch.from_numpy(rng.integers(0, 256, (288, 768, 3), dtype=np.uint8)).to(dev)
    tel = torch.from_numpy(rng.integers(0, 256, (192, 480, 3), dtype=np.uint8)).to(dev)
    pts = torch.from_numpy(np.concatenate([rng.normal(0, 18, (196608, 2)) + [25, 0], rng.normal(size=(196608, 9))], 1).astype(np.float32)).to(dev)
    bev = torch.from_numpy(rng.uniform(0, 1, (3, 320, 320)).astype(np.float32)).to(dev)
    text = V.text_rows(3, 4.2, -0.1, 0.5, 0.0, 0.03)
    out = torch.empty((160, 1146, 3), dtype=torch.uint8, device=dev)
    lay = V.layout(rgb.shape, tel.shape, GRID, bev.shape)
    (x0, x1, nxb), (y0, y1, nyb) = V.grid_bins(GRID)
    font, lut = torch.from_numpy(V.FONT.copy()).to(dev), torch.from_numpy(V.HIST_LUT.copy()).to(dev)
    tables = torch.from_numpy(V.resize_tables(rgb.shape, tel.shape, lay)).to(dev)
    counts = torch.zeros(nxb * nyb, dtype=torch.int32, device=dev)
    text_d = torch.from_numpy(text).to(dev)
    lib = _lib.load()
    res = {}
    for n in (0, 7, 15):
        prims = scene(n, rng)
        prims_d = torch.from_numpy(prims.view(np.uint8).reshape(-1).copy()).to(dev)

        def resident():
            _lib.check(lib.lav_debug_view(rgb.data_ptr(), 288, 768, tel.data_ptr(), 192, 480, pts.data_ptr(), pts.shape[0], pts.shape[1], bev.data_ptr(),
                                          320, prims_d.data_ptr(), len(prims), text_d.data_ptr(), text.shape[1], font.data_ptr(), lut.data_ptr(),
                                          tables.data_ptr(), x0, x1, nxb, y0, y1, nyb, lay["w_rgb"], lay["w_tel"], counts.data_ptr(), out.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "lav_debug_view")

        def uploaded():
            ops.debug_view(rgb, tel, pts, bev, prims, text, grid=GRID, out=out)

        row = {"records": int(len(prims))}
        for name, fn in (("stream_ops_ms", resident), ("with_upload_ms", uploaded)):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            row[name] = e0.elapsed_time(e1) / launches
        res[f"vehicles_{n}"] = row
    return res


def agent_case(ticks, rounds):
    from lav_amd.lav_agent import LAVAgent
    sc = synth.agent_scenario()
    data = [synth.agent_inputs(i, sc) for i in range(ticks)]
    res = {}
    with tempfile.TemporaryDirectory() as root:
        agents = {}
        for on in (False, True):
            path = os.path.join(root, f"cfg_{on}.yaml")
            with open(path, "w") as f:
                yaml.safe_dump(dict(synthetic_weights=True, points_per_tick=8192, debug_view=on, debug_view_dir=os.path.join(root, "views"),
                                    debug_view_flush=ticks + 1), f)     # (the ring never fills: the steady state between two flushes)
            a = LAVAgent(path)
            a.set_global_plan([({"lat": la, "lon": lo, "z": 0.0}, RoadOption(int(c))) for la, lo, c in zip(sc["lat"], sc["lon"], sc["cmds"])])
            agents[on] = a
        rates = {False: [], True: []}
        for r in range(rounds + 1):                 # round 0 warms up
            for on, a in agents.items():
                a.num_frames = 1 if r else 0        # (the first tick of a drive only stashes its sweep)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i, d in enumerate(data):
                    a.run_step(d, i * 0.05)
                torch.cuda.synchronize()
                if r:
                    rates[on].append(len(data) / (time.perf_counter() - t0))
                a.vizs.clear()
        for on, a in agents.items():
            a.destroy()
        res = {"ticks": ticks, "rounds": rounds, "ticks_per_s_view_off": float(np.median(rates[False])), "ticks_per_s_view_on": float(np.median(rates[True])),
               "all_view_off": rates[False], "all_view_on": rates[True]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "debug_view_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("debug_view_probe: no GPU; a time measured elsewhere says nothing about the MI355X")
    res = {"device": torch.cuda.get_device_name(0), "frame_bytes": 160 * 1146 * 3, "kernel": kernel_case(args.launches), "agent": agent_case(args.ticks, args.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
