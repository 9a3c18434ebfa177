"""Stage s1 of the BEV backbone alone (layers 2-4 of ConvBackbone.conv1: 64 -> 64 channels, 3x3, 160 x 160): the three per-layer launches
against lav_conv3x3_tile_f16 (ops.ConvTileRun) and against two layers fused + one per-layer launch, back to back from a HIP graph of 20
copies each, the variants alternated `--rounds` times in one process.  Prints us per stage.

    python tools/bev_tile_stage.py [--rounds 5] [--reps 50]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lav_amd import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()
DEV = torch.device("cuda", 0)
C, H, W, L, IN_GRAPH = 64, 160, 160, 3, 20
g = torch.Generator().manual_seed(1)
layers = []
for _ in range(L):
    w = torch.randn((C, C, 3, 3), generator=g) * (2.0 / (9 * C)) ** 0.5
    bn = (torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1)
    layers.append(ops.ConvLayer(w, padding=1, bn=bn, bn_eps=1e-3, relu_pre=True, precision=_lib.CONV_F16X3, device=DEV))
x = torch.randn((1, C, H, W), generator=g).abs().to(DEV)
am_x = ops.Amax(DEV)
am_x.take(1).fill_(x.abs().max())
ams = [ops.Amax(DEV) for _ in range(L)]
bufs = [torch.empty_like(x) for _ in range(L)]
tile3, tile2 = ops.ConvTileRun(layers), ops.ConvTileRun(layers[:2])


def per_layer():
    y, am = x, am_x
    for l, nxt, out in zip(layers, ams, bufs):
        y = l(y, out=out, amax_in=am, amax_out=nxt.reset())
        am = nxt
    return y


def tile():
    return tile3(x, out=bufs[2], amax_in=am_x, amax_out=ams[2].reset())


def tile_2_plus_1():
    y = tile2(x, out=bufs[1], amax_in=am_x, amax_out=ams[1].reset())
    return layers[2](y, out=bufs[2], amax_in=ams[1], amax_out=ams[2].reset())


variants = {"per_layer": per_layer, "tile": tile, "tile_2_plus_1": tile_2_plus_1}
side = torch.cuda.Stream(DEV)
graphs = {}
for name, fn in variants.items():
    with torch.cuda.stream(side):
        fn()
    side.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        for _ in range(IN_GRAPH):
            fn()
    graphs[name] = gr
want = per_layer().clone()
diff = {n: (fn() - want).abs().max().item() for n, fn in variants.items()}
res = {n: [] for n in variants}
for _ in range(a.rounds):
    for name, gr in graphs.items():
        for _ in range(3):
            gr.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        res[name].append(round(e0.elapsed_time(e1) * 1e3 / (a.reps * IN_GRAPH), 2))
print(json.dumps(dict(us_per_stage=res, best={n: min(r) for n, r in res.items()},
                      max_abs_diff_to_per_layer=diff, out_absmax=want.abs().max().item())))
