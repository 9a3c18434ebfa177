"""ERFNet's two entry DownsamplerBlocks alone (3 -> 16 -> 64 channels on three 288 x 256 cameras, raw input with (2/255, -1) folded in):
the four launches of the blocks' own engines against lav_erfnet_entry, back to back from a HIP graph of 20 copies each, the variants
alternated `--rounds` times in one process (the protocol of tools/bev_tile_stage.py).  Prints us per stage.

    python tools/erfnet_edge_stage.py [--rounds 5] [--reps 50]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lav_amd import erfnet, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()
DEV = torch.device("cuda", 0)
B, H, W, IN_GRAPH = 3, 288, 256, 20
AFFINE = (2.0 / 255.0, -1.0)
g = torch.Generator().manual_seed(1)
blocks = []
for cin, cout in ((3, 16), (16, 64)):
    blk = erfnet.DownsamplerBlock(cin, cout).eval()
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
        blk.bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.1)
        blk.bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
    blocks.append(blk)
x = torch.randint(0, 256, (B, 3, H, W), generator=g).float().to(DEV)

with ops.precision(ops.frame_precision()):
    first, second = blocks[0].engine(DEV, AFFINE), blocks[1].engine(DEV)
    fused = erfnet._entry_stage(blocks[0], blocks[1], DEV, AFFINE, first, second)
    variants = {"four_launches": lambda: second(first(x)), "entry": lambda: fused(x)}
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
    want = variants["four_launches"]().clone()
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
print(json.dumps(dict(us_per_stage=res, best={n: min(r) for n, r in res.items()}, spread={n: round(max(r) - min(r), 2) for n, r in res.items()},
                      max_abs_diff_to_four_launches=diff, out_absmax=want.abs().max().item())))
