"""Time of the heads' pieces in isolation (library HIP events, back-to-back launches): fused first convolution, grouped
deconvolution, peak extraction.  python tools/heads_probe.py

Then the stage of the frame, LiDARModel.detect (heads + peaks -> the (2, 15, 7) rows), from a replayed HIP graph of 10 copies: the dense
four-head path and the heads-at-peaks path alternated in one process, --rounds rounds (default 6) of 50 replays each; us per stage."""
import ctypes
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from lav_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda:0")
lib = _lib.load()
pipe, sds, (lm, up, seg, bra) = bench.build_pipeline(dev, eager=True)
feats = torch.randn((1, 384, 160, 160), device=dev)


def read(name):
    ms, n = ctypes.c_double(), ctypes.c_int()
    lib.lav_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(n))
    return ms.value / max(n.value, 1) * 1e3, n.value


with torch.no_grad():
    heat, size, ori, bev = lm.heads(feats)
    fn = lambda: (lm.heads(feats), ops.extract_peaks(heat[0], size[0], ori[0], apply_sigmoid=True))
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    lib.lav_profile_enable(400)
    fn(); torch.cuda.synchronize(); lib.lav_profile_reset()
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    print(f"LAV_DECONV_IMPL={os.environ.get('LAV_DECONV_IMPL', 'staged')}: " + ", ".join(f"{k} {read(k)[0]:.1f} us" for k in ("conv2d", "deconv_grouped", "extract_peaks")))

# ---- the stage from a replayed graph, both paths alternated
rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 6
COPIES, REPLAYS = 10, 50
graphs = {}
lib.lav_profile_enable(0)     # no event records inside the captures
with torch.no_grad(), ops.precision(ops.frame_precision()):
    for name, at_peaks in (("dense", False), ("at_peaks", True)):
        for _ in range(3):
            lm.detect(feats, at_peaks=at_peaks)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(COPIES):
                keep = lm.detect(feats, at_peaks=at_peaks)
        graphs[name] = (g, keep)
    times = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, (g, _) in graphs.items():
            g.replay(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPLAYS):
                g.replay()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / (REPLAYS * COPIES) * 1e6)
for name, t in times.items():
    print(f"detect[{name}] us per stage, {rounds} alternated rounds: " + " ".join(f"{v:.2f}" for v in t) + f"   best {min(t):.2f} spread {max(t) - min(t):.2f}")
lib.lav_profile_enable(400)
with torch.no_grad(), ops.precision(ops.frame_precision()):
    for _ in range(50):
        lm.detect(feats, at_peaks=True)
torch.cuda.synchronize()
print("at_peaks, back to back (library events): " + ", ".join(f"{k} {read(k)[0]:.1f} us x{read(k)[1]}" for k in ("conv2d", "deconv_grouped", "extract_peaks", "heads_at_peaks")))
