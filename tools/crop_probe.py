#!/usr/bin/env python3
"""The four rotated-crop kernels of crop.hip, timed with the library's own HIP-event timers (`crop_rotate`, `crop_rotate_backward`),
not a Python loop - a single crop is 19 us of launches from Python whatever the kernel takes - and each forced through the library's
two knobs (LAV_CROP_FWD_GENERAL / LAV_CROP_BWD_GENERAL, read on every call):

    python tools/crop_probe.py             forward at the frame's crop counts (1 ... 15) and the trainers' (96), 96 x 96 from 384 x 160 x 160,
                                           staged and gathering kernel; backward of 96 crops into 32 maps (train_full's sizes), staged and
                                           general kernel; then the agreement check
    python tools/crop_probe.py --check     the agreement check alone: forward and map gradient of a small case (3 maps of 40 x 40 x 40,
                                           5 crops of 24 x 24, two maps shared) against torch's grid_sample and its backward in float64 on
                                           the CPU, with every pair of kernels; exit status 1 beyond 2e-5 / 5e-5 of the largest gradient
    python tools/crop_probe.py --digest    sha256 of the forward output and of the map gradient on seeded data over the geometries of
                                           tests/crop_util.GEOMETRIES, 1 / 2 / 48 / 300 crops (300: two passes of the backward's crop list;
                                           1: 16 channels per workgroup), the library's dispatch and each knob - to compare two builds
                                           (LAV_AMD_LIB=other/liblav_amd.so) line for line.  LAV_CROP_CPB (8, 16, 32) is read once per
                                           process: with it set, only the forward lines of the staged 40 x 40 geometry are printed.
"""
import ctypes
import hashlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from lav_amd import _lib, ops  # noqa: E402

DEV = torch.device("cuda", 0)
KNOBS = {"dispatch": None, "fwd_general": "LAV_CROP_FWD_GENERAL", "bwd_general": "LAV_CROP_BWD_GENERAL"}


def select(kernels):
    for name, var in KNOBS.items():
        if var and name == kernels:
            os.environ[var] = "1"
        elif var:
            os.environ.pop(var, None)


def timed(lib, name, launch, reps):
    """us per launch of timer `name` over `reps` back-to-back launches (one more, untimed, first)."""
    lib.lav_profile_enable(64)
    launch(); torch.cuda.synchronize(); lib.lav_profile_reset()
    for _ in range(reps):
        launch()
    torch.cuda.synchronize()
    ms, n = ctypes.c_double(), ctypes.c_int()
    lib.lav_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(n))
    lib.lav_profile_enable(0)
    assert n.value == reps, f"{name}: {n.value} launches recorded, {reps} made"
    return ms.value / n.value * 1e3


def times(lib):
    feat = torch.randn((1, 384, 160, 160), device=DEV)
    for n in (1, 2, 4, 7, 15, 96):
        locs = torch.tensor([[3.0 * (i % 9), -5.0 - (i % 7)] for i in range(n)], device=DEV)
        oris = torch.tensor([0.3 * i for i in range(n)], device=DEV)
        launch = lambda: ops.crop_rotate(feat, locs, oris, 2.0, 96, 0.0, 0.75)
        us = {}
        for kernels in ("dispatch", "fwd_general"):
            select(kernels)
            for _ in range(5):
                launch()
            us[kernels] = timed(lib, "crop_rotate", launch, 50)
        nb = n * 384 * 96 * 96 * 4 * 2
        print(f"forward  n={n:3d}: staged {us['dispatch']:7.1f} us ({nb / us['dispatch'] / 1e3:5.0f} GB/s of the algorithmic 2 x output bytes), "
              f"gathering {us['fwd_general']:7.1f} us", flush=True)
    del feat
    M, C, H, W, n, crop = 32, 384, 160, 160, 96, 96
    g = torch.Generator().manual_seed(0)
    feat = torch.randn((M, C, H, W), generator=g).to(DEV).requires_grad_(True)
    idx = (torch.arange(n) % M).int().to(DEV)
    locs = ((torch.rand((n, 2), generator=g) - 0.5) * 30).to(DEV)
    oris = ((torch.rand(n, generator=g) - 0.5) * 6.2).to(DEV)
    select("dispatch")
    out = ops.crop_rotate_indexed(feat, idx, locs, oris, 4.0, crop, 0.0, 0.75)
    w = torch.randn(out.shape, device=DEV)

    def backward():
        feat.grad = None
        out.backward(w, retain_graph=True)
    us = {}
    for kernels in ("dispatch", "bwd_general"):
        select(kernels)
        us[kernels] = timed(lib, "crop_rotate_backward", backward, 20)
    nb = 4 * (w.numel() + feat.numel())
    print(f"backward {n} crops into {M} maps: staged {us['dispatch']:8.1f} us ({nb / us['dispatch'] / 1e3:5.0f} GB/s of grad_out read + grad_feat "
          f"written), general {us['bwd_general']:8.1f} us", flush=True)
    select("dispatch")


def check():
    from lav_amd.planner_common import crop_feature_torch
    g = torch.Generator().manual_seed(4)
    H, W, crop = 40, 40, 24
    feat = torch.randn((3, 40, H, W), generator=g)
    idx = torch.tensor([2, 0, 0, 1, 2], dtype=torch.int32)
    locs = torch.tensor([[0.0, 0.0], [1.5, -3.0], [-2.0, 1.0], [3.0, -2.0], [9.0, -9.0]])
    oris = torch.tensor([0.0, 0.4, -1.1, 3.0, 0.2])
    f_ref = feat.double().requires_grad_(True)
    ref = crop_feature_torch(f_ref[idx.long()], locs.double(), oris.double(), 2.0, crop, 0.0, 0.75)
    w = torch.randn(ref.shape, generator=g)
    (ref * w.double()).sum().backward()
    scale = float(f_ref.grad.abs().max())
    ok = True
    for fwd in ("dispatch", "fwd_general"):
        for bwd in ("dispatch", "bwd_general"):
            f_gpu = feat.to(DEV).requires_grad_(True)
            select(fwd)
            out = ops.crop_rotate_indexed(f_gpu, idx.to(DEV), locs.to(DEV), oris.to(DEV), 2.0, crop, 0.0, 0.75)
            select(bwd)
            (out * w.to(DEV)).sum().backward()
            e_out = float((out.detach().cpu().double() - ref.detach()).abs().max())
            e_grad = float((f_gpu.grad.cpu().double() - f_ref.grad).abs().max())
            good = e_out <= 2e-5 and e_grad <= 5e-5 * scale
            ok &= good
            print(f"check forward {fwd:11s} backward {bwd:11s}: max |out - grid_sample| {e_out:.2e}, max |grad - its backward| {e_grad:.2e} "
                  f"(largest gradient {scale:.2f}) {'ok' if good else 'WRONG'}", flush=True)
    select("dispatch")
    return ok


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:32]


def digest():
    from tests import crop_util as cu
    cpb = os.environ.get("LAV_CROP_CPB")
    C = 40
    for geom in ([(40, 40, 24)] if cpb else cu.GEOMETRIES):
        H, W, crop = geom
        for n in (1, 2, 48, 300):
            M = min(n, 3)
            g = torch.Generator().manual_seed(1000 * H + n)
            feat = torch.randn((M, C, H, W), generator=g).to(DEV)
            w = torch.randn((n, C, crop, crop), generator=g).to(DEV)
            idx = (torch.arange(n) % M).int().to(DEV)
            locs, oris = (t.to(DEV) for t in cu.random_poses(H, W, n, seed=n))
            for kernels in (["dispatch"] if cpb else KNOBS):
                select(kernels)
                f = feat.clone().requires_grad_(True)
                out = ops.crop_rotate_indexed(f, idx, locs, oris, cu.PPM, crop, *cu.OFFSETS[0])
                line = f"{cu.geom_id(geom)} n={n} {'cpb=' + cpb if cpb else kernels} forward {sha(out)}"
                if not cpb:
                    out.backward(w)
                    line += f" gradient {sha(f.grad)}"
                print(line, flush=True)
    select("dispatch")


if __name__ == "__main__":
    _lib.require_device()
    lib = _lib.load()
    if "--digest" in sys.argv:
        digest()
    elif "--check" in sys.argv:
        sys.exit(0 if check() else 1)
    else:
        times(lib)
        sys.exit(0 if check() else 1)
