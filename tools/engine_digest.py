#!/usr/bin/env python3
"""sha256 of every packed tensor the inference engines hold, and of every model output on a fixed seeded input - to show that a change
of the host code between the nn.Modules and the C ABI leaves what is packed and what is computed bit for bit alone: run it on both
trees with the same library and compare the two outputs.
    python tools/engine_digest.py > digest.txt
The caches are found by walking whatever the modules keep beside their parameters (dicts, lists, tuples, the layer objects of
lav_amd.ops, the closures of ERFNet's stages), so the listing does not depend on how a tree stores them; lines are sorted per model."""
import hashlib
import os
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import lav_amd  # noqa: E402
from lav_amd import _lib, ops, synth  # noqa: E402
from lav_amd.rgb import RGBBrakePredictionModel, RGBSegmentationModel  # noqa: E402
from tests.util import CFG, Y_OFF, state_dicts  # noqa: E402

DEV = torch.device("cuda", 0)
PRECISIONS = (("f16x3", _lib.CONV_F16X3), ("default", 0))


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:32]


def packed(obj, label, out, seen):
    """(label, shape, sha256) of every tensor below `obj` that is not a parameter: the layer objects' public attributes, the
    containers' items and the closures' cells; Amax buffers (written by the launches) and anything private are left out."""
    if id(obj) in seen or isinstance(obj, (torch.nn.Module, torch.nn.Parameter, ops.Amax, types.ModuleType, str, int, float, bool, type(None))):
        return
    seen.add(id(obj))
    if torch.is_tensor(obj):
        if (obj.data_ptr(), tuple(obj.shape)) not in seen:
            seen.add((obj.data_ptr(), tuple(obj.shape)))
            out.append((label, tuple(obj.shape), sha(obj)))
    elif isinstance(obj, dict):
        for k, v in obj.items():
            if k not in ("amax", "tensor_ids", "device"):
                packed(v, label, out, seen)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            packed(v, label, out, seen)
    elif isinstance(obj, types.FunctionType):
        for v in list(vars(obj).values()) + [c.cell_contents for c in obj.__closure__ or ()]:
            packed(v, label, out, seen)
    elif type(obj).__module__ == "lav_amd.ops" and hasattr(obj, "__dict__"):
        for k, v in vars(obj).items():
            if not k.startswith("_"):
                packed(v, f"{type(obj).__name__}.{k}" if torch.is_tensor(v) else label, out, seen)


def report(name, model, outputs):
    lines = []
    for mod_name, mod in model.named_modules():
        found, seen = [], set()
        for k, v in vars(mod).items():
            if k.startswith("_") and k not in ("_parameters", "_buffers", "_modules") and not k.endswith("_hooks"):
                packed(v, "tensor", found, seen)
        lines += [f"{name} {mod_name or '.'} {type(mod).__name__} {label} {shape} {h}" for label, shape, h in found]
    print("\n".join(sorted(lines)))
    for what, t in outputs:
        print(f"{name} output {what} {tuple(t.shape)} {sha(t)}")
    sys.stdout.flush()


@torch.no_grad()
def main():
    _lib.require_device()
    g = torch.Generator().manual_seed(1234)
    rand = lambda *shape: torch.rand(*shape, generator=g)
    lsd, usd = state_dicts()
    lm = lav_amd.LiDARModel(num_input=16, backbone="cnn", num_features=[64, 64], **CFG)
    bp = lav_amd.BEVPlanner(pixels_per_meter=4, crop_size=96, feature_x_jitter=1.5, feature_angle_jitter=20, x_offset=0, y_offset=Y_OFF,
                            num_cmds=6, num_plan=20, num_plan_iter=5, num_frame_stack=2)
    up = lav_amd.UniPlanner(bp, pixels_per_meter=4, crop_size=96, feature_x_jitter=1.5, feature_angle_jitter=20, x_offset=0, y_offset=Y_OFF,
                            num_cmds=6, num_plan=20, num_input_feature=384, num_plan_iter=5)
    lm.load_state_dict(lsd); up.load_state_dict(usd)
    lm.eval().to(DEV); up.eval().to(DEV)
    # one segmenter per precision, so that the listing is the same for a tree whose ERFNet keeps the engine of its last call only
    segs, bra = {p: RGBSegmentationModel([4, 6, 7, 10, 18]) for p, _ in PRECISIONS}, RGBBrakePredictionModel([4, 6, 7, 10, 18])
    for seg in segs.values():
        seg.load_state_dict(synth.seeded_state_dict(seg, prefix="seg."))
        seg.eval().to(DEV)
    keep = {k: v.clone() for k, v in bra.state_dict().items() if k.startswith("normalize.")}      # (the ImageNet constants stay)
    bra.load_state_dict({**synth.seeded_state_dict(bra, prefix="bra."), **keep})
    bra.eval().to(DEV)

    pts = torch.from_numpy(synth.stacked_lidar(2048)).to(DEV)
    bev = (rand(1, 9, 320, 320) > 0.7).float().to(DEV)
    nxp = torch.tensor([[0.0, -10.0]], device=DEV)
    rgb, small = (rand(1, 3, 288, 256) * 255).to(DEV), (rand(1, 3, 64, 64) * 255).to(DEV)
    det = [(150.0, 120.0, 4.0, 2.0, 1.0, 0.0), (200.0, 180.0, 4.0, 2.0, 0.0, 1.0)]
    outs = {n: [] for n in ("lidar", "uni", "bra", *("seg-" + p for p in segs))}
    for pname, prec in PRECISIONS:
        with ops.precision(prec):
            res = lm([pts], [len(pts)])
            outs["lidar"] += [(f"{pname} {n}", t) for n, t in zip(("features", "center", "box", "ori", "seg"), res)]
            if prec == 0:
                outs["lidar"].append((f"{pname} center_head alone", lm.center_head(res[0])))
            plan, cast, oc, om = up.infer(res[0][0], det, 3, nxp[0])
            outs["uni"] += [(f"{pname} {n}", t) for n, t in zip(("ego_plan", "ego_cast", "other_cast", "other_cmds"), (plan, cast, oc, om))]
            outs["uni"] += [(f"{pname} teacher {n}", t) for n, t in zip(("plan", "cast", "cmds"), bp.infer(bev, nxp))]
            outs["seg-" + pname].append((f"{pname} probs", segs[pname].probs(rgb)))
            outs["bra"] += [(f"{pname} trunk 288x256", bra.trunk(rgb)), (f"{pname} trunk 64x64", bra.trunk(small))]
    torch.cuda.synchronize()
    for name, model in (("lidar", lm), ("uni", up), ("bra", bra), *(("seg-" + p, m) for p, m in segs.items())):
        report(name, model, outs[name])


if __name__ == "__main__":
    main()
