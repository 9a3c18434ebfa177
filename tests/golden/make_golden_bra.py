#!/usr/bin/env python3
"""Generate the brake-net fixtures under tests/golden/ by running the REFERENCE's own Python on CPU
(lav/lav_privileged_v2.py `LAV.train_bra`, lav/utils/datasets/bra_dataset.py).  Like make_golden_seg.py it needs the reference
checkout and runs only where that is; the outputs are committed.

    python tests/golden/make_golden_bra.py            # rewrites bra_train.npz and bra_dataset.npz

bra_train.npz   three Adam steps of the reference's train_bra at batch 2 on 64 x 192 wide and 64 x 96 telephoto images (sides that
                are multiples of 32: the ResNet-18 map is 2 x 6 / 2 x 3 tokens, the seg head's logits 16 x 48 / 16 x 24), seeded
                weights (synth.seeded_state_dict, prefix "bra."), lav_amd.train.synthetic_bra_batch batches (seed 400 + step).
                The reference builds RGBBrakePredictionModel([4, 10, 18], pretrained=True), whose ResNet-18 then fetches ImageNet
                weights (lav/models/resnet.py:262-263, load_state_dict_from_url): it is patched to pretrained=False before the
                LAV is constructed, so nothing is downloaded.  Stores the loss and pred_bra per step, per parameter / buffer
                float64 sums and sums of |.|, the change of every parameter over the three steps - no weights.
bra_dataset.npz the reference BrakePredictionDataset's samples on synthetic routes with 5 cameras and the telephoto camera
                (lav_amd.data.synthetic_route, cameras=5, tel=True), read through the lmdb / cv2 stand-ins of tests/golden/_shims
                and the identity imgaug stand-in (this build has no augmentation).
"""
import os
import sys
import tempfile
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, crc, save  # noqa: E402  (sets up sys.path: shims, reference, repository)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lav_amd import synth  # noqa: E402

BRA_STEPS, BRA_BATCH, BRA_HW, BRA_TEL_HW, BRA_SEED0 = 3, 2, (64, 192), (64, 96), 400
BRA_DATASET_PICKS = (0, 3, 6)


def bra_routes(root):
    """The 'bra' fixture's routes and YAML: two synthetic routes of 8 frames, 5 camera images and a 48 x 64 telephoto image per
    frame, crop_tel_bottom 16."""
    import yaml
    from lav_amd.data import synthetic_route
    synthetic_route.make_dataset(os.path.join(root, "data"), routes=2, frames=8, seed=4, points=200, cameras=5, camera_hw=(40, 32),
                                 tel=True, tel_hw=(48, 64))
    with open(os.path.join(HERE, "dataset_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["data_dir"] = os.path.join(root, "data")
    cfg["num_plan"] = 4
    cfg["crop_tel_bottom"] = 16
    path = os.path.join(root, "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def gold_bra_train():
    sys.path.insert(0, REF)
    import lav.lav_privileged_v2 as ref_priv  # noqa: E402  (reference)
    from lav_amd.train.synthetic import synthetic_bra_batch
    torch.set_grad_enabled(True)
    ref_cls = ref_priv.RGBBrakePredictionModel
    ref_priv.RGBBrakePredictionModel = lambda *a, **k: ref_cls(*a, **dict(k, pretrained=False))     # (no ImageNet download)
    args = types.SimpleNamespace(config_path=os.path.join(REF, "config_v2.yaml"), device="cpu", lr=3e-4)
    trainer = ref_priv.LAV(args)
    bra = trainer.bra_model
    bra.load_state_dict(synth.seeded_state_dict(bra, prefix="bra."))
    before = {k: v.detach().clone().double() for k, v in bra.named_parameters()}
    losses, preds, inputs = [], [], []
    for step in range(BRA_STEPS):
        batch = synthetic_bra_batch(BRA_BATCH, seed=BRA_SEED0 + step, hw=BRA_HW, tel_hw=BRA_TEL_HW, num_classes=4)
        inputs.append(np.bitwise_xor.reduce([crc(t.numpy()) for t in batch]))
        info = trainer.train_bra(*batch)
        losses.append(info["loss"])
        preds.append(info["pred_bra"])
        print("train_bra step", step, info["loss"], info["pred_bra"], flush=True)
    sd = bra.state_dict()
    names = list(sd)
    save("bra_train", losses=np.array(losses), pred_bra=np.array(preds), names=np.array(names), input_crc=np.array(inputs, np.uint64),
         shapes=np.array([",".join(map(str, sd[k].shape)) for k in names]),
         sums=np.array([sd[k].double().sum().item() for k in names]), abs_sums=np.array([sd[k].double().abs().sum().item() for k in names]),
         delta_sums=np.array([(sd[k].double() - before[k]).sum().item() if k in before else 0.0 for k in names]),
         delta_abs_sums=np.array([(sd[k].double() - before[k]).abs().sum().item() if k in before else 0.0 for k in names]),
         pred_sem1=info["pred_sem1"].astype(np.uint8), pred_sem2=info["pred_sem2"].astype(np.uint8))
    torch.set_grad_enabled(False)


def gold_bra_dataset():
    sys.path.insert(0, REF)
    import lav.utils  # noqa: F401
    pkg = types.ModuleType("lav.utils.datasets")          # (skip the package __init__, as make_golden.gold_datasets does)
    pkg.__path__ = [os.path.join(REF, "lav", "utils", "datasets")]
    sys.modules["lav.utils.datasets"] = pkg
    from lav.utils.datasets.bra_dataset import BrakePredictionDataset
    out = {}
    with tempfile.TemporaryDirectory() as root:
        ds = BrakePredictionDataset(bra_routes(root))
        out["len"] = len(ds)
        for i in BRA_DATASET_PICKS:
            key = f"{os.path.basename(ds.dir_map[i])}/{ds.idx_map[i]}"      # (the reference walks routes in glob order)
            rgb, tel_rgb, sem, tel_sem, bra = ds[i]
            for name, a in (("rgb", rgb), ("tel_rgb", tel_rgb), ("sem", sem), ("tel_sem", tel_sem), ("bra", np.int64(bra))):
                out[f"{key}/{name}"] = np.ascontiguousarray(a)
    save("bra_dataset", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["train", "dataset"]
    if "dataset" in which:
        gold_bra_dataset()
    if "train" in which:
        gold_bra_train()
