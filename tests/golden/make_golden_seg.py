#!/usr/bin/env python3
"""Generate the camera-segmenter fixtures under tests/golden/ by running the REFERENCE's own Python on CPU
(lav/lav_privileged_v2.py `LAV.train_seg`, lav/utils/datasets/seg_dataset.py).  Like make_golden.py (whose helpers it
imports) it needs the reference checkout and runs only where that is; the outputs are committed.

    python tests/golden/make_golden_seg.py            # rewrites seg_train.npz and seg_dataset.npz

seg_train.npz   three Adam steps of the reference's train_seg at batch 2 on 48 x 256 images (every ERFNet stage then has a
                width of 128 / 64 / 32, the widths the training kernels take), seeded weights (synth.seeded_state_dict, prefix
                "seg."), lav_amd.train.synthetic_seg_batch batches (seed 300 + step).  DROPOUT IS OFF: every nn.Dropout2d of
                the reference model is patched to p = 0, so that the run is deterministic and comparable; the fixture's
                `dropout_p` records it.  Stores the loss per step, per parameter / buffer float64 sums and sums of |.|, and
                the change of every parameter over the three steps (summed) - no weights.
seg_dataset.npz the reference SegmentationDataset's samples on synthetic routes with camera images
                (lav_amd.data.synthetic_route, cameras=5), read through the lmdb / cv2 stand-ins of tests/golden/_shims and
                an identity imgaug stand-in (this build has no augmentation).
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

SEG_STEPS, SEG_BATCH, SEG_HW, SEG_SEED0 = 3, 2, (48, 256), 300
SEG_DATASET_PICKS = (0, 4, 7, 13, 24, 52)      # (frame, camera) = divmod(index, 5)


def seg_routes(root):
    """The 'seg' fixture's routes and YAML: two synthetic routes of 14 frames with 5 camera images per frame."""
    import yaml
    from lav_amd.data import synthetic_route
    synthetic_route.make_dataset(os.path.join(root, "data"), routes=2, frames=14, seed=3, points=200, cameras=5)
    with open(os.path.join(HERE, "dataset_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["data_dir"] = os.path.join(root, "data")
    cfg["num_plan"] = 4
    path = os.path.join(root, "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def gold_seg_train():
    sys.path.insert(0, REF)
    import lav.lav_privileged_v2 as ref_priv  # noqa: E402  (reference)
    from lav_amd.train.synthetic import synthetic_seg_batch
    torch.set_grad_enabled(True)
    ref_priv.RGBBrakePredictionModel = lambda *a, **k: torch.nn.Linear(1, 1)    # (ImageNet download; not part of train_seg)
    args = types.SimpleNamespace(config_path=os.path.join(REF, "config_v2.yaml"), device="cpu", lr=3e-4)
    trainer = ref_priv.LAV(args)
    seg = trainer.seg_model
    seg.load_state_dict(synth.seeded_state_dict(seg, prefix="seg."))
    for m in seg.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    before = {k: v.detach().clone().double() for k, v in seg.named_parameters()}
    losses, inputs = [], []
    for step in range(SEG_STEPS):
        rgb, sem = synthetic_seg_batch(SEG_BATCH, seed=SEG_SEED0 + step, hw=SEG_HW, num_classes=len(trainer.seg_channels) + 1)
        inputs.append(crc(rgb.numpy()) ^ crc(sem.numpy()))
        info = trainer.train_seg(rgb, sem)
        losses.append(info["loss"])
        print("train_seg step", step, info["loss"], flush=True)
    sd = seg.state_dict()
    names = list(sd)
    save("seg_train", losses=np.array(losses), names=np.array(names), dropout_p=np.float64(0.0), input_crc=np.array(inputs, np.uint64),
         sums=np.array([sd[k].double().sum().item() for k in names]), abs_sums=np.array([sd[k].double().abs().sum().item() for k in names]),
         delta_sums=np.array([(sd[k].double() - before[k]).sum().item() if k in before else 0.0 for k in names]),
         delta_abs_sums=np.array([(sd[k].double() - before[k]).abs().sum().item() if k in before else 0.0 for k in names]),
         pred_sem=info["pred_sem"].astype(np.uint8), seg_channels=np.array(trainer.seg_channels))
    torch.set_grad_enabled(False)


def gold_seg_dataset():
    sys.path.insert(0, REF)
    import lav.utils  # noqa: F401
    pkg = types.ModuleType("lav.utils.datasets")          # (skip the package __init__, as make_golden.gold_datasets does)
    pkg.__path__ = [os.path.join(REF, "lav", "utils", "datasets")]
    sys.modules["lav.utils.datasets"] = pkg
    from lav.utils.datasets.seg_dataset import SegmentationDataset
    out = {}
    with tempfile.TemporaryDirectory() as root:
        ds = SegmentationDataset(seg_routes(root))
        out["len"] = len(ds)
        for i in SEG_DATASET_PICKS:
            frame, cam = divmod(i, len(ds.camera_yaws))
            key = f"{os.path.basename(ds.dir_map[frame])}/{ds.idx_map[frame]}/{cam}"     # (the reference walks routes in glob order)
            rgb, sem = ds[i]
            out[f"{key}/rgb"], out[f"{key}/sem"] = np.ascontiguousarray(rgb), sem
    save("seg_dataset", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["train", "dataset"]
    if "dataset" in which:
        gold_seg_dataset()
    if "train" in which:
        gold_seg_train()
