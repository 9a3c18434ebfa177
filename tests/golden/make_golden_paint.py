#!/usr/bin/env python3
"""Generate tests/golden/data_paint.npz by running the REFERENCE's own Python on CPU (lav/data_paint.py's PointPainter.step,
lav/utils/datasets/point_paint_dataset.py, lav/utils/point_painting.py, lav/models/rgb.py).  Like make_golden.py (whose helpers
it imports) it needs the reference checkout and runs only where that is; the output is committed.

    python tests/golden/make_golden_paint.py            # rewrites data_paint.npz

One seeded synthetic route (tests/paint_util.paint_fixture_config: make_route(11, frames=num_plan+3, points=4000, cameras=5,
camera_hw=(288, 256))), read through the lmdb / cv2 stand-ins of tests/golden/_shims.  data_paint.py itself imports ray, wandb,
tqdm and matplotlib at module level (a `ray` stand-in would have to restate @ray.remote's actor protocol), so PointPainter.step's
four statements (data_paint.py:69-77) are composed here from the modules it imports - its dataset, its model class, its
CoordConverter and point_painting.  Records:
  len, route/frame of every index entry                          the reference PointPaintDataset's index
  f{i}/lidar_crc, lidar_s, rgbs_crc, rgbs_s, rgbs_shape          its samples (checksums and strided samples), i = 0, 1, 2
  f{i}/lidar_painted (n, 4) float32, f{i}/lidar_to_cam           PointPainter.step's result with the seeded segmenter
       (5, n, 3) int32 (int64 saturated; INT32_MIN = numpy's       (synth.seeded_state_dict, prefix "seg.") and every camera's
       INT64_MIN)                                                  CoordConverter.lidar_to_cam
  logit_absmax                                                   max |logit| of the segmenter over these 15 images
  map/lidar_painted, map/seed                                    point_painting of frame 0's sweep on tests/paint_util's random
                                                                 probability maps, normalised as data_paint.py:75
"""
import os
import sys
import tempfile
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, crc, save  # noqa: E402  (sets up sys.path: shims, reference, repository)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from lav_amd import synth  # noqa: E402
from tests import paint_util  # noqa: E402

FRAMES = 3


def gold_data_paint():
    sys.path.insert(0, REF)
    import lav.utils  # noqa: F401
    pkg = types.ModuleType("lav.utils.datasets")          # (skip the package __init__, as make_golden.gold_datasets does)
    pkg.__path__ = [os.path.join(REF, "lav", "utils", "datasets")]
    sys.modules["lav.utils.datasets"] = pkg
    from lav.models.rgb import RGBSegmentationModel
    from lav.utils import _numpy
    from lav.utils.datasets.point_paint_dataset import PointPaintDataset
    from lav.utils.point_painting import CoordConverter, point_painting
    out = {}
    with tempfile.TemporaryDirectory() as root:
        config_path = paint_util.paint_fixture_config(root)
        with open(config_path) as f:
            cfg = yaml.safe_load(f)
        dataset = PointPaintDataset(config_path)
        assert len(dataset) == FRAMES
        out["len"] = len(dataset)
        out["index"] = np.array([f"{os.path.basename(dataset.nam_map[i])}/{dataset.idx_map[i]}" for i in range(len(dataset))])
        seg_model = RGBSegmentationModel(cfg["seg_channels"])
        seg_model.load_state_dict(synth.seeded_state_dict(seg_model, prefix="seg."))
        seg_model.eval()
        converters = [CoordConverter(cam_yaw, lidar_xyz=[0, 0, cfg["camera_z"]], cam_xyz=[cfg["camera_x"], 0, cfg["camera_z"]],
                                     rgb_h=288, rgb_w=256, fov=64) for cam_yaw in cfg["camera_yaws"]]
        absmax = 0.0
        for idx in range(FRAMES):
            lidar, rgbs = dataset[idx]
            out[f"f{idx}/lidar_crc"], out[f"f{idx}/lidar_s"] = np.uint64(crc(lidar)), lidar[::16].copy()
            out[f"f{idx}/rgbs_crc"], out[f"f{idx}/rgbs_s"] = np.uint64(crc(rgbs)), rgbs[:, :, ::16, ::16].copy()
            out[f"f{idx}/rgbs_shape"] = np.array(rgbs.shape)
            # data_paint.py:71-77
            rgbs = torch.tensor(rgbs.copy()).float()
            logits = seg_model(rgbs)
            absmax = max(absmax, float(logits.abs().max()))
            sems = _numpy(torch.softmax(logits, dim=1))
            norm_sems = sems[:, 1:] * (1 - sems[:, :1])
            lidar_painted = point_painting(lidar, norm_sems, converters)
            out[f"f{idx}/lidar_painted"] = np.ascontiguousarray(lidar_painted).astype(np.float32)     # (commit's cast)
            out[f"f{idx}/lidar_to_cam"] = paint_util.clip32(np.stack([c.lidar_to_cam(lidar) for c in converters]))
            print("frame", idx, "painted rows", int((lidar_painted != 0).any(1).sum()), "of", len(lidar), flush=True)
        out["logit_absmax"] = np.float64(absmax)
        lidar, _ = dataset[0]
        sems = paint_util.random_probability_maps()[0]
        out["map/seed"], out["map/crc"] = paint_util.MAP_SEED, np.uint64(crc(sems))
        out["map/lidar_painted"] = point_painting(lidar, sems[:, 1:] * (1 - sems[:, :1]), converters).astype(np.float32)
    save("data_paint", **out)


if __name__ == "__main__":
    gold_data_paint()
