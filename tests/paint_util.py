"""Helpers shared by the point-painting tests and tests/golden/make_golden_paint.py: the fixture's route and YAML, the random
probability maps, the exclusion rule of the bit-for-bit comparisons."""
from __future__ import annotations

import os

import numpy as np

from tests.util import GOLD

PAINT_SEED = 11
PAINT_POINTS = 4000
PAINT_HW = (288, 256)
MAP_SEED = 23


def paint_fixture_config(root, routes=1, seed=PAINT_SEED, points=PAINT_POINTS, extra_frames=3, **overrides):
    """`routes` synthetic routes of num_plan + extra_frames frames with 5 cameras of 288 x 256 (route i seeded seed + i; route 0 is
    the fixture's make_route(seed, frames=num_plan+3, points=4000, cameras=5, camera_hw=(288, 256))) and the data-loader YAML
    pointed at them.  Returns the YAML's path."""
    import yaml
    from lav_amd.data import synthetic_route
    with open(os.path.join(GOLD, "dataset_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(overrides)
    counts = list(points) if isinstance(points, (list, tuple)) else [points] * routes          # (a list: ragged routes)
    towns = ["Town01", "Town03", "Town02", "Town06"]
    for i in range(routes):                                                                    # (= synthetic_route.make_dataset)
        synthetic_route.make_route(os.path.join(root, "data", f"route_{i:03d}"), seed=seed + i, frames=cfg["num_plan"] + extra_frames,
                                   points=counts[i], town=towns[i % len(towns)], cameras=5, camera_hw=PAINT_HW)
    cfg["data_dir"] = os.path.join(root, "data")
    path = os.path.join(root, "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def random_probability_maps(frames=1, ncam=5, classes=5, hw=PAINT_HW, seed=MAP_SEED) -> np.ndarray:
    """(frames, ncam, classes, H, W) float32, every pixel a Dirichlet-like draw: exponentials normalised (in float64, then rounded)."""
    r = np.random.Generator(np.random.PCG64(seed))
    e = r.exponential(1.0, (frames, ncam, classes) + tuple(hw))
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


def projection_f64(cam, lidar):
    """CameraProjection.pixels' values BEFORE truncation: (n, 3) float64 (u, v, z)."""
    xyz = lidar[:, :3].T
    c = cam.world_to_cam @ (cam.lidar_to_world @ np.r_[xyz, [np.ones(xyz.shape[1])]])
    uvz = cam.K @ np.array([c[1], -c[2], c[0]])
    with np.errstate(all="ignore"):
        return np.array([uvz[0] / (1e-5 + uvz[2]), uvz[1] / (1e-5 + uvz[2]), uvz[2]]).T


def excluded_points(cameras, lidar, hw=PAINT_HW, window=1e-9) -> np.ndarray:
    """(n,) bool: points where, for any camera, any of the float64 u, v, z before truncation lies within `window` of an integer
    while inside [-1, max(h, w) + 1] - only there can a last-bit difference between the host BLAS and the kernel move a pixel."""
    bad = np.zeros(len(lidar), bool)
    top = max(hw) + 1
    for cam in cameras:
        p = projection_f64(cam, lidar)
        with np.errstate(all="ignore"):
            near = (np.abs(p - np.rint(p)) <= window) & (p >= -1) & (p <= top)
        bad |= near.any(axis=1)
    return bad


def clip32(a) -> np.ndarray:
    """int64 pixel records as lav_paint_frames stores them: saturated to int32 (INT64_MIN, numpy's invalid, becomes INT32_MIN)."""
    return np.clip(np.asarray(a, np.int64), np.iinfo(np.int32).min, np.iinfo(np.int32).max).astype(np.int32)


def painter_cameras(cfg):
    from lav_amd.data.datasets import CameraProjection
    return [CameraProjection(y, [0, 0, cfg["camera_z"]], [cfg["camera_x"], 0, cfg["camera_z"]], 288, 256, 64) for y in cfg["camera_yaws"]]
