"""Shared by tests/test_bev_stack_host.py and tests/test_gpu_bev_stack.py: the route fixture, the loaders' default samples (drawn
once per process) and the comparison of a deferred sample with them."""
import os
import re
import subprocess
import sys

import numpy as np
import torch
import yaml

from lav_amd.data import datasets, synthetic_route
from tests.util import GOLD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (loader, sample indices): 2 routes x 30 frames give 10 samples per route - 0 and 1 (and 10: the second route's first) miss history
LOADER_CASES = (("temporal_bev", (0, 1, 7, 10)), ("bev", (0, 5)), ("lidar", (1, 12)), ("lidar_painted", (0, 16)),
                ("temporal_lidar_painted", (0, 1, 13)))
BEV_AT = {"temporal_bev": 0, "bev": 0, "lidar": 5, "lidar_painted": 5, "temporal_lidar_painted": 5}


def make_routes(root, routes=2, frames=30, points=300):
    """Seeded synthetic routes + the loader keys of tests/golden/dataset_config.yaml; returns the YAML's path."""
    synthetic_route.make_dataset(os.path.join(root, "data"), routes=routes, frames=frames, seed=0, points=points)
    with open(os.path.join(GOLD, "dataset_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["data_dir"] = os.path.join(root, "data")
    path = os.path.join(root, "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def draw(ds, idx):
    """Sample idx under its own seeds, and the next draw of both generators after it (the draws a sample consumed)."""
    torch.manual_seed(1000 + idx)
    np.random.seed(1000 + idx)
    sample = ds[idx]
    return sample, (float(torch.rand(1)), float(np.random.random()))


_default = {}


def default_samples(cfg, name, picks):
    """The default (host-rendered) samples: computed once, shared, never modified."""
    if (cfg, name) not in _default:
        ds = datasets.LOADERS[name](cfg)
        assert len(ds) == 20 and not ds.bev_on_device
        _default[(cfg, name)] = {p: draw(ds, p) for p in picks}
    return _default[(cfg, name)]


def assert_same_sample(name, idx, got, want, bev):
    """Every element of the deferred sample `got` but its record equals the default sample's; `bev` (rendered from the record)
    equals the default sample's map."""
    at = BEV_AT[name]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        if k == at:
            bev = np.asarray(bev)
            assert bev.dtype == w.dtype == np.uint8 and bev.shape == w.shape, (name, idx, bev.dtype, bev.shape, w.shape)
            assert np.array_equal(bev, w), f"{name} sample {idx}: {int((bev != w).sum())} BEV pixels differ"
            continue
        g, w = np.asarray(g), np.asarray(w)
        if name in ("lidar", "lidar_painted") and k == 0:       # rows past num_points are np.empty
            g, w = g[:got[1]], w[:want[1]]
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{name} sample {idx} element {k}"


def run_driver(cfg, tmp, *extra, timeout=900, env=None):
    """train_bev_v2.py over the recorded routes of cfg: two steps of batch 2, every step logged; returns the logged lines."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "train_bev_v2.py"), "--config-path", cfg, "--batch-size", "2", "--num-epoch", "1",
                        "--num-workers", "0", "--num-per-log", "1", "--save-dir", os.path.join(tmp, "ck"), *extra],
                       capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert '"steps": 2' in r.stdout, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if re.match(r"\d+ \{", ln)]
    assert len(lines) == 2 and all("loss" in ln for ln in lines), r.stdout
    return lines
