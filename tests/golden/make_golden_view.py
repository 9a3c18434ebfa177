#!/usr/bin/env python3
"""tests/golden/debug_view.npz: the LiDAR panel of the agent's debug view, computed by the REFERENCE's own lidar_to_bev
(team_code_v2/lav_agent_fast.py:567-581, imported under the stand-ins of tests/golden/_shims as make_golden.py imports it) on two
small hand-made clouds.  Inputs and output only; tests/test_debug_view_host.py compares lav_amd.agent.debug_view.lidar_panel.

    python tests/golden/make_golden_view.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("LAV_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(HERE, "_shims"), os.path.join(REF, "team_code_v2"), REPO]

import numpy as np  # noqa: E402

import lav_agent_fast as ref_agent  # noqa: E402  (reference)

# (min_x, max_x, min_y, max_y, pixels_per_meter): 64 x 64 bins with edges that float32 holds exactly (step 17 / 64), and 60 x 50
# bins whose edges it does not (steps 13 / 60 and 11 / 50)
GRIDS = dict(a=(-4, 12, -8, 8, 4), b=(-2, 10, -5, 5, 5))


def cloud(grid, seed):
    min_x, max_x, min_y, max_y, ppm = grid
    nx, ny = (max_x - min_x) * ppm, (max_y - min_y) * ppm
    ex, ey = np.linspace(min_x, max_x + 1, nx + 1), np.linspace(min_y, max_y + 1, ny + 1)
    rng = np.random.default_rng(seed)
    f32 = np.float32
    rows = [rng.uniform((min_x - 2, min_y - 2), (max_x + 3, max_y + 3), (1500, 2))]          # inside and outside the grid
    # on every interior edge (as float32 holds it), and one float32 step to either side
    on_x = np.stack([ex.astype(f32), rng.uniform(min_y, max_y, nx + 1).astype(f32)], 1)
    on_y = np.stack([rng.uniform(min_x, max_x, ny + 1).astype(f32), ey.astype(f32)], 1)
    rows += [on_x, on_y]
    for d in (-np.inf, np.inf):
        rows += [np.stack([np.nextafter(on_x[:, 0], f32(d)), on_x[:, 1]], 1), np.stack([on_y[:, 0], np.nextafter(on_y[:, 1], f32(d))], 1)]
    # the corners: first edges (inside), last edges (inclusive), and just outside
    rows.append([[ex[0], ey[0]], [ex[-1], ey[-1]], [ex[-1], ey[0]], [ex[0], ey[-1]], [ex[3], ey[-1]], [ex[-1], ey[5]],
                 [np.nextafter(f32(ex[-1]), f32(np.inf)), ey[2]], [ex[2], np.nextafter(f32(ey[-1]), f32(np.inf))],
                 [np.nextafter(f32(ex[0]), f32(-np.inf)), ey[2]], [ex[2], np.nextafter(f32(ey[0]), f32(-np.inf))]])
    # cells holding exactly 9, 10, 11 and 300 points: below, at and past the clamp (nothing else falls into them)
    xy = np.concatenate([np.asarray(r, np.float64) for r in rows]).astype(f32).astype(np.float64)
    rows = []
    for k, n in enumerate((9, 10, 11, 300)):
        cx, cy = 7 + 5 * k, 11 + 3 * k
        xy = xy[~((xy[:, 0] >= ex[cx]) & (xy[:, 0] < ex[cx + 1]) & (xy[:, 1] >= ey[cy]) & (xy[:, 1] < ey[cy + 1]))]
        sx, sy = 0.01 * (ex[1] - ex[0]), 0.01 * (ey[1] - ey[0])
        rows.append(np.stack([rng.uniform(ex[cx] + sx, ex[cx + 1] - sx, n), rng.uniform(ey[cy] + sy, ey[cy + 1] - sy, n)], 1))
    rows.insert(0, xy)
    # rows the graphed pipeline marks absent, and infinities
    rows.append([[np.nan, 0.0], [0.0, np.nan], [np.nan, np.nan], [np.inf, 0.0], [0.0, -np.inf]])
    xy = np.concatenate([np.asarray(r, np.float64) for r in rows]).astype(f32)
    pts = np.concatenate([xy, rng.normal(size=(len(xy), 2)).astype(f32)], 1)                # x, y, z, intensity
    return pts[rng.permutation(len(pts))]


def main():
    out = {}
    for name, grid in GRIDS.items():
        pts = cloud(grid, seed=len(name) + ord(name))
        assert len(pts) <= 4096
        min_x, max_x, min_y, max_y, ppm = grid
        # what visualize() does with it (:460-465)
        panel = ref_agent.lidar_to_bev(pts, min_x=min_x, max_x=max_x, min_y=min_y, max_y=max_y, pixels_per_meter=ppm).astype(np.uint8)
        out[f"{name}/grid"], out[f"{name}/points"], out[f"{name}/panel"] = np.array(grid, np.int64), pts, panel
        print(name, grid, pts.shape, panel.shape, "grey levels", np.unique(panel).tolist())
    path = os.path.join(HERE, "debug_view.npz")
    np.savez_compressed(path, **out)
    print(f"debug_view.npz  {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
