#!/usr/bin/env python3
"""tests/golden/log_view.npz: what the trainers' visual log (lav_amd/train/log_view.py) is pinned against, recorded from the REFERENCE
and from matplotlib.  Recorded results only; tests/test_log_view_host.py compares.

    python tests/golden/make_golden_log.py

palette/*   the reference's own visualize_semantic_processed (lav/utils/visualization.py, imported under the cv2 stand-in of
            tests/golden/_shims) on one seeded label map, for the label lists [4, 6, 7, 10] (config_v2.yaml's seg_channels),
            [4, 10, 18] (the brake net's) and its default; SEM_COLORS as (label, r, g, b) rows.
boxes/*     a dozen seeded detections (x, y, w, h, cos, sin) and matplotlib's corners of the Rectangle that log_lidar_info builds for
            each (lav/utils/logger.py:122, the expression restated here around matplotlib's own transform).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("LAV_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(HERE, "_shims"), REF, REPO]

import numpy as np  # noqa: E402
from matplotlib.patches import Rectangle  # noqa: E402

from lav.utils import visualization as ref_viz  # noqa: E402  (reference)

LABEL_LISTS = dict(seg=[4, 6, 7, 10], bra=[4, 10, 18], default=None)


def corners(rect) -> np.ndarray:
    if hasattr(rect, "get_corners"):
        return np.asarray(rect.get_corners(), np.float64)
    return rect.get_patch_transform().transform(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64))


def main():
    rng = np.random.default_rng(36)
    out = {}
    sem = rng.integers(0, 8, (24, 40)).astype(np.int64)          # labels 0 .. 7: past every list's last class
    out["palette/sem"] = sem
    for name, labels in LABEL_LISTS.items():
        out[f"palette/{name}"] = ref_viz.visualize_semantic_processed(sem) if labels is None else ref_viz.visualize_semantic_processed(sem, labels)
        out[f"palette/{name}_labels"] = np.array(labels if labels is not None else ref_viz.visualize_semantic_processed.__defaults__[0], np.int64)
    out["palette/sem_colors"] = np.array([(k,) + tuple(v) for k, v in sorted(ref_viz.SEM_COLORS.items())], np.int64)
    dets, quads = [], []
    for _ in range(12):
        x, y = int(rng.integers(0, 320)), int(rng.integers(0, 320))
        w, h = float(rng.uniform(0.5, 12)), float(rng.uniform(1, 25))
        a, s = rng.uniform(-np.pi, np.pi), rng.uniform(0.5, 1.5)          # the orientation maps are not normalised
        cos, sin = float(s * np.cos(a)), float(s * np.sin(a))
        rect = Rectangle((x, y) + [w, h] @ np.array([[-sin, cos], [-cos, -sin]]), w * 2, h * 2, angle=np.rad2deg(np.arctan2(sin, cos) - np.pi / 2))
        dets.append((x, y, w, h, cos, sin))
        quads.append(corners(rect))
    out["boxes/det"], out["boxes/corners"] = np.array(dets, np.float64), np.array(quads, np.float64)
    path = os.path.join(HERE, "log_view.npz")
    np.savez_compressed(path, **out)
    print(f"log_view.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
