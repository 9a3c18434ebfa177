"""Seeded builders of small frames for the box-metric tests (tests/test_eval_det_host.py, tests/test_gpu_eval_det.py).

A frame is a dict of eval_det's positional arguments (NumPy arrays) plus "kw", its keyword arguments.  The map is 41 x 53 pixels (no
multiple of anything), the ego pixel (26, 30) at 4 pixels per metre, so that a pixel coordinate on a quarter is an exact float32 number
of metres and the ground-truth pixel is exact.  An actor's box is written into the size / orientation maps at the one pixel the
evaluator reads, min(W - 1, int(px + 0.5)): later actors overwrite earlier ones there, as the loader's strongest Gaussian would."""
from __future__ import annotations

import numpy as np

H, W, T = 41, 53, 2
PPM, CENTRE, RADIUS = 4.0, (26.0, 30.0), 8.0
ARGS = ("rows", "locs", "typs", "n", "size_map", "ori_map")
Q = 1 << 20
DYADIC = (0.25, 0.5, 0.75)


def blank(D=15, G=20, h=H, w=W, **kw):
    """No actors, no rows above any threshold, empty maps."""
    rows = np.zeros((2, D, 7), np.float32)
    rows[..., 0] = -1e5                                   # what lav_extract_peaks leaves in unused rows
    return dict(rows=rows, locs=np.zeros((G, T + 1, 2), np.float32), typs=np.zeros(G, np.int32), n=0, size_map=np.zeros((2, h, w), np.float32),
                ori_map=np.zeros((2, h, w), np.float32), kw=dict(ppm=PPM, centre=CENTRE, radius_px=RADIUS, **kw))


def put_actor(f, g, typ, px, py, w=2.0, h=4.0, c=1.0, s=0.0):
    """Actor g of class typ at pixel (px, py) (on a quarter) with half extents (w, h) pixels and direction (c, s)."""
    cx, cy = f["kw"]["centre"]
    f["locs"][g] = np.array([(px - cx) / PPM, (py - cy) / PPM], np.float32)[None]
    f["typs"][g] = typ
    f["n"] = max(f["n"], g + 1)
    Hm, Wm = f["size_map"].shape[1:]
    if 0 <= px < Wm and 0 <= py < Hm:
        ix, iy = min(Wm - 1, int(px + 0.5)), min(Hm - 1, int(py + 0.5))
        f["size_map"][:, iy, ix] = (w, h)
        f["ori_map"][:, iy, ix] = (c, s)


def put_row(f, c, r, score, x, y, w=2.0, h=4.0, cos=1.0, sin=0.0):
    f["rows"][c, r] = (score, x, y, w, h, cos, sin)


def pair_scene(pred, gt, cls=1, score=0.9, **kw):
    """One row (x, y, w, h, cos, sin) and one actor (px, py, w, h, c, s) of class `cls`."""
    f = blank(D=1, G=1, **kw)
    put_actor(f, 0, cls, *gt)
    put_row(f, cls, 0, score, *pred)
    return f


S2 = float(np.sqrt(2.0))
# name -> (prediction, ground truth, IoU or None where only the kernel == specification matters)
HAND = dict(identical=((20.0, 12.0, 3.0, 5.0, 0.6, 0.8), (20.0, 12.0, 3.0, 5.0, 0.6, 0.8), 1.0),
            edge_sharing=((24.0, 12.0, 3.0, 2.0, 1.0, 0.0), (20.0, 12.0, 3.0, 2.0, 1.0, 0.0), 0.0),       # (with direction (1, 0), h is the extent along x)
            half=((20.0, 12.0, 1.0, 0.5, 1.0, 0.0), (20.0, 12.0, 1.0, 1.0, 1.0, 0.0), 0.5),
            octagon=((20.0, 12.0, 0.5, 0.5, 1.0, 1.0), (20.0, 12.0, 0.5, 0.5, 1.0, 0.0), 2.0 * (S2 - 1.0) / (2.0 - 2.0 * (S2 - 1.0))),
            disjoint=((27.0, 12.0, 2.0, 3.0, 0.0, 1.0), (20.0, 12.0, 2.0, 3.0, 1.0, 0.0), 0.0),
            flipped=((20.0, 12.0, 2.0, 4.0, -1.0, 0.0), (20.0, 12.0, 2.0, 4.0, 1.0, 0.0), 1.0),
            turned=((21.0, 13.0, 2.0, 4.5, 0.0, -2.0), (20.0, 12.0, 2.5, 4.0, 3.0, 0.25), None))


def random_scene(seed, D=15, G=20, n=None, used=None, heavy=False, nbins=256, bad=False, **kw):
    """A seeded frame: actors of both classes in and around the map with random boxes, rows near some of them in descending score with
    boxes near theirs.  heavy: every actor and row inside a 12 x 12 pixel area (boxes overlap many others).  bad: some invalid boxes
    on both sides (w = 0, negative h, cos = sin = 0, NaN, Inf), NaN scores and rows below min_score in between."""
    rng = np.random.default_rng(seed)
    f = blank(D, G, nbins=nbins, **kw)
    n = G if n is None else n
    used = min(D, 12) if used is None else used
    quarter = lambda v: float(np.round(v * 4) / 4)
    for g in range(n):
        if heavy:
            px, py = quarter(rng.uniform(20, 32)), quarter(rng.uniform(10, 22))
        else:
            px, py = quarter(rng.uniform(-3, W + 3)), quarter(rng.uniform(-3, H + 3))
        a = rng.uniform(-np.pi, np.pi)
        scale = rng.choice([1.0, 1.0, 0.5, 3.0])          # the maps' directions need not be unit vectors
        put_actor(f, g, int(rng.integers(0, 3)) % 2 if g % 7 else 2, px, py, np.float32(rng.uniform(0.5, 4)), np.float32(rng.uniform(1, 8)),
                  np.float32(np.cos(a) * scale), np.float32(np.sin(a) * scale))
    for c in range(2):
        scores = np.sort(rng.uniform(0.05, 1.0, used).astype(np.float32))[::-1]
        own = [g for g in range(n) if f["typs"][g] == c]
        for r in range(used):
            a = rng.uniform(-np.pi, np.pi)
            w, h = rng.uniform(0.5, 4), rng.uniform(1, 8)
            if own and rng.random() < 0.75:
                g = own[int(rng.integers(0, len(own)))]
                px, py = f["locs"][g, 0].astype(np.float64) * PPM + np.asarray(CENTRE)
                x, y = np.round(px + rng.uniform(-3, 3)), np.round(py + rng.uniform(-3, 3))
                if 0 <= px < W and 0 <= py < H and rng.random() < 0.8:          # a box near the actor's own
                    ix, iy = min(W - 1, int(px + 0.5)), min(H - 1, int(py + 0.5))
                    w, h = f["size_map"][:, iy, ix] * rng.uniform(0.8, 1.25, 2)
                    gc, gs = f["ori_map"][:, iy, ix]
                    a = np.arctan2(gs, gc) + rng.normal(0, 0.3) + (np.pi if rng.random() < 0.2 else 0.0)
            elif heavy:
                x, y = rng.integers(20, 33), rng.integers(10, 23)
            else:
                x, y = rng.integers(0, W), rng.integers(0, H)
            put_row(f, c, r, scores[r], x, y, w, h, np.cos(a), np.sin(a))
    if bad:
        broken = [(0.0, 3.0, 1.0, 0.0), (2.0, -1.0, 1.0, 0.0), (2.0, 3.0, 0.0, 0.0), (np.nan, 3.0, 1.0, 0.0), (2.0, np.inf, 1.0, 0.0),
                  (2.0, 3.0, np.nan, 0.5), (2.0, 3.0, np.inf, 0.0)]
        for c in range(2):
            for k, r in enumerate(rng.choice(used, min(used, 4), replace=False)):
                f["rows"][c, r, 3:7] = broken[(k + 3 * c) % len(broken)]
            if used >= 3:
                f["rows"][c, 1, 0] = np.nan
                f["rows"][c, 2, 0] = 0.05
        inside = [g for g in range(n) if f["typs"][g] in (0, 1) and 0 <= f["locs"][g, 0, 0] * PPM + CENTRE[0] < W and 0 <= f["locs"][g, 0, 1] * PPM + CENTRE[1] < H]
        for k, g in enumerate(inside[::3]):
            px, py = f["locs"][g, 0].astype(np.float64) * PPM + np.asarray(CENTRE)
            ix, iy = min(W - 1, int(px + 0.5)), min(H - 1, int(py + 0.5))
            f["size_map"][:, iy, ix] = broken[k % len(broken)][:2]
            f["ori_map"][:, iy, ix] = broken[k % len(broken)][2:]
    return f


def positional(f):
    return [f[k] for k in ARGS]
