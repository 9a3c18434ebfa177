"""Seeded builders of small frames for the open-loop evaluation tests (tests/test_eval_host.py, tests/test_gpu_eval.py).

A frame is a dict of eval_frame's positional arguments (NumPy arrays) plus "kw", its keyword arguments.  The default geometry is chosen
to break tilings: 37 x 53 pixels is no multiple of a tile or of 4 (planes 1 and 2 of the predictions then start off a 16-byte boundary
and the last pixels are a tail), T = 20 waypoints, D = 20 rows per class.  The ego pixel is (26, 30) at 4 pixels per metre, so that a
pixel coordinate on a quarter is an exact float32 number of metres."""
from __future__ import annotations

import numpy as np

H, W, T, D = 37, 53, 20, 20
PPM, CENTRE, RADIUS = 4.0, (26.0, 30.0), 8.0
ARGS = ("pred_bev", "bev", "mask", "rows", "locs", "typs", "n", "ego_plan", "ego_locs", "cmd", "other_cast", "other_cmds", "other_row")
Q = 1 << 20


def metres(px, py, centre=CENTRE):
    """float32 ego-frame metres of a pixel (exact for pixels on a quarter)."""
    return np.array([(px - centre[0]) / PPM, (py - centre[1]) / PPM], np.float32)


def track(px, py, step=(0.0, -0.25), centre=CENTRE):
    """(T + 1, 2) float32: an actor at pixel (px, py) moving `step` metres per frame (quarters: every sum is exact)."""
    return (metres(px, py, centre)[None] + np.arange(T + 1, dtype=np.float32)[:, None] * np.asarray(step, np.float32)[None]).astype(np.float32)


def blank(h=H, w=W, G=4, cmd=2, centre=CENTRE):
    """Nothing predicted, nothing labelled, no actors, no rows above any threshold, the plan on its target."""
    rows = np.zeros((2, D, 7), np.float32)
    rows[..., 0] = -1e5                                   # what lav_extract_peaks leaves in unused rows
    ego = track(centre[0], centre[1])
    return dict(pred_bev=np.zeros((3, h, w), np.float32), bev=np.zeros((4, h, w), np.uint8), mask=np.ones((h, w), np.uint8), rows=rows,
                locs=np.zeros((G, T + 1, 2), np.float32), typs=np.zeros(G, np.int32), n=0, ego_plan=ego[1:].copy(), ego_locs=ego, cmd=cmd,
                other_cast=None, other_cmds=None, other_row=None, kw=dict(ppm=PPM, centre=centre, radius_px=RADIUS))


def put_row(f, c, r, score, x, y):
    f["rows"][c, r] = (score, x, y, 2.0, 4.0, 1.0, 0.0)


def put_actor(f, g, typ, px, py, step=(0.0, -0.25)):
    f["locs"][g] = track(px, py, step, f["kw"]["centre"])
    f["typs"][g] = typ
    f["n"] = max(f["n"], g + 1)


def forecasts(f, rows_of, casts, cmds=None):
    f["other_row"] = np.asarray(rows_of, np.int32)
    f["other_cast"] = np.asarray(casts, np.float32).reshape(len(rows_of), 6, T, 2)
    f["other_cmds"] = np.asarray(cmds if cmds is not None else np.tile(np.arange(6, 0, -1, dtype=np.float32) / 8, (len(rows_of), 1)), np.float32)


def scene_empty():
    f = blank()
    f["rows"][:, :3, 0] = (0.1 - 1e-3, 0.05, 0.0)         # nothing above min_score
    f["rows"][:, :3, 1:3] = 10.0
    f["locs"][:] = track(20, 10)                          # actors in the table, but n = 0
    f["typs"][:] = 1
    return f


def scene_compete():
    """Class 1: rows 0 and 1 both within the radius of actor 0, actor 1 farther away; row 2 on actor 1."""
    f = blank()
    put_actor(f, 0, 1, 20, 10)
    put_actor(f, 1, 1, 40, 10)
    put_row(f, 1, 0, 0.9, 22, 10)
    put_row(f, 1, 1, 0.8, 21, 10)
    put_row(f, 1, 2, 0.7, 40, 12)
    return f


def scene_tie():
    """Class 1: actors 1 and 3 at equal distance from row 0; actors 0 and 2 are pedestrians elsewhere.  The forecast of row 0 is actor
    1's future moved by exactly 1 m in x in every mode: which actor the row took shows in the forecast error."""
    f = blank()
    put_actor(f, 0, 0, 45, 30)
    put_actor(f, 1, 1, 20, 10)
    put_actor(f, 2, 0, 50, 5)
    put_actor(f, 3, 1, 24, 10, step=(0.5, 0.25))
    put_row(f, 1, 0, 0.5, 22, 10)
    forecasts(f, [0], np.tile(f["locs"][1, 1:] + np.array([1.0, 0.0], np.float32), (6, 1, 1)))
    return f


def scene_outside():
    """Class 1 centres at x = -0.5, W - 0.25, exactly 0 and exactly W, and at y = -0.25, H - 0.25 and exactly H."""
    f = blank(G=8)
    for g, (px, py) in enumerate([(-0.5, 10), (W - 0.25, 10), (0, 10), (W, 10), (10, -0.25), (10, H - 0.25), (10, H)]):
        put_actor(f, g, 1, px, py)
    put_row(f, 1, 0, 0.9, 0, 10)
    put_row(f, 1, 1, 0.6, 52, 10)
    put_row(f, 1, 2, 0.5, 45, 10)                         # 8 px from the actor at x = W: a true positive if that one counted
    return f


def scene_edges():
    """Scores exactly 1.0, min_score, det_score and NaN (thresholds 0.125 and 0.25, exact in float32); pred_bev exactly at the threshold
    on channel 0; the mask zero on all of channel 2's support; a plan half a metre off."""
    f = blank(cmd=5)
    f["kw"].update(min_score=0.125, det_score=0.25)
    for g, (px, py) in enumerate([(10, 10), (40, 20), (5, 30)]):
        put_actor(f, g, 0, px, py)
    put_row(f, 0, 0, 1.0, 10, 10)
    put_row(f, 0, 1, 0.5, 30, 30)
    put_row(f, 0, 2, 0.25, 40, 20)
    put_row(f, 0, 3, 0.125, 5, 30)
    put_row(f, 0, 4, np.nan, 5, 30)
    f["mask"][:, 30:] = 0
    f["pred_bev"][0] = 0.5
    f["bev"][0, :3, :4] = 1
    f["pred_bev"][1] = 0.75
    f["bev"][1, :10] = 1
    f["pred_bev"][2] = 0.25
    f["pred_bev"][2, :, 30:] = 0.75
    f["bev"][2, :, 30:] = 1
    f["ego_plan"] = (f["ego_locs"][1:] + np.array([0.0, 0.5], np.float32)).astype(np.float32)
    return f


def random_frame(seed, h=H, w=W, G=10, n=None, N=0, used=12, centre=CENTRE, lowest=0.05):
    """A seeded frame with everything in it: random maps, actors in and around the map, rows near some of them in descending score,
    N forecasts of class-1 rows (true and false positives), a noisy plan."""
    rng = np.random.default_rng(seed)
    f = blank(h, w, G, cmd=int(rng.integers(0, 6)), centre=centre)
    f["pred_bev"] = rng.random((3, h, w)).astype(np.float32)
    f["bev"] = (rng.random((4, h, w)) < 0.4).astype(np.uint8)
    f["mask"] = (rng.random((h, w)) < 0.8).astype(np.uint8)
    n = G if n is None else n
    for g in range(G):
        put_actor(f, g, int(rng.integers(0, 3)) % 2 if g % 5 else 2, rng.uniform(-4, w + 4), rng.uniform(-4, h + 4),
                  step=(rng.uniform(-0.5, 0.5), rng.uniform(-1, 0)))
    f["n"] = n
    for c in range(2):
        scores = np.sort(rng.uniform(lowest, 1.0, used).astype(np.float32))[::-1]
        own = [g for g in range(n) if f["typs"][g] == c]
        for r in range(used):
            if own and rng.random() < 0.7:
                g = own[int(rng.integers(0, len(own)))]
                px, py = f["locs"][g, 0] * PPM + np.asarray(centre)
                x, y = np.round(px + rng.uniform(-6, 6)), np.round(py + rng.uniform(-6, 6))
            else:
                x, y = rng.integers(0, w), rng.integers(0, h)
            put_row(f, c, r, scores[r], x, y)
    if N:
        rows_of = np.sort(rng.choice(used, N, replace=False))
        casts = np.zeros((N, 6, T, 2), np.float32)
        for k in range(N):
            g = int(rng.integers(0, G))
            casts[k] = f["locs"][g, 1:][None] + rng.normal(0, 0.5, (6, T, 2)).astype(np.float32)
        cmds = rng.random((N, 6)).astype(np.float32)
        cmds[0, 1] = cmds[0, 4] = 2.0                    # a duplicate maximum: the first one is the top mode
        forecasts(f, rows_of, casts, cmds)
    f["ego_plan"] = (f["ego_locs"][1:] + rng.normal(0, 0.3, (T, 2))).astype(np.float32)
    return f


def scene_nonfinite():
    """A NaN in the plan, an Inf in one mode of the second of three forecasts (each of a true positive: only those are looked at)."""
    rng = np.random.default_rng(5)
    f = blank()
    f["pred_bev"] = rng.random((3, H, W)).astype(np.float32)
    f["bev"] = (rng.random((4, H, W)) < 0.4).astype(np.uint8)
    for k in range(3):
        put_actor(f, k, 1, 8 + 15 * k, 12)
        put_row(f, 1, k, 0.9 - 0.1 * k, 8 + 15 * k, 12)
    forecasts(f, [0, 1, 2], [f["locs"][k, 1:][None] + rng.normal(0, 0.5, (6, T, 2)) for k in range(3)])
    f["other_cast"][1, 3, 7, 0] = np.inf
    f["ego_plan"][4, 1] = np.nan
    return f


def scene_others(N):
    return random_frame(20 + N, N=N)


def scene_full():
    """As many actors as the kernel takes, and all 20 rows used in both classes."""
    return random_frame(9, G=64, N=7, used=D, lowest=0.15)


SCENES = dict(empty=scene_empty, compete=scene_compete, tie=scene_tie, outside=scene_outside, edges=scene_edges, nonfinite=scene_nonfinite,
              others0=lambda: scene_others(0), others1=lambda: scene_others(1), others7=lambda: scene_others(7), full=scene_full)


def perfect(shift=0.0, seed=3):
    """Predictions that are the ground truth: pred_bev = the labels, a row of score 0.9 on every actor's (integer) pixel, the plan on its
    target and every forecast mode on its actor's future - all moved by `shift` metres in x."""
    rng = np.random.default_rng(seed)
    f = blank(G=8, cmd=1)
    f["bev"] = (rng.random((4, H, W)) < 0.4).astype(np.uint8)
    f["pred_bev"] = f["bev"][:3].astype(np.float32)
    spots = [(5, 5), (15, 9), (25, 13), (35, 17), (45, 21), (10, 25), (20, 29), (30, 33)]
    counts = [0, 0]
    for g, (px, py) in enumerate(spots):
        c = g % 2
        put_actor(f, g, c, px, py, step=(0.25, -0.5))
        put_row(f, c, counts[c], 0.9, px, py)
        counts[c] += 1
    move = np.array([shift, 0.0], np.float32)
    ones = [g for g in range(8) if g % 2 == 1]
    forecasts(f, list(range(len(ones))), [np.tile(f["locs"][g, 1:] + move, (6, 1, 1)) for g in ones])
    f["ego_plan"] = (f["ego_locs"][1:] + move).astype(np.float32)
    return f


def positional(f):
    return [f[k] for k in ARGS]
