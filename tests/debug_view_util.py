"""Shared by tests/test_debug_view_host.py and tests/test_gpu_debug_view.py: the small geometries, their clouds and the scenes
drawn on the LiDAR panel."""
import numpy as np

AGENT_GRID = (-10, 70, -40, 40, 4)
CMD_THRESH = 0.2

# name -> (grid, camera image shape, telephoto image shape, ego pixel).  lav_debug_view renders 32 x 16 tiles of the frame; every
# frame here spans at least two tiles in each direction with a partial last tile in both (24 or 25 rows: 16 + 8 / 9; 164 or 170
# columns: five tiles + 4 / 10), so none had to be enlarged.
#   even:  canvas 48 x (120 + 112 + 48 + 48) = 48 x 328, frame 24 x 164: both scales of the second resize are exactly 2
#   odd:   canvas 50 x (125 + 116 + 50 + 50) = 50 x 341, frame 25 x 170: the vertical scale is exactly 2, the horizontal 341 / 170
#          (the same images on a 50-row canvas make camera panels of 125 and 116 columns, not the 48-row canvas's 120 and 112)
#   wide:  canvas 48 x (121 + 112 + 48 + 48) = 48 x 329, frame 24 x 164: an odd-width canvas
GEOMETRIES = {
    "even": ((-2, 10, -6, 6, 4), (40, 100, 3), (30, 70, 3), (24, 40)),
    "odd": ((-2, 8, -5, 5, 5), (40, 100, 3), (30, 70, 3), (25, 40)),
    "wide": ((-2, 10, -6, 6, 4), (40, 101, 3), (30, 70, 3), (24, 40)),
}
FRAMES = {"even": (24, 164, 328), "odd": (25, 170, 341), "wide": (24, 164, 329)}      # frame rows, frame columns, canvas columns
SCENES = ("empty", "full", "pile", "straddle", "overlap")


def images(rgb_shape, tel_shape, seed=0):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, rgb_shape, dtype=np.uint8)
    tel = rng.integers(0, 256, tel_shape, dtype=np.uint8)
    rgb[:, :3], rgb[:, -3:], tel[:2], tel[-2:] = 255, 0, 7, 250          # distinct borders: the edge clamping shows
    return rgb, tel


def cloud(grid, n=3000, seed=1, columns=11):
    """A cloud with rows inside and outside the grid, on every edge as float32 holds it, cells below, at and past the clamp, NaN
    rows (the graphed pipeline's absent points) and infinities."""
    min_x, max_x, min_y, max_y, ppm = grid
    nx, ny = (max_x - min_x) * ppm, (max_y - min_y) * ppm
    ex, ey = np.linspace(min_x, max_x + 1, nx + 1), np.linspace(min_y, max_y + 1, ny + 1)
    rng = np.random.default_rng(seed)
    f32 = np.float32
    rows = [rng.uniform((min_x - 2, min_y - 2), (max_x + 3, max_y + 3), (n, 2))]
    rows.append(np.stack([ex.astype(f32), rng.uniform(min_y, max_y, nx + 1).astype(f32)], 1))
    rows.append(np.stack([rng.uniform(min_x, max_x, ny + 1).astype(f32), ey.astype(f32)], 1))
    rows.append([[ex[0], ey[0]], [ex[-1], ey[-1]], [ex[-1], ey[0]], [ex[0], ey[-1]], [np.nextafter(f32(ex[-1]), f32(np.inf)), ey[1]]])
    for k, c in enumerate((9, 10, 11, 300)):
        cx, cy = 3 + 4 * k, 5 + 3 * k
        rows.append(np.stack([rng.uniform(ex[cx], ex[cx + 1], c), rng.uniform(ey[cy], ey[cy + 1], c)], 1))
    rows.append([[np.nan, 0.0], [0.0, np.nan], [np.nan, np.nan], [np.inf, 0.0], [0.0, -np.inf], [-np.inf, np.inf]])
    xy = np.concatenate([np.asarray(r, np.float64) for r in rows]).astype(f32)
    pts = np.concatenate([xy, rng.normal(size=(len(xy), columns - 2)).astype(f32)], 1)
    pts[rng.random(len(pts)) < 0.05, 0] = np.nan
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def pred_bev(grid, width=None, seed=2):
    nx = (grid[1] - grid[0]) * grid[4]
    rng = np.random.default_rng(seed)
    bev = rng.uniform(0, 1, (3, nx, width or (grid[3] - grid[2]) * grid[4])).astype(np.float32)
    bev[:, 0, :4] = [[1.0, 1.0, 0.0, 1 / 3], [1.0, 0.0, 0.0, 1 / 3], [1.0, 1.0, 0.0, 1 / 3]]      # the range's ends and a mean that is not exact
    return bev


def scene(kind, grid, ego, seed=3):
    """(pred_loc, cast_locs, cast_cmds, det, tgt) of a scene, in the units the reference hands to visualize: metres relative to
    the ego pixel for locations, panel pixels for detections."""
    rng = np.random.default_rng(seed)
    ppm = grid[4]
    H, W = (grid[1] - grid[0]) * ppm, (grid[3] - grid[2]) * ppm
    f32 = np.float32
    to_loc = lambda px: ((np.asarray(px, np.float64) - ego) / ppm).astype(f32)          # noqa: E731
    plan = to_loc(np.stack([ego[0] + rng.uniform(-3, 3, 20), ego[1] - np.arange(20) * 1.5], 1))
    none = (np.zeros((0, 6, 20, 2), f32), np.zeros((0, 6), f32), [[], []])               # the reference's CPU zeros for no vehicles
    if kind == "empty":
        return (plan, *none, [0.5, -3.0])
    if kind == "full":         # 15 vehicles, every command above the threshold: 1800 forecast dots all over the panel
        starts = rng.uniform((0, 0), (W, H), (15, 1, 1, 2))
        locs = to_loc(starts + np.cumsum(rng.normal(0, 1.2, (15, 6, 20, 2)), axis=2))
        cmds = rng.uniform(0.2, 1.0, (15, 6)).astype(f32)
        cmds[0, 0], cmds[0, 1] = CMD_THRESH, 1.0
        det = [[(3.0, 3.0, 1.0, 1.0, 1.0, 0.0)], [(float(x), float(y), float(w), float(h), float(np.cos(a)), float(np.sin(a)))
                                                  for x, y, w, h, a in zip(rng.integers(0, W, 15), rng.integers(0, H, 15), rng.uniform(1, 6, 15),
                                                                           rng.uniform(1, 9, 15), rng.uniform(0, 6.3, 15))]]
        return plan, locs, cmds, det, [2.0, -4.0]
    if kind == "pile":         # every dot within a few pixels of one spot: more records than a tile's list holds
        spot = np.array([W * 0.6, H * 0.4])
        locs = to_loc(spot + rng.uniform(-3, 3, (15, 6, 20, 2)))
        cmds = rng.uniform(0.25, 1.0, (15, 6)).astype(f32)
        det = [[], [(float(spot[0]), float(spot[1]), 2.0, 3.0, 0.6, 0.8)] * 15]
        return to_loc(spot + rng.uniform(-2, 2, (20, 2))), locs, cmds, det, list((spot - ego) / ppm)
    if kind == "straddle":     # on the left and right edges of the panel, on its top and bottom, and wholly outside it
        xs = np.array([-60.0, -2, -1, 0, 1, W - 2, W - 1, W, W + 1, W + 60])
        ys = np.array([-40.0, -1, 0, H / 2, H - 1, H, H + 40])
        pts = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
        locs = to_loc(np.resize(pts, (4, 6, 20, 2)))
        cmds = np.full((4, 6), 0.9, f32)
        cmds[1, 2], cmds[2, 5] = 0.1, np.float32(0.19999)                                # below the threshold: not drawn
        det = [[], [(-1.0, 10.0, 3.0, 5.0, 0.8, 0.6), (W - 0.5, 20.0, 4.0, 2.0, 0.0, 1.0), (W + 30.0, 5.0, 3.0, 3.0, 1.0, 0.0), (-40.0, 5.0, 3.0, 3.0, 1.0, 0.0),
                        (10.0, -2.0, 6.0, 2.0, 0.6, -0.8), (W / 2, H + 1.0, 3.0, 8.0, 0.28, 0.96), (1e9, -1e9, 1e9, 1.0, 1.0, 0.0), (5.0, 5.0, 0.0, 0.0, 1.0, 0.0)]]
        return to_loc(pts[:20]), locs, cmds, det, [400.0, -400.0]                        # (the target is clipped to [0, 255])
    if kind == "overlap":      # plan, forecasts, a box and the target on the same pixels: the later kind wins
        line = np.stack([np.full(20, ego[0] + 2.0), ego[1] - 2.0 * np.arange(20)], 1)
        locs = to_loc(np.resize(line + [1.0, 0.0], (2, 6, 20, 2)))
        cmds = np.array([[0.2, 0.4, 0.6, 0.8, 1.0, 0.3], [0.9, 0.1, 0.5, 0.7, 0.25, 1.5]], f32)
        det = [[], [(ego[0] + 2.0, ego[1] - 10.0, 2.0, 6.0, 1.0, 0.0), (ego[0] + 3.0, ego[1] - 8.0, 4.0, 4.0, 0.7071, 0.7071)]]
        return to_loc(line), locs, cmds, det, [2.0 / ppm, -10.0 / ppm]
    raise KeyError(kind)


def controls(seed=4):
    """(cmd, spd, steer, throt, brake, pred_bra) for the text."""
    rng = np.random.default_rng(seed)
    return int(rng.integers(0, 6)), float(rng.uniform(0, 9)), float(rng.uniform(-1, 1)), float(rng.uniform(0, 0.8)), float(rng.integers(0, 2)), float(rng.uniform(0, 1))
