"""Shared by tests/test_crop_host.py and tests/test_gpu_crop.py: the geometries and poses of the rotated-crop tests, a float64
statement of the crop as a matrix, and the library's kernel choice restated in float32.

The crop is linear in the map: out[i] = A[i] @ map, A[i] of shape (crop * crop, H * W), row = output pixel y * crop + x,
column = map pixel sy * W + sx.  crop_matrix_f64 writes A[i] down from the formulas in the header comment of crop.hip."""
import math

import numpy as np
import torch

PPM = 2.0
OFFSETS = ((0.0, 0.75), (0.1, 0.5))
ORIS = (0.0, math.pi / 2, math.pi, -math.pi / 2, math.pi / 4, 0.3, -1.2, 2.9)
LOC_KINDS = ("zero", "whole_pixel", "half_pixel", "half_off", "off_map", "centred")

# (H, W, crop) -> (forward kernel, backward kernel) the library picks on its own; tests/test_crop_host.py checks this column against
# the float32 restatement of the two predicates below
GEOMETRIES = {
    (12, 12, 12): ("staged", "staged"),     # pitch exactly 1, a single tile
    (24, 24, 13): ("staged", "staged"),     # odd crop, 2 x 2 map tiles, 1 output tile
    (40, 40, 24): ("staged", "staged"),     # the trainer's pitch; 3 x 3 map tiles, 2 x 2 output tiles
    (20, 28, 14): ("general", "staged"),    # W > H: x pitch 1.45
    (28, 20, 14): ("staged", "general"),    # H > W: 4 candidates per axis - the only natural route to k_crop_rotate_bwd_general
    (3, 5, 2): ("general", "staged"),       # the smallest legal sizes
}
SQUARE = tuple(g for g in GEOMETRIES if g[0] == g[1])


def geom_id(g):
    return "%dx%d_crop%d" % g


def locs_of(H, W, ppm=PPM):
    """One location per kind, in metres.  The kernel shifts the grid by rx = loc_x ppm / (H/2), ry = loc_y ppm / (W/2) in
    normalised units, where one map pixel is 2/(W-1) along x and 2/(H-1) along y."""
    px, py = H / ((W - 1) * ppm), W / ((H - 1) * ppm)       # metres per map pixel along x / y
    return {"zero": (0.0, 0.0),
            "whole_pixel": (2 * px, -1 * py),
            "half_pixel": (0.5 * px, 1.5 * py),
            "half_off": (H / (2 * ppm), 0.0),                    # rx = 1: the crop's centre on the map's right edge
            "off_map": (6 * H / (2 * ppm), -6 * W / (2 * ppm))}   # rx = 6, ry = -6: |k R (xs, ys)| <= sqrt(2), the pivot terms < 2


def poses(H, W, crop, ox, oy, ppm=PPM):
    """Every kind of location at every orientation -> locs (48, 2) float32, oris (48,) float32, kinds (list of 48 names).
    `centred` cancels the pivot terms of the translation (tx = ty = 0, which a fixed location does at ori = 0 only): where the
    pitch is 1 the four axis-aligned orientations then sample pixel centres, up to the rounding floorf has to cope with."""
    at = locs_of(H, W, ppm)
    k = crop / H
    locs, oris, kinds = [], [], []
    for kind in LOC_KINDS:
        for o in ORIS:
            if kind == "centred":
                cs, sn = math.cos(o), math.sin(o)
                loc = (-(-k * ox * cs + k * oy * sn + ox) * (H / 2) / ppm, -(-k * ox * sn - k * oy * cs + oy) * (W / 2) / ppm)
            else:
                loc = at[kind]
            locs.append(loc); oris.append(o); kinds.append(kind)
    return torch.tensor(locs, dtype=torch.float32), torch.tensor(oris, dtype=torch.float32), kinds


def random_poses(H, W, n, seed, ppm=PPM):
    """n seeded poses: centres up to 1.2 half-maps from the middle (some crops partly off the map), any orientation."""
    r = np.random.Generator(np.random.PCG64(seed))
    locs = r.uniform(-1.2, 1.2, (n, 2)) * np.array([H / (2 * ppm), W / (2 * ppm)])
    oris = r.uniform(-math.pi, math.pi, n)
    return torch.from_numpy(locs.astype(np.float32)), torch.from_numpy(oris.astype(np.float32))


def chunks(n, size=8):
    return [slice(a, min(a + size, n)) for a in range(0, n, size)]


def crop_positions_f64(H, W, crop, locs, oris, ppm, ox, oy):
    """Sample position (ix, iy), in map pixels, of every output pixel: two (n, crop, crop) float64 arrays indexed [i, y, x]."""
    locs = np.asarray(locs, dtype=np.float64).reshape(-1, 2)
    oris = np.asarray(oris, dtype=np.float64).reshape(-1)
    k = crop / H
    cs, sn = np.cos(oris), np.sin(oris)
    tx = -k * ox * cs + k * oy * sn + ox + locs[:, 0] * ppm / (H / 2)
    ty = -k * ox * sn - k * oy * cs + oy + locs[:, 1] * ppm / (W / 2)
    lin = np.linspace(-1.0, 1.0, crop)
    xs, ys = lin[None, None, :], lin[None, :, None]
    cs, sn, tx, ty = (a[:, None, None] for a in (cs, sn, tx, ty))
    gx = k * cs * xs - k * sn * ys + tx
    gy = k * sn * xs + k * cs * ys + ty
    return (gx + 1) / 2 * (W - 1), (gy + 1) / 2 * (H - 1)        # align_corners=True


def crop_matrix_f64(H, W, crop, locs, oris, ppm, ox, oy):
    """(n, crop * crop, H * W) float64: bilinear weights of the four pixels around each sample position, zeros outside the map."""
    ix, iy = crop_positions_f64(H, W, crop, locs, oris, ppm, ox, oy)
    n = ix.shape[0]
    ix, iy = ix.reshape(n, -1), iy.reshape(n, -1)
    fx, fy = np.floor(ix), np.floor(iy)
    wx1, wy1 = ix - fx, iy - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    A = np.zeros((n, crop * crop, H * W), dtype=np.float64)
    i_idx, r_idx = np.meshgrid(np.arange(n), np.arange(crop * crop), indexing="ij")
    for dx, dy, w in ((0, 0, (1 - wx1) * (1 - wy1)), (1, 0, wx1 * (1 - wy1)), (0, 1, (1 - wx1) * wy1), (1, 1, wx1 * wy1)):
        xx, yy = x0 + dx, y0 + dy
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        A[i_idx[ok], r_idx[ok], (yy * W + xx)[ok]] = w[ok]
    return A


def torch_crop_matrix(H, W, crop, locs, oris, ppm, ox, oy, dtype):
    """The same matrices from planner_common.crop_feature_torch (affine_grid + grid_sample on the CPU) on identity maps, computed
    in `dtype`: (n, crop * crop, H * W)."""
    from lav_amd.planner_common import crop_feature_torch
    n = locs.shape[0]
    basis = torch.eye(H * W, dtype=dtype).view(1, H * W, H, W).expand(n, -1, -1, -1)
    out = crop_feature_torch(basis, locs.to(dtype), oris.to(dtype), ppm, crop, ox, oy)
    return out.reshape(n, H * W, crop * crop).transpose(1, 2)


# crop.hip's host-side kernel choice, restated operation by operation in float32 (crop_fwd_staged_ok / crop_bwd_staged_ok; the
# tile sizes are its FWD_TILE = BWD_TW = 16 and BWD_MAXSPAN = 3)
def _pitches(H, W, crop):
    f = np.float32
    k, step = f(crop) / f(H), f(2) / f(crop - 1)
    return k * step * f(0.5) * f(W - 1), k * step * f(0.5) * f(H - 1)     # map pixels per output pixel along x / y


def fwd_staged_ok(H, W, crop):
    f = np.float32
    return bool(f(15) * f(1.41421357) * max(_pitches(H, W, crop)) + f(5) <= f(32))


def bwd_staged(H, W, crop):
    """-> (staged?, candidates per axis, upper bound of a tile's box side)."""
    f = np.float32
    pitch_min = min(_pitches(H, W, crop))
    reach = f(1.41421357) / pitch_min + f(0.01)
    span = int(np.floor(f(2) * reach)) + 1
    box = f(15) * f(1.41421357) / pitch_min + f(2) * reach + f(3)
    return bool(span <= 3 and box <= f(32)), span, float(box)
