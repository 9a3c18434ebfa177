"""Reference of lav_heads_at_peaks for tests/test_heads_peaks_host.py and tests/test_gpu_heads_at_peaks.py: torch on the CPU in
float64 of the module's own layers (Conv2d -> ReLU -> BatchNorm2d eval -> ConvTranspose2d), evaluated densely and gathered at the rows;
the 2e-6 sum|a||b| bar of the hidden dot products carried through the tail's weights; rows placed by hand."""
import copy

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn


def make_head(cin, hidden, outs, seed):
    """(conv, bn, deconv) of lav_amd.lidar.Head's shape with seeded float32 parameters and running statistics, in eval mode."""
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(cin, hidden, 3, 1, 1, bias=False)
    bn = nn.BatchNorm2d(hidden)
    ct = nn.ConvTranspose2d(hidden, outs, 3, 2, 1, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (3.0 * cin ** 0.5))
        bn.running_mean.copy_(0.3 * torch.randn(hidden, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(hidden, generator=g))
        bn.weight.copy_(1.0 + 0.3 * torch.randn(hidden, generator=g))      # some negative scales among them is fine: |scale| in the bar
        bn.bias.copy_(0.2 * torch.randn(hidden, generator=g))
        ct.weight.copy_(torch.randn(ct.weight.shape, generator=g) / (2.0 * hidden ** 0.5))
        ct.bias.copy_(0.5 * torch.randn(outs, generator=g))
    for m in (conv, bn, ct):
        m.eval()
    return conv, bn, ct


def dense_reference(feat, head):
    """feat (cin, H, W) -> (values (outs, 2H, 2W) float64, bound (outs, 2H, 2W)): the head's layers in float64, and
    2e-6 * sum|w||f| of every hidden dot product, times |BatchNorm scale|, carried through |tail weights|."""
    conv, bn, ct = (copy.deepcopy(m).double() for m in head)
    x = feat.double()[None]
    with torch.no_grad():
        vals = ct(bn(F.relu(conv(x))))[0]
        scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).abs()
        mag = F.conv2d(x.abs(), conv.weight.abs(), None, 1, 1) * scale[None, :, None, None]
        bound = 2e-6 * F.conv_transpose2d(mag, ct.weight.abs(), None, 2, 1, 1)[0]
    return vals, bound


def live_mask(rows, H, W):
    """Rows lav_heads_at_peaks evaluates: score above the sentinel, x / y finite and inside [0, 2W) x [0, 2H)."""
    r = np.asarray(rows, np.float64)
    with np.errstate(invalid="ignore"):
        return (r[..., 0] > -1e4) & (r[..., 1] >= 0) & (r[..., 1] < 2 * W) & (r[..., 2] >= 0) & (r[..., 2] < 2 * H)


def gather(rows, maps, H, W):
    """rows (ncls, D, 3) float32, maps: list of (outs, 2H, 2W) arrays -> (ncls, D, sum outs): the maps at (y, x) of every live row,
    zeros for the others."""
    rows = np.asarray(rows)
    live = live_mask(rows, H, W)
    out = np.zeros(rows.shape[:2] + (sum(m.shape[0] for m in maps),), np.float64)
    for c in range(rows.shape[0]):
        for d in range(rows.shape[1]):
            if live[c, d]:
                x, y = int(rows[c, d, 1]), int(rows[c, d, 2])
                out[c, d] = np.concatenate([np.asarray(m)[:, y, x] for m in maps])
    return out


def hand_rows(H, W, ncls=2, max_det=15):
    """(ncls, max_det, 3) float32 rows placed by hand on a 2H x 2W map: all four parities, the four corners (the odd last row /
    column is where hidden index H resp. W must be dropped), pixels next to each border, one pixel twice, rows of the other class,
    and three rows that must come back as zeros: the sentinel, x = NaN, y = 2H.  Returns (rows, indices (cls, d) of the bad rows)."""
    X, Y = 2 * W - 1, 2 * H - 1
    c0 = [(0, 0), (X, 0), (0, Y), (X, Y),                      # corners
          (2, 2), (3, 2), (2, 3), (3, 3),                      # even/even, odd/even, even/odd, odd/odd in the interior
          (1, 4), (X - 1, 3), (4, 1), (5, Y - 1),              # next to the left, right, top, bottom border
          (3, 3),                                              # the same pixel again
          (X, 2), (1, Y)]
    c1 = [(X - 2, Y - 2), (0, 5), (6, 0), (X, Y - 1), (X - 1, Y), (7, 4), (2, 5), (3, 3), (1, 1), (X - 3, 1), (4, Y), (5, 5)]
    rows = np.zeros((ncls, max_det, 3), np.float32)
    for c, pts in enumerate((c0, c1)):
        assert len(pts) <= max_det and all(0 <= x <= X and 0 <= y <= Y for x, y in pts)
        for d, (x, y) in enumerate(pts):
            rows[c, d] = (0.9 - 0.01 * d - 0.3 * c, x, y)
    bad = [(1, 12), (1, 13), (1, 14)]
    rows[1, 12] = (-1e5, 0, 0)                                  # lav_extract_peaks' "no candidate" row
    rows[1, 13] = (0.5, np.nan, 3)
    rows[1, 14] = (0.4, 2, 2 * H)
    return rows, bad
