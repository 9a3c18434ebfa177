"""The loaders' BEV map stacks as plane records, rendered behind the upload (`--bev-on-device` of train_bev_v2 / train_full_v2).

Every BEV output plane of every loader of lav_amd.data.datasets is

    out = ( W2( crop( W1(src) ) ) > 0 )

src a decoded uint8 map plane, W1 and W2 cv2.warpAffine(INTER_LINEAR, border 0) as lav_amd.data.image restates it (8-bit fixed point),
crop(I)[r, c] = I[r + shift[0], c + shift[1]] with zero where the index leaves the image - the loaders' pad by MARGIN, then slice.
The temporal stack rotates by the relative heading (W1), shifts by the ego motion and the jitter and rotates by the angle jitter
(W2); the single-frame loaders rotate by the jitter (W1), shift the columns and have W2 = identity, which the fixed-point path passes
exactly.

A loader built with bev_on_device=True returns a BevRecord where its tuple holds `bev`: the decoded planes, the twelve inverse-map
coefficients of every plane (float64, from the same NumPy expressions warp_affine_linear evaluates: the device computes no sine, no
cosine and no quotient) and its shift.  BevStacker renders a batch of records: lav_bev_stack_u8 (csrc/bev_stack.hip, one launch) for
planes in HBM, bev_stack_numpy - the specification - for planes on the host; the two agree bit for bit.

PARITY UNPINNED against OpenCV itself, as for warp_affine_linear: what is pinned is the kernel against this module, and this module
against the reference loaders run over that restatement (tests/test_data_host.py).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import image

IDENTITY = np.array(image.IDENTITY_INVERSE_MAP, np.float64)
COORD_LIMIT = float(1 << 30)      # |source coordinate| a coefficient set may produce: keeps the 1/1024-pixel integers far inside int64


class BevRecord(NamedTuple):
    """planes (..., P, H, W) uint8: the decoded sources in output-channel order (zeros for a missing history frame);
    coef (..., P, 12) float64: i00, i01, i10, i11, b1, b2 of W1, then of W2; shift (..., P, 2) int32: rows, columns."""
    planes: object
    coef: object
    shift: object


def plane_record(planes: np.ndarray, w1, shift, w2=None, limit: int = None, frame=None) -> BevRecord:
    """The record of C planes that share their warps.  planes (C, H, W) uint8; w1 / w2: forward 2 x 3 matrices as
    image.rotation_matrix_2d returns them (w2 None: the identity); shift (rows, columns).  limit: the largest |shift| the host path can
    render (its zero border): beyond it a ValueError names the frame."""
    planes = np.ascontiguousarray(planes, np.uint8)
    sr, sc = int(shift[0]), int(shift[1])
    if limit is not None and (abs(sr) > limit or abs(sc) > limit):
        raise ValueError(f"frame {frame}: BEV shift ({sr}, {sc}) is beyond the +-{limit} pixel border the map is padded with")
    row = np.concatenate([image.inverse_map(w1), IDENTITY if w2 is None else image.inverse_map(w2)])
    n = len(planes)
    return BevRecord(planes, np.tile(row, (n, 1)), np.tile(np.array([sr, sc], np.int32), (n, 1)))


def zero_record(n: int, h: int, w: int) -> BevRecord:
    """n planes that render to zeros (a history frame before the route's first)."""
    return BevRecord(np.zeros((n, h, w), np.uint8), np.tile(np.concatenate([IDENTITY, IDENTITY]), (n, 1)), np.zeros((n, 2), np.int32))


def concat_records(records) -> BevRecord:
    return BevRecord(*(np.concatenate(parts) for parts in zip(*records)))


def is_identity(coef6, h: int, w: int) -> bool:
    """The inverse map that the fixed-point path passes exactly (image sides up to the +-32768 coordinate clamp)."""
    return bool(np.all(np.asarray(coef6) == IDENTITY)) and h <= 32768 and w <= 32768


def _as_numpy(a, dtype):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype)


def check_record(planes_shape, coef, shift):
    """coef (N, 12) float64 and shift (N, 2) int32 of a record whose planes have `planes_shape` (..., H, W); raises on a shape that
    does not match, a coefficient that is not finite or a map that leaves +-2^30 pixels."""
    if len(planes_shape) < 3:
        raise ValueError(f"planes: expected (..., P, H, W), got {tuple(planes_shape)}")
    lead, (h, w) = tuple(planes_shape[:-2]), planes_shape[-2:]
    coef, shift = _as_numpy(coef, np.float64), _as_numpy(shift, np.int32)
    if coef.shape != lead + (12,) or shift.shape != lead + (2,):
        raise ValueError(f"planes {tuple(planes_shape)} need coef {lead + (12,)} and shift {lead + (2,)}, got {coef.shape} and {shift.shape}")
    coef, shift = coef.reshape(-1, 12), shift.reshape(-1, 2)
    if not np.isfinite(coef).all():
        raise ValueError("coef: a coefficient is not finite")
    reach = np.abs(coef[:, [0, 2, 6, 8]]) * w + np.abs(coef[:, [1, 3, 7, 9]]) * h + np.abs(coef[:, [4, 5, 10, 11]])
    if reach.size and reach.max() >= COORD_LIMIT:
        raise ValueError(f"coef: a map reaches {reach.max():.3g} pixels (limit 2^30)")
    return coef, shift


def crop_shift(img: np.ndarray, sr: int, sc: int) -> np.ndarray:
    """crop(I)[r, c] = I[r + sr, c + sc] for (H, W, C) images, zero outside: pad / slice for any shift."""
    H, W = img.shape[:2]
    out = np.zeros_like(img)
    r0, r1, c0, c1 = max(0, -sr), min(H, H - sr), max(0, -sc), min(W, W - sc)
    if r1 > r0 and c1 > c0:
        out[r0:r1, c0:c1] = img[r0 + sr:r1 + sr, c0 + sc:c1 + sc]
    return out


def bev_stack_numpy(planes, coef, shift, threshold: bool = True) -> np.ndarray:
    """The specification: planes (..., P, H, W) uint8, coef (..., P, 12), shift (..., P, 2) -> (..., P, H, W) uint8, W2(crop(W1(src))) > 0
    per plane, or the interpolated values themselves with threshold=False.  Runs of planes with equal coefficients and shift are
    warped together (as the loaders warp a frame's channels); an identity map is skipped, the fixed-point path would pass it exactly."""
    planes = _as_numpy(planes, np.uint8)
    coef, shift = check_record(planes.shape, coef, shift)
    h, w = planes.shape[-2:]
    src = planes.reshape(-1, h, w)
    out = np.empty_like(src)
    n, lo = len(src), 0
    while lo < n:
        hi = lo + 1
        while hi < n and np.array_equal(coef[hi], coef[lo]) and np.array_equal(shift[hi], shift[lo]):
            hi += 1
        img = src[lo:hi].transpose(1, 2, 0)
        if not is_identity(coef[lo, :6], h, w):
            img = image.warp_inverse_linear(img, coef[lo, :6])
        if shift[lo].any():
            img = crop_shift(img, int(shift[lo, 0]), int(shift[lo, 1]))
        if not is_identity(coef[lo, 6:], h, w):
            img = image.warp_inverse_linear(np.ascontiguousarray(img), coef[lo, 6:])
        out[lo:hi] = img.transpose(2, 0, 1)
        lo = hi
    out = out.reshape(planes.shape)
    return (out > 0).astype(np.uint8) if threshold else out


class BevStacker:
    """Renders BevRecords: planes in HBM through lav_bev_stack_u8 (one launch per batch, on the current stream; the coefficient tables
    are uploaded with it), planes on the host through bev_stack_numpy.  Returns the uint8 `bev` tensor the trainers take, on the
    planes' device."""

    def __init__(self, threshold: bool = True):
        self.threshold = bool(threshold)

    def __call__(self, record, device=None) -> torch.Tensor:
        planes, coef, shift = record
        if not isinstance(planes, torch.Tensor):
            planes = torch.from_numpy(np.ascontiguousarray(planes, np.uint8))
        if device is not None:
            planes = planes.to(device)
        if planes.dtype != torch.uint8:
            raise ValueError(f"planes: expected uint8, got {planes.dtype}")
        if planes.is_cuda:
            from .. import ops
            return ops.bev_stack_u8(planes, coef, shift, self.threshold)
        return torch.from_numpy(bev_stack_numpy(planes, coef, shift, self.threshold))
