"""The three OpenCV calls the reference's data loaders make, restated on numpy + PIL (this image has no cv2):
`cv2.imdecode`, `cv2.getRotationMatrix2D` and `cv2.warpAffine(..., flags=cv2.INTER_LINEAR)` on 8-bit images
(lav/utils/datasets/basic_dataset.py:84-101, bev_dataset.py:81-85).

warp_affine_linear follows OpenCV 4's fixed-point path for 8-bit bilinear warps (imgproc/src/imgwarp.cpp: warpAffine ->
remapBilinear): the inverse map is evaluated in 1/1024 pixel integers with a rounding offset of 16, source coordinates are
cut to 1/32 pixel, the four weights are (32 - a)(32 - b) * 32 / 32768 exactly, the sum is rounded with +2^14 >> 15, and
pixels outside the source read the constant border 0.  PARITY UNPINNED against OpenCV itself (none here to compare with);
the loaders only use the result through `> 0`, so only pixels whose interpolated value rounds to zero could differ.

resize_linear_u8 restates a fourth call, `cv2.resize` on 8-bit images (the agent's debug view, team_code_v2/lav_agent_fast.py:
497-503), in the same way and with the same caveat: parity with OpenCV itself is UNPINNED.
"""
from __future__ import annotations

import io

import numpy as np

IMREAD_GRAYSCALE, IMREAD_COLOR = 0, 1
INTER_LINEAR = 1


def imdecode(buf, mode: int) -> np.ndarray:
    """Encoded image bytes -> (H, W) uint8 for IMREAD_GRAYSCALE, (H, W, 3) BGR uint8 for IMREAD_COLOR."""
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(buf)))
    if mode == IMREAD_GRAYSCALE:
        return np.asarray(im.convert("L"))
    if mode == IMREAD_COLOR:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])
    raise NotImplementedError(f"imdecode mode {mode}")


def imencode_png(img: np.ndarray) -> bytes:
    """(H, W) uint8 -> PNG bytes (what the data collector stores under map_*/sem_* keys); for building test routes."""
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img)).save(out, format="PNG")
    return out.getvalue()


def rotation_matrix_2d(center, angle_deg: float, scale: float = 1.0) -> np.ndarray:
    """cv2.getRotationMatrix2D: positive angles rotate counter-clockwise about `center` (x, y), origin top-left."""
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))      # cv::Point2f
    a = angle_deg * np.pi / 180.0
    alpha, beta = np.cos(a) * scale, np.sin(a) * scale
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], np.float64)


def resize_linear_table(src: int, dst: int) -> np.ndarray:
    """One axis of resize_linear_u8 as (dst, 4) int32 rows (i0, i1, w0, w1): output index d reads source indices i0 and i1 with
    the 11-bit weights w0 and w1.  The source coordinate is float32((d + 0.5) * scale - 0.5) with scale = src / dst in float64;
    its floor is the index and the rest the fraction; an index left of the image or on / right of its last pixel is clamped to
    the edge with the fraction zeroed; the weights are rint(2048 * (1 - fraction)) and rint(2048 * fraction) in float32."""
    if src < 1 or dst < 1:
        raise ValueError(f"resize_linear_table: sizes {src} -> {dst}")
    scale = np.float64(src) / np.float64(dst)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i0 = np.floor(f).astype(np.int64)
    f = f - i0.astype(np.float32)
    left, right = i0 < 0, i0 >= src - 1
    f[left | right] = 0
    i0[left] = 0
    i0[right] = src - 1
    w0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int32)
    w1 = np.rint(f * np.float32(2048)).astype(np.int32)
    return np.stack([i0.astype(np.int32), np.minimum(i0 + 1, src - 1).astype(np.int32), w0, w1], axis=1)


def resize_linear_u8(image: np.ndarray, dsize) -> np.ndarray:
    """cv2.resize(image, dsize) (dsize = (width, height), INTER_LINEAR) for uint8 images of shape (H, W) or (H, W, C), restating
    OpenCV 4's fixed-point path for 8-bit bilinear resizing (imgproc/src/resize.cpp: HResizeLinear / VResizeLinear): the
    horizontal pass is S[i0] * w0 + S[i1] * w1 unshifted (resize_linear_table holds the indices and the 11-bit weights), the
    vertical pass (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.  Written from the memory of that source: this
    function is the specification of the debug view (lav_amd/agent/debug_view.py, csrc/debug_view.hip reproduces it bit for
    bit); PARITY UNPINNED against OpenCV itself, as for warp_affine_linear."""
    if image.dtype != np.uint8:
        raise TypeError("resize_linear_u8 restates the 8-bit fixed-point path only")
    src = image if image.ndim == 3 else image[..., None]
    dw, dh = int(dsize[0]), int(dsize[1])
    tx, ty = resize_linear_table(src.shape[1], dw), resize_linear_table(src.shape[0], dh)
    s = src.astype(np.int64)
    rows = s[:, tx[:, 0]] * tx[:, 2].astype(np.int64)[None, :, None] + s[:, tx[:, 1]] * tx[:, 3].astype(np.int64)[None, :, None]
    b0, b1 = ty[:, 2].astype(np.int64)[:, None, None], ty[:, 3].astype(np.int64)[:, None, None]
    out = (((b0 * (rows[ty[:, 0]] >> 4)) >> 16) + ((b1 * (rows[ty[:, 1]] >> 4)) >> 16) + 2) >> 2
    out = np.minimum(out, 255).astype(np.uint8)          # (saturate_cast: a weight pair may sum to 2049)
    return out if image.ndim == 3 else out[..., 0]


IDENTITY_INVERSE_MAP = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def inverse_map(M) -> np.ndarray:
    """The six float64 coefficients (i00, i01, i10, i11, b1, b2) warpAffine derives from the forward matrix M: output pixel (x, y)
    samples the source at (i00 x + i01 y + b1, i10 x + i11 y + b2)."""
    m = np.array(M, np.float64).reshape(2, 3)
    # forward map -> inverse map, exactly as warpAffine does it
    D = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = m[1, 1] * D, m[0, 0] * D
    i00, i01, i10, i11 = a11, m[0, 1] * -D, m[1, 0] * -D, a22
    b1 = -i00 * m[0, 2] - i01 * m[1, 2]
    b2 = -i10 * m[0, 2] - i11 * m[1, 2]
    return np.array([i00, i01, i10, i11, b1, b2], np.float64)


def warp_affine_linear(image: np.ndarray, M: np.ndarray) -> np.ndarray:
    """cv2.warpAffine(image, M, (W, H), flags=INTER_LINEAR) for uint8 images of shape (H, W) or (H, W, C); constant border 0."""
    if image.dtype != np.uint8:
        raise TypeError("warp_affine_linear restates the 8-bit fixed-point path only")
    return warp_inverse_linear(image, inverse_map(M))


def warp_inverse_linear(image: np.ndarray, coef) -> np.ndarray:
    """warp_affine_linear from the inverse map's coefficients (inverse_map's six): the fixed-point remap itself.  This is the
    arithmetic lav_bev_stack_u8 (csrc/bev_stack.hip) reproduces bit for bit."""
    if image.dtype != np.uint8:
        raise TypeError("warp_inverse_linear restates the 8-bit fixed-point path only")
    src = image if image.ndim == 3 else image[..., None]
    H, W, _ = src.shape
    i00, i01, i10, i11, b1, b2 = (np.float64(c) for c in coef)
    AB_SCALE, ROUND = 1024, 16
    xs = np.arange(W, dtype=np.float64)
    ys = np.arange(H, dtype=np.float64)
    adelta = np.rint(i00 * xs * AB_SCALE).astype(np.int64)
    bdelta = np.rint(i10 * xs * AB_SCALE).astype(np.int64)
    X0 = np.rint((i01 * ys + b1) * AB_SCALE).astype(np.int64) + ROUND
    Y0 = np.rint((i11 * ys + b2) * AB_SCALE).astype(np.int64) + ROUND
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    sx = np.clip(X >> 5, -32768, 32767)
    sy = np.clip(Y >> 5, -32768, 32767)
    fx, fy = (X & 31), (Y & 31)
    w = np.stack([(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx], 0) * 32          # sums to 32768

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
        return v * ok[..., None]

    acc = (tap(sy, sx) * w[0][..., None] + tap(sy, sx + 1) * w[1][..., None]
           + tap(sy + 1, sx) * w[2][..., None] + tap(sy + 1, sx + 1) * w[3][..., None])
    out = ((acc + (1 << 14)) >> 15).astype(np.uint8)
    return out if image.ndim == 3 else out[..., 0]
