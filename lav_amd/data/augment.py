"""Image augmentation of the camera trainers (`train_seg.py --augment`, `train_bra_v2.py --augment`).

The reference passes every camera image of its 'seg' and 'bra' loaders through `augment(0.5)` (lav/utils/augmenter.py): seven
imgaug operations - Gaussian blur, additive Gaussian noise, pixel dropout, brightness multiply, linear contrast, partial
grayscale, an elastic warp - in random order, each with probability 0.5; only the image is augmented, never the labels.
imgaug does not exist here, so the semantics below are this project's own restatement of that call and of imgaug 0.4's documented
behaviour.  PARITY WITH IMGAUG IS UNPINNED: there are no recorded imgaug outputs to compare with, and its random stream is not
reproduced.  What is pinned: the HIP kernel (csrc/augment.hip, `ops.augment_u8`) against `augment_numpy` below - bit for bit for
every op but noise - and `augment_numpy` against independent checks (tests/test_augment_host.py).

The specification
  per-sample parameters   drawn on the host from np.random.Generator(np.random.Philox(key=seed, counter=[0, 0, sample id, stream
                          tag])): the order (a permutation of the 7 ops), 7 Bernoulli(prob) activations, every op's scalars and
                          the per_channel Bernoulli(0.5) of noise / dropout / multiply / contrast - always all of them, in one fixed
                          sequence, so that sample n's record does not depend on the batch it arrives in.
                          sample id = rank + world * (images this Augmenter has drawn so far).
  per-pixel randomness    Philox4x32-10, key = the 64-bit seed, counter = (x, y, sample id, stream tag << 16 | op << 8 | draw):
                          a pixel's words depend on its global coordinates only.  Uniforms are (word >> 8) * 2^-24.
  every op                uint8 HWC RGB -> uint8: float32 arithmetic, every product and sum rounded separately in a fixed order,
                          round-half-to-even and clip to [0, 255] after the op (as imgaug does between augmenters).
  blur       sigma ~ U(0, 0.5), skipped below 1e-3.  Separable 5-tap Gaussian, weights in float64 on the host, normalised, passed
             as float32; horizontal pass, then vertical (float32 in between); border reflect-101.
  noise      scale ~ U(0, 12.75).  v + scale z, z = sqrt(-2 log u1) cos(2 pi u2), u1 in (0, 1]; one z per pixel or per pixel-channel.
  dropout    p ~ U(0.01, 0.1).  0 where u < p, per pixel or per pixel-channel.
  multiply   m ~ U(1/1.2, 1.2), one or three.  v m.
  contrast   a ~ U(1/1.2, 1.2), one or three.  128 + a (v - 128).
             These two take their float32 parameter into float64, where the expression is exact (24 + 8 bits), and round that: the
             correctly rounded value.  A float32 product misses it wherever it rounds ONTO a tie - v = 9, m = float32(1/1.2):
             7.49999982 -> 7.5 -> 8 - which the range ends 1/1.2 and 1.2 do on a twelfth of the grey levels.
  grayscale  alpha ~ U(0, 0.5).  g = (4899 R + 9617 G + 1868 B + 8192) >> 14;  v + alpha (g - v).
  elastic    alpha ~ U(0.5, 3.5), sigma = 0.25.  Raw field (dx, dy) = 2u - 1 per pixel, smoothed with the 5-tap scheme at sigma 0.25
             (reflect-101), times alpha; the image sampled at (x - dx, y - dy) with Keys' bicubic (a = -0.75), taps outside the
             image count as 0, rows summed first, in tap order.
prob = 0, or a sample whose seven draws are all inactive, returns the input bytes.
"""
from __future__ import annotations

import numpy as np
import torch

BLUR, NOISE, DROPOUT, MULTIPLY, CONTRAST, GRAYSCALE, ELASTIC = range(7)
OP_NAMES = ("blur", "noise", "dropout", "multiply", "contrast", "grayscale", "elastic")
NUM_OPS = 7
FIELD_SIGMA = 0.25

# lav_augment_params of include/lav_amd.h: 32 four-byte words per image
PARAMS_DTYPE = np.dtype([
    ("order", np.int32, 7), ("active", np.int32), ("per_channel", np.int32), ("sample", np.uint32), ("tag", np.uint32),
    ("blur_sigma", np.float32), ("blur_w", np.float32, 5), ("noise_scale", np.float32), ("dropout_p", np.float32),
    ("multiply", np.float32, 3), ("contrast", np.float32, 3), ("gray_alpha", np.float32), ("elastic_alpha", np.float32),
    ("field_w", np.float32, 5)])
assert PARAMS_DTYPE.itemsize == 128

RANGES = dict(blur_sigma=(0.0, 0.5), noise_scale=(0.0, 0.05 * 255), dropout_p=(0.01, 0.1), multiply=(1 / 1.2, 1.2),
              contrast=(1 / 1.2, 1.2), gray_alpha=(0.0, 0.5), elastic_alpha=(0.5, 3.5))


# ------------------------------------------------------------------------------------------------------------ Philox4x32-10
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32(c0, c1, c2, c3, key):
    """Philox4x32-10 (Salmon et al., Random123) over arrays of counters: c0..c3 broadcastable integer arrays of 32-bit words,
    key the 64-bit seed (key word 0 = its low half) or a pair of words.  Returns four uint32 arrays."""
    k0, k1 = (int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF) if np.isscalar(key) else (int(key[0]), int(key[1]))
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c).astype(np.uint64) & _LO for c in (c0, c1, c2, c3)))
    for r in range(10):
        p0, p1 = _M0 * c0, _M1 * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _uniform(word):
    return (word >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)                       # [0, 1)


def _uniform_open(word):
    return ((word >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)      # (0, 1]


def _pixel_words(h, w, rec, op, draw, seed):
    y, x = np.mgrid[0:h, 0:w]
    return philox4x32(x, y, int(rec["sample"]), int(rec["tag"]) | op << 8 | draw, seed)


# ------------------------------------------------------------------------------------------------------------ parameter tables
def gaussian_taps(sigma: float) -> np.ndarray:
    """The normalised 5-tap Gaussian, computed in float64, as float32; the identity kernel for sigma = 0."""
    if sigma <= 0:
        return np.array([0, 0, 1, 0, 0], np.float32)
    k = np.exp(-np.arange(-2, 3, dtype=np.float64) ** 2 / (2.0 * float(sigma) ** 2))
    return (k / k.sum()).astype(np.float32)


def make_params(n=1, order=None, active=(), sample0=0, sample_step=1, stream_tag=0, per_channel=(), blur_sigma=0.25, noise_scale=5.0,
                dropout_p=0.05, multiply=1.0, contrast=1.0, gray_alpha=0.25, elastic_alpha=2.0) -> np.ndarray:
    """An explicit table of n records (tests, probes): `active` / `per_channel` are collections of op ids or names, `order` a
    permutation of the op ids (default 0..6), multiply / contrast one value or three; samples sample0, sample0 + sample_step ..."""
    ident = lambda ops_: sum(1 << (OP_NAMES.index(o) if isinstance(o, str) else int(o)) for o in set(ops_))
    p = np.zeros(n, PARAMS_DTYPE)
    order = list(range(NUM_OPS)) if order is None else [OP_NAMES.index(o) if isinstance(o, str) else int(o) for o in order]
    if sorted(order) != list(range(NUM_OPS)):
        raise ValueError(f"order {order} is not a permutation of the {NUM_OPS} ops")
    p["order"] = order
    p["active"] = ident(active)
    p["per_channel"] = ident(per_channel)
    p["sample"] = (sample0 + sample_step * np.arange(n)) & 0xFFFFFFFF
    p["tag"] = (int(stream_tag) & 0xFFFF) << 16
    p["blur_sigma"], p["blur_w"] = blur_sigma, gaussian_taps(blur_sigma)
    p["noise_scale"], p["dropout_p"], p["gray_alpha"], p["elastic_alpha"] = noise_scale, dropout_p, gray_alpha, elastic_alpha
    p["multiply"] = np.broadcast_to(np.asarray(multiply, np.float32), (3,))
    p["contrast"] = np.broadcast_to(np.asarray(contrast, np.float32), (3,))
    p["field_w"] = gaussian_taps(FIELD_SIGMA)
    return p


def check_params(params: np.ndarray, n: int) -> np.ndarray:
    params = np.ascontiguousarray(params)
    if params.dtype != PARAMS_DTYPE or params.shape != (n,):
        raise ValueError(f"params: expected {n} records of augment.PARAMS_DTYPE, got {params.dtype} {params.shape}")
    if n and not (np.sort(params["order"], axis=1) == np.arange(NUM_OPS)).all():
        raise ValueError("params: every record's order must be a permutation of the 7 ops")
    return params


def draw_sample(prob: float, seed: int, sample: int, stream_tag: int = 0) -> np.ndarray:
    """The record of one sample id: a pure function of (prob, seed, sample, stream_tag)."""
    rng = np.random.Generator(np.random.Philox(key=int(seed), counter=[0, 0, int(sample), int(stream_tag)]))
    p = make_params(1, sample0=sample, stream_tag=stream_tag)      # (one record: the assignments below broadcast into it)
    p["order"] = rng.permutation(NUM_OPS)
    active = rng.random(NUM_OPS) < prob
    pc = rng.random(NUM_OPS) < 0.5          # (used by noise, dropout, multiply, contrast)
    u = lambda name, size=None: rng.uniform(*RANGES[name], size=size)
    sigma = np.float32(u("blur_sigma"))
    p["blur_sigma"], p["blur_w"] = sigma, gaussian_taps(float(sigma))
    p["noise_scale"], p["dropout_p"] = u("noise_scale"), u("dropout_p")
    m, c = u("multiply", 3), u("contrast", 3)
    p["multiply"] = m if pc[MULTIPLY] else m[0]
    p["contrast"] = c if pc[CONTRAST] else c[0]
    p["gray_alpha"], p["elastic_alpha"] = u("gray_alpha"), u("elastic_alpha")
    if sigma < 1e-3:                        # imgaug skips such a blur
        active[BLUR] = False
    p["active"] = sum(1 << o for o in range(NUM_OPS) if active[o])
    p["per_channel"] = sum(1 << o for o in (NOISE, DROPOUT, MULTIPLY, CONTRAST) if pc[o])
    return p


# ------------------------------------------------------------------------------------------------------------ the ops in NumPy
_f = np.float32


def _round_clip(v):
    return np.clip(np.rint(v), 0, 255).astype(np.float32)


def _reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def _smooth5(a, wts):
    """The separable 5-tap filter of a float32 (H, W, ...) array: horizontal pass, then vertical, reflect-101, taps summed in order."""
    h, w = a.shape[:2]
    xs = [_reflect101(np.arange(w) + t - 2, w) for t in range(5)]
    ys = [_reflect101(np.arange(h) + t - 2, h) for t in range(5)]
    hp = wts[0] * a[:, xs[0]]
    for t in range(1, 5):
        hp = hp + wts[t] * a[:, xs[t]]
    out = wts[0] * hp[ys[0]]
    for t in range(1, 5):
        out = out + wts[t] * hp[ys[t]]
    return out


def _cubic(t):
    t1, t2 = t + _f(1), _f(1) - t
    w0 = ((_f(-0.75) * t1 + _f(3.75)) * t1 - _f(6)) * t1 + _f(3)
    w1 = ((_f(1.25) * t - _f(2.25)) * t) * t + _f(1)
    w2 = ((_f(1.25) * t2 - _f(2.25)) * t2) * t2 + _f(1)
    return [w0, w1, w2, ((_f(1) - w0) - w1) - w2]


def _gauss(a, b):
    return np.sqrt(_f(-2) * np.log(_uniform_open(a))) * np.cos(_f(6.2831854820251465) * _uniform(b))


def _apply(op, v, rec, seed):
    """One op on a float32 (H, W, 3) image of integer values; returns the same."""
    h, w = v.shape[:2]
    if op == BLUR:
        return _round_clip(_smooth5(v, rec["blur_w"]))
    if op == NOISE:
        q = _pixel_words(h, w, rec, NOISE, 0, seed)
        z = _gauss(q[0], q[1])[..., None]
        if rec["per_channel"] >> NOISE & 1:
            q1 = _pixel_words(h, w, rec, NOISE, 1, seed)
            z = np.stack([z[..., 0], _gauss(q[2], q[3]), _gauss(q1[0], q1[1])], axis=-1)
        return _round_clip(v + rec["noise_scale"] * z)
    if op == DROPOUT:
        q = _pixel_words(h, w, rec, DROPOUT, 0, seed)
        u = np.stack([_uniform(q[c]) for c in range(3)], axis=-1) if rec["per_channel"] >> DROPOUT & 1 else _uniform(q[0])[..., None]
        return np.where(u < rec["dropout_p"], _f(0), v)
    if op == MULTIPLY:      # (float64: exact, see the module header)
        return _round_clip(v.astype(np.float64) * rec["multiply"].astype(np.float64))
    if op == CONTRAST:
        return _round_clip(128.0 + rec["contrast"].astype(np.float64) * (v.astype(np.float64) - 128.0))
    if op == GRAYSCALE:
        i = v.astype(np.int64)
        g = ((4899 * i[..., 0] + 9617 * i[..., 1] + 1868 * i[..., 2] + 8192) >> 14).astype(np.float32)[..., None]
        return _round_clip(v + rec["gray_alpha"] * (g - v))
    if op == ELASTIC:
        q = _pixel_words(h, w, rec, ELASTIC, 0, seed)
        raw = np.stack([_f(2) * _uniform(q[0]) - _f(1), _f(2) * _uniform(q[1]) - _f(1)], axis=-1)
        d = _smooth5(raw, rec["field_w"]) * rec["elastic_alpha"]
        y, x = np.mgrid[0:h, 0:w]
        sx, sy = x.astype(np.float32) - d[..., 0], y.astype(np.float32) - d[..., 1]
        fx, fy = np.floor(sx), np.floor(sy)
        wx, wy = _cubic(sx - fx), _cubic(sy - fy)
        ix, iy = fx.astype(np.int64) - 1, fy.astype(np.int64) - 1
        padded = np.zeros((h + 2, w + 2, 3), np.float32)      # a ring of zeros: every tap outside the image lands on it
        padded[1:-1, 1:-1] = v
        out = None
        for j in range(4):
            yy = np.clip(iy + j, -1, h) + 1
            row = None
            for t in range(4):
                xx = np.clip(ix + t, -1, w) + 1
                term = wx[t][..., None] * padded[yy, xx]
                row = term if row is None else row + term
            term = wy[j][..., None] * row
            out = term if out is None else out + term
        return _round_clip(out)
    raise ValueError(f"op {op}")


def augment_numpy(images, params: np.ndarray, seed: int) -> np.ndarray:
    """The specification in NumPy: images (B, H, W, 3) uint8 (array or CPU tensor) -> the augmented uint8 array.  This is what
    `--device cpu` trains with and what the kernel is tested against."""
    images = images.numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
        raise ValueError(f"images: expected (B, H, W, 3) uint8, got {images.dtype} {images.shape}")
    params = check_params(params, images.shape[0])
    out = images.copy()
    for b in range(images.shape[0]):
        rec = params[b]
        ops_ = [int(o) for o in rec["order"] if rec["active"] >> int(o) & 1]
        if not ops_:
            continue
        v = images[b].astype(np.float32)
        for op in ops_:
            v = _apply(op, v, rec, seed)
        out[b] = v.astype(np.uint8)
    return out


class Augmenter:
    """augment(prob) of the reference for batches of uint8 images: on a cuda tensor the HIP kernel (one launch per batch), on a
    CPU tensor `augment_numpy`; both from the same host-drawn records, so the two agree (bit for bit except noise's rounding ties).
    rank / world: every rank draws its own sample ids (rank + world * k); stream_tag separates streams that share sample ids
    (train_bra's wide and telephoto images)."""

    def __init__(self, prob=0.5, seed=2021, rank=0, world=1, stream_tag=0):
        if not 0.0 <= prob <= 1.0:
            raise ValueError(f"prob {prob} outside [0, 1]")
        self.prob, self.seed, self.rank, self.world, self.stream_tag = float(prob), int(seed), int(rank), int(world), int(stream_tag)
        self.count = 0          # images this Augmenter has drawn records for

    def draw(self, n: int) -> np.ndarray:
        """The parameter table of the next n samples."""
        ids = self.rank + self.world * (self.count + np.arange(n))
        self.count += n
        if n == 0:
            return np.zeros(0, PARAMS_DTYPE)
        return np.concatenate([draw_sample(self.prob, self.seed, int(i), self.stream_tag) for i in ids])

    def __call__(self, images: torch.Tensor, params: np.ndarray = None) -> torch.Tensor:
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
            raise ValueError(f"images: expected (B, H, W, 3) uint8, got {images.dtype} {tuple(images.shape)}")
        params = self.draw(images.shape[0]) if params is None else params
        if not params["active"].any():
            return images
        if images.is_cuda:
            from .. import ops
            return ops.augment_u8(images, params, self.seed)
        return torch.from_numpy(augment_numpy(images, params, self.seed))
