"""Exactly representable data for the convolution kernels (tests/test_conv_exact_host.py, tests/test_gpu_conv_exact.py).

csrc/split_arith.hpp says which partial products each precision keeps (f32: all; bf16x6: a0b0 a0b1 a1b0 a0b2 a2b0 a1b1; f16x3: a0b0 a0b1
a1b0 under power-of-two scales) and that they are accumulated in fp32.  When the operands put all of their information into kept
products and every partial sum is representable, the float64 result is the ONLY correct answer - whatever the dispatch, the tiling, the
split-K plan or the hand-off - and a kernel must return it bit for bit.  This module makes such data, checks that it is such data
(`preconditions`), and restates the specification in torch (`Emulator`: for the host test only; the GPU tests compare with float64).

Data classes (seeded generators):
  A   dense small integers on both sides: every k index and every tap contributes (indexing, halos, borders, strides, windows, split-K).
  B   f16x3: activations 2^e (H0 + H1) - H0 an 11-bit value, H1 below half of H0's quantum with 10 more bits, one pinned element
      that is the tensor's maximum - against one tap +-2^k per output channel: a0 and a1 must both arrive.
  D   the same for f32 / bf16x6 with full fp32 patterns.  Precondition 1 gives one of fp32's 24 bits to the piece products (the
      first bf16 piece can round up to the next power of two, and a0 + a2 then spans 25 bits), so the patterns carry 23
      significant bits: N(0, 1) values with the last mantissa bit cleared.  All of a0, a1, a2 are still needed.
  C   the mirror image: activations +- powers of two, one nonzero weight per output channel carrying the pattern (two fp16 pieces
      under the weight tensor's scale, whose maximum is channel 0's tap; 23 bits for f32 / bf16x6).
  E   f32 / bf16x6 only (f16x3 drops a1 b1 by design): both sides +-(2^p +- 2^(p-9-j)), two bf16 pieces of one bit
      each, the weights one tap per output channel - the one kept product none of B, D, C needs, a1 b1, must arrive.
  R   runs and chains (intermediate maps never leave the kernel): sparse ternary weights (at most 4 nonzeros per output channel: at
      most 4x growth per layer) or one-tap weights (no growth), folded BatchNorm scale a power of two, shift a small integer.

A case is an object with `forward(mul)`: the operation in float64 torch with every matrix product routed through `mul(op, a, b)`
(op bilinear) and every epilogue value shown to `mul.see`.  Plain() gives the float64 reference, Emulator() the specification,
Recorder() what `preconditions` inspects, the Fault* classes the arithmetic faults of the sensitivity checks."""
from __future__ import annotations

import math
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

F32, BF16X6, F16X3 = "f32", "bf16x6", "f16x3"
PRECISIONS = (F32, BF16X6, F16X3)
# split_arith.hpp: which (piece of a, piece of b) products are kept
KEPT = {F32: ((0, 0),), BF16X6: ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)), F16X3: ((0, 0), (0, 1), (1, 0))}
NPIECES = {F32: 1, BF16X6: 3, F16X3: 2}
BOUND_BITS = 2            # a handed-in bound may be 4x above the true maximum
MIN_HEADROOM_BITS = 10    # what must stay between the smallest fp16 piece bit and fp16's subnormal quantum 2^-24 under such a bound


# ---------------------------------------------------------------------------------------------- bits
def low_bit_exp(t: torch.Tensor) -> torch.Tensor:
    """Exponent of the lowest set bit of every NONZERO element of a float64 tensor (1-d result; remembered on the tensor object)."""
    memo = getattr(t, "_low_bit_exp", None)
    if memo is not None and memo[0] == t._version:
        return memo[1]
    t._low_bit_exp = (t._version, _low_bit_exp(t))
    return t._low_bit_exp[1]


def _low_bit_exp(t):
    v = t[t != 0].double().abs()
    m, e = torch.frexp(v)                                   # v = m 2^e, m in [0.5, 1)
    mi = (m * float(1 << 53)).to(torch.int64)
    low = mi & -mi
    _, le = torch.frexp(low.double())                       # low = 2^(le - 1)
    return e.to(torch.int64) - 53 + (le.to(torch.int64) - 1)


def odd_part_max(t: torch.Tensor) -> float:
    """The largest |element| / (its lowest set bit): what an element is in units of its own quantum."""
    v = t[t != 0].double().abs()
    return float((v / torch.exp2(low_bit_exp(t).double())).max()) if v.numel() else 0.0


def quantum(t: torch.Tensor) -> float:
    """The largest power of two that divides every element (1.0 for an all-zero tensor)."""
    le = low_bit_exp(t)
    return math.ldexp(1.0, int(le.min())) if le.numel() else 1.0


def scale_of(m: float) -> float:
    """f16_scale_of: the power of two that puts m into [16384, 32768); exponent floored at -100; 1 for m = 0."""
    m = float(np.float32(m))
    if not m > 0.0:
        return 1.0
    _, e = math.frexp(m)
    return math.ldexp(1.0, max(e, -100) - 15)


def finite_max(t: torch.Tensor) -> float:
    return float(t.abs().max()) if t.numel() else 0.0


_pieces_memo: dict = {}


def pieces(t: torch.Tensor, precision: str, scale: float | None = None):
    """The pieces of a float64 tensor of fp32 values as split_arith.hpp words them, in the tensor's own units (float64).  The last few
    results are remembered by tensor object (the host test splits the same operand many times)."""
    if precision == F16X3 and scale is None:
        scale = scale_of(finite_max(t))
    key = (id(t), t._version, precision, scale)
    hit = _pieces_memo.get(key)
    if hit is None:
        if sum(v[0].numel() * len(v[1]) for v in _pieces_memo.values()) + t.numel() * NPIECES[precision] > 60_000_000:
            _pieces_memo.clear()
        hit = _pieces_memo[key] = (t, _pieces(t, precision, scale))       # (t itself is kept: its id stays its own)
        for p in hit[1]:
            p._any = bool(p.any())
    return list(hit[1])


def nonzero(p) -> bool:
    """Whether a piece has a nonzero element (remembered for the pieces `pieces` made)."""
    return p._any if hasattr(p, "_any") else bool(p.any())


def _pieces(t, precision, scale):
    t32 = t.float()
    if precision == F32:
        return [t32.double()]
    if precision == BF16X6:
        p0 = t32.bfloat16().float()
        r1 = t32 - p0
        p1 = r1.bfloat16().float()
        p2 = (r1 - p1).bfloat16().float()
        return [p0.double(), p1.double(), p2.double()]
    s = scale
    u = t32 / s
    h0 = u.half().float()
    h1 = (u - h0).half().float()
    return [h0.double() * s, h1.double() * s]


# ---------------------------------------------------------------------------------------------- products
class Plain:
    """The float64 reference."""

    def __call__(self, op, a, b):
        return op(a, b)

    def see(self, t):
        return t


class Recorder(Plain):
    def __init__(self):
        self.products, self.seen = [], []

    def __call__(self, op, a, b):
        out = op(a, b)
        self.products.append((op, a, b, out))
        return out

    def see(self, t):
        self.seen.append(t)
        return t


class Emulator(Plain):
    """split_arith.hpp in torch: the pieces (round to nearest), the kept products only, float64 products and sums.  `drop`: one kept
    product left out (a fault for the sensitivity checks); `bound`: the factor a handed-in activation bound is above the maximum."""

    def __init__(self, precision, drop=None, bound=1.0):
        self.precision, self.drop, self.bound = precision, drop, bound

    def __call__(self, op, a, b):
        sa = scale_of(finite_max(a) * self.bound) if self.precision == F16X3 else None
        pa, pb = pieces(a, self.precision, sa), pieces(b, self.precision)
        out = None
        for i, j in KEPT[self.precision]:
            if (i, j) == self.drop or not nonzero(pa[i]) or not nonzero(pb[j]):
                continue
            term = op(pa[i], pb[j])
            out = term if out is None else out + term
        return op(a, b) * 0.0 if out is None else out


class FaultShiftedTap(Plain):
    """Every weight tensor read one tap (or, for a single tap, one input channel) further."""

    def __call__(self, op, a, b):
        dim = -1 if b.shape[-1] > 1 else (-2 if b.shape[-2] > 1 else 1)
        return op(a, torch.roll(b, 1, dims=dim))


class FaultLastKBlock(Plain):
    """The last block of k (input channels: 16, or one where there are fewer than 32) never added."""

    def __call__(self, op, a, b):
        a = a.clone()
        a[:, -(16 if a.shape[1] >= 32 else 1):] = 0
        return op(a, b)


class FaultHaloColumn(Plain):
    """One column of every map a product reads taken as zero: column 16 (a tile edge), or the first one of a narrower map."""

    def __call__(self, op, a, b):
        a = a.clone()
        a[..., 16 if a.shape[-1] > 16 else 0] = 0
        return op(a, b)


# ---------------------------------------------------------------------------------------------- preconditions
def _check_fp32(t, what):
    t = t.double()
    mag = t.abs()
    assert float(mag.max()) < float("inf"), f"precondition 3 ({what}): not finite"           # (NaN fails the next line)
    assert torch.equal(t.float().double(), t), f"precondition 3 ({what}): a value is not an fp32 number"
    smallest = float(torch.where(mag == 0, torch.full_like(mag, float("inf")), mag).min())
    assert smallest >= 2.0 ** -126, f"precondition 3 ({what}): an fp32 subnormal"


def _check_budget(op, a, b, qa, qb, what, max_terms=None):
    """1: all terms of an output are multiples of q and sum |a||b| < 2^23 q - with one global quantum q = qa qb (from the number of terms
    of an output and the largest factors where that suffices, else from sum |a||b| itself), or, where every output has a single term,
    per term (each factor in units of its own lowest bit)."""
    q = qa * qb
    terms = float(max_terms(a, b)) if max_terms is not None else float(op((a != 0).double(), (b != 0).double()).max())
    if terms * finite_max(a) * finite_max(b) < 2.0 ** 23 * q:
        return
    if terms <= 1.0:
        big = odd_part_max(a) * odd_part_max(b)        # |a||b| / (low bit of a x low bit of b), at most
        assert big < 2.0 ** 23, f"precondition 1 ({what}): a single term of {big:.6g} >= 2^23 times its own quantum"
        return
    mag = float(op(a.abs(), b.abs()).max())
    assert mag < 2.0 ** 23 * q, f"precondition 1 ({what}): sum|a||b| {mag:.6g} >= 2^23 q, q = {q:.6g}, with up to {terms:.0f} terms per output"


def _check_pieces(a, b, qa, qb, precision, what):
    """2: both operands are the exact sum of their pieces under the scale f16_scale_of derives from the true maximum (and under a
    bound 4x above it for the activations), and no dropped product has both factors nonzero.  Returns the fp16 headroom in bits: how
    far the lowest bit of a scaled operand (its quantum over the scale: the second piece's lowest bit) stays above fp16's subnormal
    quantum 2^-24 under such a bound."""
    headroom = None
    pa, pb = pieces(a, precision), pieces(b, precision)
    assert torch.equal(sum(pa), a.double()) and torch.equal(sum(pb), b.double()), f"precondition 2 ({what}): the pieces do not sum to the operand"
    for i in range(NPIECES[precision]):
        for j in range(NPIECES[precision]):
            if (i, j) not in KEPT[precision]:
                assert not (nonzero(pa[i]) and nonzero(pb[j])), f"precondition 2 ({what}): the dropped product a{i} b{j} is not zero"
    if precision == F16X3:
        sa, sb = scale_of(finite_max(a)) * 2.0 ** BOUND_BITS, scale_of(finite_max(b))
        assert torch.equal(sum(pieces(a, precision, sa)), a.double()), f"precondition 2 ({what}): not two fp16 pieces under a bound {2 ** BOUND_BITS}x above the maximum"
        headroom = int(min(math.log2(qa / sa), math.log2(qb / sb))) + 24
        assert headroom >= MIN_HEADROOM_BITS, f"precondition 2 ({what}): {headroom} bits above fp16's subnormal quantum"
    return headroom


def preconditions(case, precisions):
    """Asserts the three preconditions on the float64 chain of `case` for every precision of `precisions` (one name or several);
    returns (the float64 result, the smallest fp16 headroom in bits or None).  A case that fails here is a broken test, not a
    tolerance to widen."""
    if isinstance(precisions, str):
        precisions = (precisions,)
    rec = Recorder()
    final = case.forward(rec)
    headroom = None
    for n, (op, a, b, out) in enumerate(rec.products):
        what = f"{case.name}, product {n}"
        _check_fp32(a, what + ", a"); _check_fp32(b, what + ", b"); _check_fp32(out, what + ", result")
        qa, qb = quantum(a), quantum(b)
        _check_budget(op, a, b, qa, qb, what, getattr(case, "max_terms", None))
        for precision in precisions:
            h = _check_pieces(a, b, qa, qb, precision, f"{what}, {precision}")
            headroom = h if headroom is None else (headroom if h is None else min(h, headroom))
    for n, t in enumerate(rec.seen):
        _check_fp32(t, f"{case.name}, epilogue value {n}")
    if not (rec.products and final is rec.products[-1][3]):
        _check_fp32(final, case.name + ", result")
    return final, headroom


# ---------------------------------------------------------------------------------------------- generators
def rng_of(*key):
    return np.random.Generator(np.random.PCG64(zlib.crc32(repr(key).encode())))


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def integers(rng, shape, bound):
    return t64(rng.integers(-bound, bound + 1, size=shape))


def signs(rng, shape):
    return rng.integers(0, 2, size=shape) * 2.0 - 1.0


def pow2(rng, shape, lo=-3, hi=3):
    """Dense +- powers of two."""
    return t64(signs(rng, shape) * np.exp2(rng.integers(lo, hi + 1, size=shape)))


def pattern23(rng, shape):
    """N(0, 1) in fp32 with the last mantissa bit cleared: 23 significant bits, all three bf16 pieces in use."""
    v = rng.standard_normal(shape).astype(np.float32)
    v = (v.view(np.uint32) & np.uint32(0xFFFFFFFE)).view(np.float32)
    return t64(v)


def pattern_two_fp16(rng, shape, e=-20, pin=True):
    """+- 2^e (H0 + H1) 2^j: H0 = m 2^10 with 11-bit m, |H1| <= 511 < half of H0's quantum, j in {0, 1}; the first element pinned to the maximum."""
    m = rng.integers(1024, 2048, size=shape)
    r = rng.integers(-511, 512, size=shape)
    j = rng.integers(0, 2, size=shape)
    v = signs(rng, shape) * (m * 1024 + r) * np.exp2(j + e)
    if pin:
        v.reshape(-1)[0] = (2047 * 1024 + 511) * 2.0 ** (1 + e)
    return t64(v)


def pattern_two_bf16(rng, shape, lo=-3, hi=3):
    """+-(2^p +- 2^(p - 9 - j)), j in {0, 1, 2}: the first bf16 piece is 2^p, the second the small term, the third zero."""
    p = rng.integers(lo, hi + 1, size=shape)
    j = rng.integers(0, 3, size=shape)
    return t64(signs(rng, shape) * (np.exp2(p) + signs(rng, shape) * np.exp2(p - 9 - j)))


def one_tap(rng, wshape, out_dim, values):
    """A weight tensor with exactly one nonzero element per output channel (dimension out_dim), at a random place of that channel's block;
    values: one per output channel (channel 0 first)."""
    w = np.zeros(wshape)
    wv = np.moveaxis(w, out_dim, 0)                     # a view of w, output channel first
    n, block = wshape[out_dim], wv[0].size
    out = np.zeros((n, block))
    out[np.arange(n), rng.integers(0, block, size=n)] = np.asarray(values, dtype=np.float64).reshape(-1)
    wv[...] = out.reshape(wv.shape)
    return t64(w)


def sparse_ternary(rng, wshape, out_dim, nnz=4):
    """+-1 at up to nnz random places of every output channel's block, zero elsewhere."""
    w = np.zeros(wshape)
    wv = np.moveaxis(w, out_dim, 0)
    n, block = wshape[out_dim], wv[0].size
    out = np.zeros((n, block))
    for _ in range(nnz):
        out[np.arange(n), rng.integers(0, block, size=n)] = signs(rng, n)
    wv[...] = out.reshape(wv.shape)
    return t64(w)


def pow2_bn(rng, ch, scales=(0.5, 1.0), shift_bound=2, zero_shift=False):
    """BatchNorm statistics that fold to scale in `scales` (powers of two) and an integer or half-integer shift, with eps = 0:
    (mean, var, gamma, beta) in float32, and the folded (scale, shift) in float64.  var = 4: its square root is exact."""
    scale = np.asarray(scales)[rng.integers(0, len(scales), size=ch)]
    mean = np.zeros(ch) if zero_shift else rng.integers(-1, 2, size=ch).astype(np.float64)
    beta = np.zeros(ch) if zero_shift else rng.integers(-shift_bound, shift_bound + 1, size=ch).astype(np.float64)
    var = np.full(ch, 4.0)
    gamma = scale * 2.0
    bn = tuple(torch.from_numpy(v.astype(np.float32)) for v in (mean, var, gamma, beta))
    return bn, t64(scale), t64(beta - mean * scale)


def affine(y, scale, shift):
    return y * scale[None, :, None, None] + shift[None, :, None, None]


# ---------------------------------------------------------------------------------------------- ops.ConvLayer
ConvGeom = namedtuple("ConvGeom", "name B cin cout kh kw stride ph pw dh dw transposed out_pad H W force force_precisions")


def conv_geometries(own_batch=False):
    """The geometries of tests/test_gpu_conv.py's case lists (CASES, F16_CASES, TAP_PAIR_CASES, DIRECT_CASES, the small-cin cases), each
    once, at batch 2.  own_batch=True: F16_CASES' single images and DIRECT_CASES at their own batches (1 ... 7) - the plan search counts
    the pixels of the whole batch, so the batch decides between the direct and the split kernel there; TAP_PAIR_CASES' plans are
    pinned and the small-cin kernel is chosen by the channel count, whatever the batch.  A pinned plan (LAV_SPLIT_FORCE) goes
    with the precisions that list runs it at: F16_CASES' with f16x3, TAP_PAIR_CASES' with bf16x6; every other launch takes the plan
    search's choice."""
    from tests import test_gpu_conv as T
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    out = {}

    def add(name, B, cin, cout, k, s, p, d, tr, op, H, W, force="", precision=None):
        if own_batch and (B == 2 or not (name.startswith("direct: ") or (name.startswith("f16: ") and B == 1))):
            return
        (kh, kw), (ph, pw), (dh, dw) = pair(k), pair(p), pair(d)
        key = (B if own_batch else 2, cin, cout, kh, kw, s, ph, pw, dh, dw, bool(tr), op, H, W, force)
        old = out.get(key)
        fp = tuple(sorted(set(old.force_precisions if old else ()) | ({precision} if force else set())))
        out[key] = ConvGeom(old.name if old else name + (f" (batch {B})" if own_batch else ""), *key, fp)
    for name, cin, cout, k, s, p, d, tr, op, H, W in T.CASES:
        add(name, 2, cin, cout, k, s, p, d, tr, op, H, W)
    for name, B, cin, cout, k, s, p, tr, op, H, W, force in T.F16_CASES:
        add("f16: " + name, B, cin, cout, k, s, p, 1, tr, op, H, W, force, F16X3)
    for name, B, cin, cout, k, s, p, H, W, force in T.TAP_PAIR_CASES:
        add("tap pairs: " + name, B, cin, cout, k, s, p, 1, False, 0, H, W, force, BF16X6)
    for name, B, cin, cout, k, s, p, d, H, W in T.DIRECT_CASES:
        add("direct: " + name, B, cin, cout, k, s, p, d, False, 0, H, W)
    for cin, k, cout, B, H, W in T.SMALL_CIN_CASES:
        add(f"small cin: {k}x{k} s2 {cin}->{cout} {H}x{W}", B, cin, cout, k, 2, k // 2, 1, False, 0, H, W)
    return list(out.values())


def conv_classes(precision):
    """The data classes a precision runs: name -> generator key."""
    return {"A": "A", "B": "B", "C": "C16"} if precision == F16X3 else {"A": "A", "D": "D", "C": "C24", "E": "E"}


EPILOGUES = ("none", "bias", "relu_affine_windows", "affine_residual_relu")


_conv_memo: dict = {}


def _content_key(t):
    memo = getattr(t, "_content_key", None)
    if memo is None or memo[0] != t._version:
        memo = t._content_key = (t._version, zlib.adler32(t.contiguous().numpy()))
    return memo[1]


class ConvLayerCase:
    """One ops.ConvLayer launch: geometry g, data class key, epilogue.  Attributes are what the layer is built from (float32 tensors);
    x is the full input (its channel window is x[:, in_off:in_off + cin])."""

    def __init__(self, g: ConvGeom, key: str, epilogue: str = "none", batch: int | None = None):
        assert epilogue == "none" or key == "A", "additive epilogues are exact on integers only"
        self.g, self.key, self.epilogue = g, key, epilogue
        self.name = f"{g.name} / class {key} / {epilogue}"
        rng = rng_of("conv", tuple(g), key)
        B = batch or g.B
        xs = (B, g.cin, g.H, g.W)
        ws = (g.cin, g.cout, g.kh, g.kw) if g.transposed else (g.cout, g.cin, g.kh, g.kw)
        od = 1 if g.transposed else 0
        K = g.cin * g.kh * g.kw
        if key == "A":
            ax, aw = (7, 3) if K <= 4608 else (2, 2)
            x, w = integers(rng, xs, ax), integers(rng, ws, aw)
        elif key == "B":
            x, w = pattern_two_fp16(rng, xs), one_tap(rng, ws, od, signs(rng, g.cout) * np.exp2(rng.integers(-3, 4, size=g.cout)))
        elif key == "D":
            x, w = pattern23(rng, xs), one_tap(rng, ws, od, signs(rng, g.cout) * np.exp2(rng.integers(-3, 4, size=g.cout)))
        elif key == "C24":
            x, w = pow2(rng, xs), one_tap(rng, ws, od, pattern23(rng, (g.cout,)).numpy())
        elif key == "E":
            x, w = pattern_two_bf16(rng, xs), one_tap(rng, ws, od, pattern_two_bf16(rng, (g.cout,)).numpy())
        elif key == "C16":
            x, w = pow2(rng, xs), one_tap(rng, ws, od, pattern_two_fp16(rng, (g.cout,), e=-12).numpy())
        else:
            raise KeyError(key)
        self.w = w.float()
        self._ab = None
        self.in_off = self.out_off = 0
        self.in_total, self.out_total = g.cin, g.cout
        self.bias = self.bn = self.residual = None
        self.relu_pre = self.relu_post = False
        self._scale = self._shift = None
        if epilogue != "none":
            self.bias = integers(rng, (g.cout,), 3).float()
        if epilogue == "relu_affine_windows":
            self.in_off, self.in_total, self.out_off, self.out_total = 8, g.cin + 16, 8, g.cout + 16
            full = integers(rng, (B, self.in_total, g.H, g.W), 7)          # the channels beside the window hold other integers
            full[:, 8:8 + g.cin] = x
            x = full
            self.relu_pre = True
        if epilogue in ("relu_affine_windows", "affine_residual_relu"):
            self.bn, self._scale, self._shift = pow2_bn(rng, g.cout, scales=(0.5, 1.0, 2.0))
        self.x = x.float()
        if epilogue == "affine_residual_relu":
            self.relu_post = True
            oh, ow = self.out_hw()
            self.residual = integers(rng, (B, g.cout, oh, ow), 7).float()

    def out_hw(self):
        g = self.g
        if g.transposed:
            f = lambda n, k, p: (n - 1) * g.stride - 2 * p + k + g.out_pad
            return f(g.H, g.kh, g.ph), f(g.W, g.kw, g.pw)
        f = lambda n, k, p, d: (n + 2 * p - d * (k - 1) - 1) // g.stride + 1
        return f(g.H, g.kh, g.ph, g.dh), f(g.W, g.kw, g.pw, g.dw)

    def max_terms(self, a, b):
        """Terms of an output: at most the nonzero weights of its output channel."""
        return int((b != 0).sum(dim=(0, 2, 3) if self.g.transposed else (1, 2, 3)).max())

    def op(self, a, b, dense=False):
        """The convolution in float64.  One-tap weights (at most one nonzero per output channel) take a short cut with the same terms:
        every output channel's input channel is gathered and convolved on its own (test_conv_exact_host.py compares the two).  Results
        are remembered by the operands' contents: the host test asks for the same product many times (a class-A piece IS the operand)."""
        g = self.g
        oh, ow = self.out_hw()
        if 2.0 * a.shape[0] * oh * ow * b.numel() < 3e8:                  # cheaper than hashing its operands
            return self._conv(a, b, dense)
        key = (tuple(g), dense, tuple(a.shape), _content_key(a), _content_key(b))
        if _conv_memo and next(iter(_conv_memo))[0] != key[0]:
            _conv_memo.clear()                                            # one geometry at a time
        if key not in _conv_memo:
            _conv_memo[key] = self._conv(a, b, dense)
        return _conv_memo[key]

    def _conv(self, a, b, dense):
        g = self.g
        bt = b.transpose(0, 1) if g.transposed else b                     # output channel first
        if not dense and bt.shape[1] >= 16 and int((bt != 0).sum(dim=(1, 2, 3)).max()) <= 1:
            ci = (bt != 0).any(dim=3).any(dim=2).double().argmax(dim=1)
            a, b = a[:, ci], bt[torch.arange(bt.shape[0]), ci][:, None]   # (B, cout, H, W), (cout, 1, kh, kw)
            if g.transposed:
                return F.conv_transpose2d(a, b, None, g.stride, (g.ph, g.pw), g.out_pad, groups=g.cout)
            return F.conv2d(a, b, None, g.stride, (g.ph, g.pw), (g.dh, g.dw), groups=g.cout)
        if g.transposed:
            return F.conv_transpose2d(a, b, None, g.stride, (g.ph, g.pw), g.out_pad)
        return F.conv2d(a, b, None, g.stride, (g.ph, g.pw), (g.dh, g.dw))

    def layer_kwargs(self):
        g = self.g
        kw = dict(stride=g.stride, padding=(g.ph, g.pw), dilation=(g.dh, g.dw), transposed=g.transposed, output_padding=g.out_pad, bias=self.bias,
                  bn=self.bn, bn_eps=0.0, relu_pre=self.relu_pre, relu_post=self.relu_post)
        if self.in_total != g.cin:
            kw.update(in_c_total=self.in_total, in_c_offset=self.in_off, out_c_total=self.out_total, out_c_offset=self.out_off)
        return kw

    def forward(self, mul):
        """The window of the output, float64: conv (+ bias) (-> ReLU) (-> affine) (+ residual) (-> ReLU), the C ABI's order."""
        if self._ab is None:
            self._ab = (self.x.double()[:, self.in_off:self.in_off + self.g.cin].contiguous(), self.w.double())
        y = mul(self.op, *self._ab)
        if self.bias is not None:
            y = mul.see(y + self.bias.double()[None, :, None, None])
        if self.relu_pre:
            y = F.relu(y)
        if self.bn is not None:
            y = mul.see(affine(y, self._scale, self._shift))
        if self.residual is not None:
            y = mul.see(y + self.residual.double())
        if self.relu_post:
            y = F.relu(y)
        return y


# ---------------------------------------------------------------------------------------------- class R: runs, tile runs, pairs, chains
RUN_GEOMS = [(64, 37, 53, 2), (128, 40, 40, 5), (128, 80, 80, 5)]          # ops.ConvRun: C, H, W, L
TILE_GEOMS = [(5, 7, 3), (9, 17, 3), (37, 53, 2), (37, 53, 3), (16, 32, 1)]   # ops.ConvTileRun at 64 channels: H, W, L
R_KINDS = ("ternary", "one_tap")


def r_weights(rng, shape, kind):
    if kind == "ternary":
        return sparse_ternary(rng, shape, 0, 4)
    return one_tap(rng, shape, 0, signs(rng, shape[0]))


class RunCase:
    """L layers conv3x3 (no bias) -> ReLU -> affine at C channels on one (1, C, H, W) map of integers in [-7, 7]."""

    def __init__(self, C, H, W, L, kind):
        self.name = f"run C {C} {H}x{W} L {L} / class R {kind}"
        rng = rng_of("run", C, H, W, L, kind)
        self.x = integers(rng, (1, C, H, W), 7).float()
        self.layers = []          # (weight f32, bn tuple, scale f64, shift f64)
        for _ in range(L):
            bn, scale, shift = pow2_bn(rng, C)
            self.layers.append((r_weights(rng, (C, C, 3, 3), kind).float(), bn, scale, shift))

    def forward(self, mul):
        y = self.x.double()
        for w, _, scale, shift in self.layers:
            y = mul.see(affine(F.relu(mul(lambda a, b: F.conv2d(a, b, None, 1, 1), y, w.double())), scale, shift))
        return y


PAIR_GEOMS = [(128, 36, 32, 1), (128, 36, 32, 2), (128, 36, 32, 16)]             # ops.Conv1dPair: C, H, W, dilation (with and without the residual)
CHAIN_GEOMS = [(128, 36, 32, (2, 4, 8, 16)), (64, 20, 64, (1, 3))]                # ops.Conv1dPairChain: blocks of (undilated pair, dilated pair + block input)


class PairsCase:
    """Conv1dPair layers one after the other on a (2, C, H, W) map: conv3x1 + bias -> ReLU -> conv1x3 + bias -> affine (-> + the input of
    the pair before, where flagged; `own_residual`: + the pair's own input, the single launch's residual) -> ReLU.  dils: (d_a, d_b) per pair."""

    def __init__(self, C, H, W, dils, residual, kind, own_residual=False, B=2):
        self.name = f"pairs C {C} {H}x{W} dilations {dils} residual {residual or own_residual} / class R {kind}"
        rng = rng_of("pairs", C, H, W, tuple(dils), tuple(residual), kind, own_residual)
        self.C, self.dils, self.residual, self.own_residual = C, list(dils), list(residual), own_residual
        self.x = integers(rng, (B, C, H, W), 7).float()
        self.pairs = []          # (wa, ba, wb, bb, bn tuple, scale, shift)
        for _ in dils:
            bn, scale, shift = pow2_bn(rng, C)
            self.pairs.append((r_weights(rng, (C, C, 3, 1), kind).float(), integers(rng, (C,), 1).float(),
                               r_weights(rng, (C, C, 1, 3), kind).float(), integers(rng, (C,), 1).float(), bn, scale, shift))

    def forward(self, mul):
        ins = [self.x.double()]
        for (wa, ba, wb, bb, _, scale, shift), (da, db), res in zip(self.pairs, self.dils, self.residual):
            x = ins[-1]
            mid = F.relu(mul.see(mul(lambda a, b: F.conv2d(a, b, None, 1, (da, 0), (da, 1)), x, wa.double()) + ba.double()[None, :, None, None]))
            y = mul.see(mul(lambda a, b: F.conv2d(a, b, None, 1, (0, db), (1, db)), mid, wb.double()) + bb.double()[None, :, None, None])
            y = mul.see(affine(y, scale, shift))
            if res:
                y = mul.see(y + ins[-2])
            elif self.own_residual:
                y = mul.see(y + x)
            ins.append(F.relu(y))
        return ins[-1]


def pair_case(C, H, W, d, with_res, kind):
    return PairsCase(C, H, W, [(d, d)], [False], kind, own_residual=with_res)


def block_case(C, H, W, d, kind):
    """One non_bottleneck_1d block as a two-pair chain: the undilated pair, then the dilated one with the block's input added."""
    return PairsCase(C, H, W, [(1, 1), (d, d)], [False, True], kind)


def chain_case(C, H, W, dils, kind):
    d2, res = [], []
    for d in dils:
        d2 += [(1, 1), (d, d)]
        res += [False, True]
    return PairsCase(C, H, W, d2, res, kind)


# ---------------------------------------------------------------------------------------------- fp32 kernels: grouped deconv, pointwise upconv
DECONV_GEOMS = [((1, 2, 2, 4), 40, 37, 44, 2), ((3, 3), 16, 5, 4, 3)]        # ops.GroupedDeconv 3x3 stride 2 pad 1 out_pad 1: outs, cin per group, H, W, B
UPCONV_GEOMS = [(64, 128, 1, 0, 0, 9, 13), (128, 128, 4, 1, 2, 12, 10)]       # ops.PointwiseUpconv: cin, cout, k, pad, out_pad, H, W
FP32_CLASSES = ("A", "D", "C")


def _class_pair(rng, key, xs, ws, od, cout):
    if key == "A":
        return integers(rng, xs, 7), integers(rng, ws, 3)
    if key == "D":
        return pattern23(rng, xs), one_tap(rng, ws, od, signs(rng, cout) * np.exp2(rng.integers(-3, 4, size=cout)))
    return pow2(rng, xs), one_tap(rng, ws, od, pattern23(rng, (cout,)).numpy())


class DeconvCase:
    """ops.GroupedDeconv, identity epilogue: ConvTranspose2d(cin_g, o, 3, 2, 1, 1) per group on its own channels, + bias (integers in class A, else 0)."""

    def __init__(self, outs, cin_g, H, W, B, key):
        self.name = f"grouped deconv outs {outs} cin {cin_g} {H}x{W} B {B} / class {key}"
        rng = rng_of("deconv", tuple(outs), cin_g, H, W, B, key)
        self.outs, self.cin_g = outs, cin_g
        self.ws, self.biases = [], []
        xs = []
        for o in outs:
            x, w = _class_pair(rng, key, (B, cin_g, H, W), (cin_g, o, 3, 3), 1, o)
            xs.append(x); self.ws.append(w.float())
            self.biases.append((integers(rng, (o,), 3) if key == "A" else torch.zeros(o, dtype=torch.float64)).float())
        self.x = torch.cat(xs, dim=1).float()

    def forward(self, mul):
        ys = []
        for i, (w, b) in enumerate(zip(self.ws, self.biases)):
            y = mul(lambda a, b_: F.conv_transpose2d(a, b_, None, 2, 1, 1), self.x.double()[:, i * self.cin_g:(i + 1) * self.cin_g], w.double())
            ys.append(mul.see(y + b.double()[None, :, None, None]))
        return torch.cat(ys, dim=1)


class UpconvCase:
    """ops.PointwiseUpconv: ConvTranspose2d(cin, cout, k, k, pad, out_pad, no bias) -> ReLU -> affine (shift 0 outside class A)."""

    def __init__(self, cin, cout, k, pad, opad, H, W, key, B=2):
        self.name = f"pointwise upconv {cin}->{cout} k {k} pad {pad} out_pad {opad} {H}x{W} / class {key}"
        rng = rng_of("upconv", cin, cout, k, pad, opad, H, W, key)
        self.geom = (cin, cout, k, pad, opad)
        x, w = _class_pair(rng, key, (B, cin, H, W), (cin, cout, k, k), 1, cout)
        self.x, self.w = x.float(), w.float()
        self.bn, self.scale, self.shift = pow2_bn(rng, cout, scales=(0.5, 1.0, 2.0), zero_shift=key != "A")

    def forward(self, mul):
        cin, cout, k, pad, opad = self.geom
        y = mul(lambda a, b: F.conv_transpose2d(a, b, None, k, pad, opad), self.x.double(), self.w.double())
        return mul.see(affine(F.relu(y), self.scale, self.shift))


# ---------------------------------------------------------------------------------------------- weight gradient
# B, cin, cout, H, W, stride (3x3, pad 1); a seventh entry is the kernel size k (pad k // 2): the 7x7 stride-2 stem, one ky per task
WGRAD_GEOMS = [(2, 64, 64, 20, 32, 1), (2, 64, 128, 20, 24, 2), (2, 64, 64, 24, 24, 2, 7)]


class WgradCase:
    """lav_conv_wgrad (bf16x6) / lav_conv_wgrad_amax (two fp16 pieces): dw = sum over (n, y, x) of dy * x.  Class A: integers on both sides.
    Class D (bf16 entry) / B (fp16 entry): dy has ONE nonzero element per output channel, +- a power of two, and x carries the pattern.
    k: the kernel size (k x k, pad k // 2)."""

    def __init__(self, B, cin, cout, H, W, stride, key, k=3):
        self.name = f"wgrad B {B} {cin}->{cout} {H}x{W} s{stride}{'' if k == 3 else f' k{k}'} / class {key}"
        self.geom = (B, cin, cout, H, W, stride)
        self.k = k
        rng = rng_of("wgrad", B, cin, cout, H, W, stride, key, *(() if k == 3 else (k,)))
        ys = (B, cout, H // stride, W // stride)
        if key == "A":
            x, dy = integers(rng, (B, cin, H, W), 7), integers(rng, ys, 3)
        else:
            x = pattern23(rng, (B, cin, H, W)) if key == "D" else pattern_two_fp16(rng, (B, cin, H, W))
            dy = one_tap(rng, ys, 1, signs(rng, cout) * np.exp2(rng.integers(-3, 4, size=cout)))
        self.x, self.dy = x.float(), dy.float()

    def forward(self, mul):
        B, cin, cout, H, W, s = self.geom
        k = self.k
        return mul(lambda a, b: torch.nn.grad.conv2d_weight(a, (cout, cin, k, k), b, stride=s, padding=k // 2), self.x.double(), self.dy.double())


# ---------------------------------------------------------------------------------------------- the training convolution
# One autograd step of lav_amd.train.hipnn.conv2d: forward (lav_conv2d), data gradient (the transposed lav_conv2d plan over the same
# weight tensor), weight gradient (lav_conv_wgrad / lav_conv_wgrad_amax).  dgrad / wgrad: who must take the leg - "lib" or "torch" -
# by the conditions of _Conv2d.backward and _wgrad_hip with LAV_TRAIN_WGRAD_MINPIX=1 (None: the leg is not asked for).
TrainGeom = namedtuple("TrainGeom", "name B cin cout kh kw stride ph pw dh dw H W x_grad env dgrad wgrad")


def _tg(name, B, cin, cout, k, s, p, H, W, dgrad, wgrad, d=(1, 1), x_grad=True, env=()):
    return TrainGeom(name, B, cin, cout, *k, s, *p, *d, H, W, x_grad, tuple(env), dgrad if x_grad else None, wgrad)


TRAIN_CONV_GEOMS = [
    _tg("a 3x3 s1 p1 64->64 12x16", 2, 64, 64, (3, 3), 1, (1, 1), 12, 16, "lib", "lib"),
    _tg("b 3x3 s2 p1 64->128 20x24 op1", 2, 64, 128, (3, 3), 2, (1, 1), 20, 24, "lib", "lib"),
    _tg("c 3x3 s2 p1 64->128 21x25 op0", 2, 64, 128, (3, 3), 2, (1, 1), 21, 25, "lib", "torch"),
    _tg("d 3x3 s2 p1 128->64 21x24 oph0 opw1", 1, 128, 64, (3, 3), 2, (1, 1), 21, 24, "torch", "torch"),
    _tg("e 3x3 s2 p1 128->64 20x24 strided dgrad on torch", 1, 128, 64, (3, 3), 2, (1, 1), 20, 24, "torch", "lib",
        env=(("LAV_TRAIN_DGRAD_STRIDED", "torch"),)),
    _tg("f 7x7 s2 p3 64->64 24x24", 2, 64, 64, (7, 7), 2, (3, 3), 24, 24, "lib", "lib"),
    _tg("g 7x7 s2 p3 64->64 25x27", 2, 64, 64, (7, 7), 2, (3, 3), 25, 27, "lib", "torch"),
    _tg("h 7x7 s2 p3 3->64 24x32 x without gradient", 2, 3, 64, (7, 7), 2, (3, 3), 24, 32, "lib", "torch", x_grad=False),
    _tg("h 7x7 s2 p3 3->64 24x32", 2, 3, 64, (7, 7), 2, (3, 3), 24, 32, "lib", "torch"),
    _tg("i 3x1 p(1,0) 64->64 12x16", 2, 64, 64, (3, 1), 1, (1, 0), 12, 16, "lib", "torch"),
    _tg("j 3x3 s1 p0 64->64 10x14", 2, 64, 64, (3, 3), 1, (0, 0), 10, 14, "lib", "torch"),
    _tg("k 3x3 dilation 2 p2 16->16 12x16", 2, 16, 16, (3, 3), 1, (2, 2), 12, 16, "torch", "torch", d=(2, 2)),
    _tg("l 3x3 s1 p1 48->40 13x17", 2, 48, 40, (3, 3), 1, (1, 1), 13, 17, "lib", "torch"),
    _tg("m 7x7 s2 p3 384->64 24x24", 1, 384, 64, (7, 7), 2, (3, 3), 24, 24, "lib", "lib"),
]


class _Leg:
    """One product of a TrainConvCase as a case of its own (`preconditions` and the host checks take one result)."""

    def __init__(self, case, n):
        self.case, self.n = case, n
        self.name = f"{case.name} / {('y', 'dx', 'dw')[n]}"

    def forward(self, mul):
        return self.case.product(n=self.n, mul=mul)


class TrainConvCase:
    """One autograd step of hipnn.conv2d at geometry g on class A: x in [-7, 7], w and dy in [-3, 3] ([-2, 2] on every side for
    K = cin kh kw > 4608, ConvLayerCase's rule - x and w ARE a ConvLayerCase's).  Three bilinear products: F.conv2d, its data gradient
    written as F.conv_transpose2d with the output padding of each dimension, torch.nn.grad.conv2d_weight."""

    def __init__(self, g: TrainGeom, key: str = "A"):
        assert key == "A", "the three legs share their operands: integers only"
        self.g, self.key = g, key
        self.name = f"train conv {g.name} / class {key}"
        self.fwd = ConvLayerCase(ConvGeom(g.name, g.B, g.cin, g.cout, g.kh, g.kw, g.stride, g.ph, g.pw, g.dh, g.dw, False, 0, g.H, g.W, "", ()), key)
        self.x, self.w = self.fwd.x, self.fwd.w
        oh, ow = self.fwd.out_hw()
        rng = rng_of("train conv", tuple(g[1:13]), key)
        self.dy = integers(rng, (g.B, g.cout, oh, ow), 3 if g.cin * g.kh * g.kw <= 4608 else 2).float()
        # the rows / columns of x the strided forward never reached
        self.out_pad = (g.H - ((oh - 1) * g.stride - 2 * g.ph + g.dh * (g.kh - 1) + 1), g.W - ((ow - 1) * g.stride - 2 * g.pw + g.dw * (g.kw - 1) + 1))

    def product(self, n, mul):
        g = self.g
        s, p, d = g.stride, (g.ph, g.pw), (g.dh, g.dw)
        x, w, dy = self.x.double(), self.w.double(), self.dy.double()
        if n == 0:
            return mul(self.fwd.op, x, w)
        if n == 1:
            return mul(lambda a, b: F.conv_transpose2d(a, b, None, s, p, self.out_pad, 1, d), dy, w)
        return mul(lambda a, b: torch.nn.grad.conv2d_weight(a, tuple(w.shape), b, stride=s, padding=p, dilation=d), x, dy)

    def legs(self):
        return [_Leg(self, n) for n in range(3)]

    def forward(self, mul):
        """(y, dx, dw) in float64 (dx also where the step does not ask for it)."""
        return tuple(self.product(n, mul) for n in range(3))


# One step per 16-channel chunk on the split kernel (a 1x1 layer; the one-tap parity class of b and c above is the other instance):
# the third chunk is staged into the first one's buffer while the first tap is still being fetched unless the kernel waits.
ONE_STEP_GEOM = ConvGeom("1x1 s1 128->128 24x24 (one step per chunk)", 2, 128, 128, 1, 1, 1, 0, 0, 1, 1, False, 0, 24, 24, "", ())

TRAIN_CONVT_GEOMS = [(2, 128, 128, 4, 2, 1, 0, 10, 12), (2, 128, 64, 4, 4, 0, 0, 5, 6), (2, 64, 128, 3, 2, 1, 1, 8, 8)]   # B, cin, cout, k, stride, pad, out_pad, H, W


class TrainConvTCase(TrainConvCase):
    """One autograd step of hipnn._ConvT2d (LAV_TRAIN_CONVT=hip) on class A: forward on the transposed plan (x and w ARE a transposed
    ConvLayerCase's), data gradient = the ordinary convolution of dy with the same tensor; the weight gradient is torch's."""

    def __init__(self, B, cin, cout, k, stride, pad, out_pad, H, W):
        self.geom = (B, cin, cout, k, stride, pad, out_pad, H, W)
        self.name = f"train convT {k}x{k} s{stride} p{pad} op{out_pad} {cin}->{cout} {H}x{W} / class A"
        self.fwd = ConvLayerCase(ConvGeom(self.name, B, cin, cout, k, k, stride, pad, pad, 1, 1, True, out_pad, H, W, "", ()), "A")
        self.x, self.w = self.fwd.x, self.fwd.w
        self.dy = integers(rng_of("train convT", self.geom), (B, cout, *self.fwd.out_hw()), 3).float()

    def product(self, n, mul):
        B, cin, cout, k, s, p, op, H, W = self.geom
        if n == 0:
            return mul(self.fwd.op, self.x.double(), self.w.double())
        return mul(lambda a, b: F.conv2d(a, b, None, s, p), self.dy.double(), self.w.double())

    def legs(self):
        return [_Leg(self, n) for n in range(2)]

    def forward(self, mul):
        """(y, dx) in float64."""
        return tuple(self.product(n, mul) for n in range(2))


# ---------------------------------------------------------------------------------------------- the BEV backbone
BACKBONE_CANVASES = [(48, 64), (96, 128), (160, 160), (320, 320)]


def fill_backbone(backbone):
    """One-tap weights +-1, BatchNorm with eps 0 that folds to scale 1 and a shift in {1, 2, 3}, on the modules of a ConvBackbone (before
    its engine is built).  Returns the float64 parameters in execution order: {"s1": [(w, shift)], ..., "ups": [(w, shift, k, pad, out_pad)]}."""
    from torch import nn
    rng = rng_of("backbone")
    params = {}
    with torch.no_grad():
        for name in ("conv1", "conv2", "conv3", "upconv1", "upconv2", "upconv3"):
            seq = getattr(backbone, name)
            params[name] = []
            for j in range(0, len(seq), 3):
                conv, bn = seq[j], seq[j + 2]
                tr = isinstance(conv, nn.ConvTranspose2d)
                cout = conv.weight.shape[1 if tr else 0]
                w = one_tap(rng, tuple(conv.weight.shape), 1 if tr else 0, signs(rng, cout))
                shift = t64(rng.integers(1, 4, size=cout))
                conv.weight.copy_(w.float())
                bn.eps = 0.0
                bn.running_mean.zero_(); bn.running_var.fill_(1.0); bn.weight.fill_(1.0); bn.bias.copy_(shift.float())
                params[name].append((w, shift, conv.stride[0], conv.padding[0], conv.output_padding[0] if tr else 0))
    return params


class BackboneCase:
    """ConvBackbone on a (B, 64, H, W) canvas of integers in [0, 7] with fill_backbone's parameters."""

    def __init__(self, params, B, H, W):
        self.name = f"backbone B {B} canvas {H}x{W}"
        self.params = params
        self.x = t64(rng_of("canvas", B, H, W).integers(0, 8, size=(B, 64, H, W))).float()

    def forward(self, mul):
        y, feats = self.x.double(), []
        one = torch.ones(1, dtype=torch.float64)
        for name in ("conv1", "conv2", "conv3"):
            for w, shift, s, p, _ in self.params[name]:
                y = mul.see(affine(F.relu(mul(lambda a, b, s=s, p=p: F.conv2d(a, b, None, s, p), y, w)), one.expand(len(shift)), shift))
            feats.append(y)
        outs = []
        for name, f in zip(("upconv1", "upconv2", "upconv3"), feats):
            (w, shift, s, p, op), = self.params[name]
            outs.append(mul.see(affine(F.relu(mul(lambda a, b, s=s, p=p, op=op: F.conv_transpose2d(a, b, None, s, p, op), f, w)), one.expand(len(shift)), shift)))
        return torch.cat(outs, dim=1)


# ---------------------------------------------------------------------------------------------- comparison
def assert_exact(got: torch.Tensor, want: torch.Tensor, what: str):
    """torch.equal(kernel output in float64 on the host, float64 reference); on failure: how many outputs differ, the worst difference
    and the first differing index."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if torch.equal(got, want):
        return
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    diff = torch.where(bad, (got - want).abs(), torch.zeros_like(want))
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    first = tuple(int(v) for v in bad.nonzero()[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ from float64; worst |difference| {float(diff.max()):.6g}; "
                         f"first at {first}: kernel {float(got[first])!r}, float64 {float(want[first])!r}")
