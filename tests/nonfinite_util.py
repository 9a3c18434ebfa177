"""NaN and Inf through every epilogue (tests/test_nonfinite_host.py, tests/test_gpu_nonfinite.py).

include/lav_amd.h promises that a non-finite activation makes the outputs it reaches non-finite and changes no other bit.  A ReLU written
`v > 0.f ? v : 0.f` or fmaxf(v, 0.f), and a 2x2 pooling nested from fmaxf, break the first half silently: the NaN comes out as a finite
number that no health check counts.  `check` decides from four tensors - the kernel on planted and on clean input, the float64 torch
reference on planted and on clean input - whether a kernel kept the promise:

  NaN plant   bad = isnan(reference on the planted input), a proper non-empty subset of the outputs.  Where bad: the kernel gives NaN.
              Elsewhere: the kernel's output equals its own clean run bit for bit (uint32 views).
  Inf plant   (+Inf in the first planted element, -Inf in the second.)  Where the reference is non-finite: the kernel is non-finite (the
              split precisions give NaN for Inf, as documented).  Where the plant does not reach: bit for bit the clean run.  Where it
              reaches and the reference is finite - a -Inf that a ReLU turned into 0 - the kernel gives a finite number or NaN, never Inf.
              "Reaches" is `reach` = the NaN plant's `bad` at the same elements (a ReLU output of 0 can EQUAL the clean reference where
              the clean value was negative too, so "differs from the clean reference" alone would ask a split precision for clean bits
              where it rightly holds NaN); without `reach`: where the two references differ.

The references are plain torch in float64 on the CPU, with the ReLU and the 2x2 pooling handed in: torch.relu / F.max_pool2d for the
reference, `drop_relu` / `drop_pool` (the device arithmetic before csrc/common.hpp's relu_nan / max_nan) for the emulations the host
test shows the rule rejecting.  Weights are dense and never zero, BatchNorm scales never zero (exact_util.pow2_bn), so what a plant
reaches does not depend on sparsity.  Planted elements hold 0.25 in the clean input - never a tensor's maximum, so a scale taken from
the finite maximum is the clean run's.

Kernels that hand a scale from layer to layer (ConvRun, ConvTileRun, the fp16 pair chain: per workgroup, per row or per tensor, from the
largest FINITE value) get one dominant channel: its BatchNorm shift is 768 and every other value stays below 512, so at EVERY pixel of
EVERY intermediate map the largest magnitude lies near 768, inside [512, 1024) - whatever region a maximum is taken over, and whatever
part of it a plant has turned into NaN, the power-of-two scale is the clean run's, and bit equality outside the reach is a fair demand
(`handoff_premise`, asserted on the host for every such case with the narrower bucket [640, 960]: a kernel's rounding cannot leave it)."""
from __future__ import annotations

import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import exact_util as E

NAN, INF = float("nan"), float("inf")
PLANTS = ("nan", "inf")
CLEAN_AT_PLANT = 0.25
DOMINANT = 768.0


class RuleViolation(AssertionError):
    """The kernel (or emulation) broke the rule."""


class BrokenPremise(AssertionError):
    """The case itself is unfit: the reference's reach is empty or everything, or the clean run is not finite."""


# ---------------------------------------------------------------------------------------------- the rule
def _first(mask):
    return tuple(int(v) for v in np.argwhere(mask)[0])


def check(plant, got_planted, got_clean, ref_planted, ref_clean, reach=None, what=""):
    """Raises RuleViolation / BrokenPremise (see the module docstring); returns the reach (bool array) of a NaN plant."""
    gp, gc = (np.ascontiguousarray(t.detach().cpu().float().numpy()) for t in (got_planted, got_clean))
    rp, rc = (t.detach().cpu().double().numpy() for t in (ref_planted, ref_clean))
    if not (gp.shape == gc.shape == rp.shape == rc.shape):
        raise BrokenPremise(f"{what}: shapes {gp.shape} {gc.shape} {rp.shape} {rc.shape}")
    if not np.isfinite(rc).all():
        raise BrokenPremise(f"{what}: the clean reference is not finite")
    if not np.isfinite(gc).all():
        raise RuleViolation(f"{what}: the clean run is not finite")
    same_bits = gp.view(np.uint32) == gc.view(np.uint32)
    if plant == "nan":
        bad = np.isnan(rp)
        if not 0 < int(bad.sum()) < bad.size:
            raise BrokenPremise(f"{what}: the NaN reaches {int(bad.sum())} of {bad.size} reference outputs")
        if np.isinf(rp).any():
            raise BrokenPremise(f"{what}: the reference of a NaN plant holds an Inf")
        dropped, moved, leaked = bad & ~np.isnan(gp), ~bad & ~same_bits, np.zeros_like(bad)
    elif plant == "inf":
        nonfin = ~np.isfinite(rp)
        if not 0 < int(nonfin.sum()) < nonfin.size:
            raise BrokenPremise(f"{what}: the reference is non-finite at {int(nonfin.sum())} of {nonfin.size} outputs")
        inside = np.asarray(reach, bool) if reach is not None else rp != rc
        if inside.shape != rp.shape or (nonfin & ~inside).any() or inside.all():
            raise BrokenPremise(f"{what}: the reach does not fit the reference")
        dropped = nonfin & np.isfinite(gp)
        moved = ~inside & ~same_bits
        leaked = inside & ~nonfin & np.isinf(gp)
        bad = inside
    else:
        raise KeyError(plant)
    said = []
    if dropped.any():
        i = _first(dropped)
        said.append(f"{int(dropped.sum())} outputs are finite where the reference is {'NaN' if plant == 'nan' else 'non-finite'} "
                    f"(first at {i}: {gp[i]!r}, clean run {gc[i]!r})")
    if moved.any():
        i = _first(moved)
        said.append(f"{int(moved.sum())} outputs outside the reach differ from the clean run's bits (first at {i}: {gp[i]!r} vs {gc[i]!r})")
    if leaked.any():
        i = _first(leaked)
        said.append(f"{int(leaked.sum())} outputs are Inf where the reference is finite (first at {i})")
    if said:
        raise RuleViolation(f"{what}, {plant} plant: " + "; ".join(said))
    return bad


def check_case(got, refs, what):
    """got / refs: {"clean" | "nan" | "inf": tuple of tensors}; every output of the case under both plants."""
    for n, (gc, rc) in enumerate(zip(got["clean"], refs["clean"])):
        reach = check("nan", got["nan"][n], gc, refs["nan"][n], rc, what=f"{what}, output {n}")
        check("inf", got["inf"][n], gc, refs["inf"][n], rc, reach=reach, what=f"{what}, output {n}")


# ---------------------------------------------------------------------------------------------- what the reference is handed
def drop_relu(v):
    """`v > 0.f ? v : 0.f` (and fmaxf(v, 0.f)): a NaN becomes 0."""
    return torch.where(v > 0, v, torch.zeros_like(v))


def drop_pool(x, k=2):
    """fmaxf(fmaxf(a, b), fmaxf(c, d)) over 2x2 windows: a NaN is dropped."""
    assert k == 2
    h, w = x.shape[-2] // 2 * 2, x.shape[-1] // 2 * 2
    a, b, c, d = x[..., 0:h:2, 0:w:2], x[..., 0:h:2, 1:w:2], x[..., 1:h:2, 0:w:2], x[..., 1:h:2, 1:w:2]
    return torch.fmax(torch.fmax(a, b), torch.fmax(c, d))


GOOD = dict(relu=torch.relu, pool=F.max_pool2d)


def dense(rng, shape, bound):
    """+-U(0.5, 1) * bound in float32: dense, never zero."""
    return torch.from_numpy((E.signs(rng, shape) * rng.uniform(0.5, 1.0, size=shape) * bound).astype(np.float32))


def normal(rng, shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def spatial_plants(B, c_in, c_co, H, W, radius=1):
    """[interior element, corner element] of a (B, C, H, W) map: the centre of image 0 (pixel (1, 1) where the centre's reach of `radius`
    pixels would cover a single image together with the corner's) and the last pixel of the last image."""
    iy, ix = H // 2, W // 2
    if B == 1 and (iy - radius <= 0 and iy + radius >= H - 1) and (ix - radius <= 0 and ix + radius >= W - 1):
        iy, ix = min(1, H - 1), min(1, W - 1)
    return [(0, c_in, iy, ix), (B - 1, c_co, H - 1, W - 1)]


class Case:
    """x: the clean float32 input (planted elements hold 0.25); plants: [interior, corner]; forward(x64, relu, pool) -> tuple of float64
    outputs.  relu / pool: whether the operation has a ReLU / a 2x2 pooling an emulation can break."""
    relu, pool = True, False
    handoffs = None          # forward_maps(x64) of the cases that hand scales on

    def input(self, plant):
        x = self.x.clone()
        for i, at in enumerate(self.plants):
            assert float(x[at]) == CLEAN_AT_PLANT
            if plant != "clean":
                x[at] = NAN if plant == "nan" else (INF if i == 0 else -INF)
        return x

    def outputs(self, relu=torch.relu, pool=F.max_pool2d):
        return {p: self.forward(self.input(p).double(), relu, pool) for p in ("clean",) + PLANTS}

    def place(self):
        for at in self.plants:
            self.x[at] = CLEAN_AT_PLANT
        assert float(self.x.abs().max()) > 1.0


_refs: dict = {}


def references(case):
    """The float64 references of a case, computed once per name and never written to (the last few cases are kept)."""
    if case.name not in _refs:
        while len(_refs) >= 8:
            _refs.pop(next(iter(_refs)))
        with torch.no_grad():
            _refs[case.name] = case.outputs()
    return _refs[case.name]


def handoff_premise(case):
    """Every pixel of every map a scale is taken from has its largest magnitude in [640, 960] on the clean input: well inside [512, 1024)."""
    with torch.no_grad():
        maps = case.forward_maps(case.x.double())
    for n, m in enumerate(maps):
        top = m.abs().amax(dim=1)
        lo, hi = float(top.min()), float(top.max())
        if not (640.0 <= lo and hi <= 960.0):
            raise BrokenPremise(f"{case.name}: map {n} has per-pixel maxima in [{lo:.6g}, {hi:.6g}], not inside [640, 960]")


def _dominant_bn(rng, C, shift=DOMINANT):
    """exact_util.pow2_bn (scales 0.5 / 1, eps 0) with channel C // 3 the dominant one: scale 1, shift `shift`."""
    (mean, var, gamma, beta), scale, sh = E.pow2_bn(rng, C)
    c = C // 3
    mean[c], gamma[c], beta[c], scale[c], sh[c] = 0.0, 2.0, shift, 1.0, shift
    return (mean, var, gamma, beta), scale, sh


def _dominant_input(rng, shape):
    x = normal(rng, shape, 40.0)
    x[:, shape[1] // 3] = DOMINANT + normal(rng, (shape[0],) + tuple(shape[2:])).abs()
    return x


# ---------------------------------------------------------------------------------------------- ops.ConvLayer
@functools.lru_cache(maxsize=2)
def _conv_products(g):
    """(weight, clean window, plants inside the window, {plant: the convolution in float64}) of geometry g: one product for the four
    epilogues, the three inputs stacked into one batch."""
    rng = E.rng_of("nonfinite conv", tuple(g))
    inner = E.ConvLayerCase(g, "A")
    w = dense(rng, tuple(inner.w.shape), 1.0 / np.sqrt(g.cin * g.kh * g.kw))
    xw = normal(rng, (g.B, g.cin, g.H, g.W), 2.0)
    plants = spatial_plants(g.B, g.cin // 2, g.cin - 1, g.H, g.W, radius=max(g.kh * g.dh, g.kw * g.dw))
    if not g.transposed and g.stride > 1:
        # a strided window does not read every pixel (1x1 stride 2 reads the even ones): the interior plant moves to the first tap of an
        # output, the corner plant to the last pixel the last output reads
        first = lambda i, p: max((i + p) // g.stride * g.stride - p, 0)
        last = lambda n, k, p, d: min((n + 2 * p - d * (k - 1) - 1) // g.stride * g.stride - p + d * (k - 1), n - 1)
        (b0, c0, y0, x0), (b1, c1, _, _) = plants
        plants = [(b0, c0, first(y0, g.ph), first(x0, g.pw)), (b1, c1, last(g.H, g.kh, g.ph, g.dh), last(g.W, g.kw, g.pw, g.dw))]
    for at in plants:
        xw[at] = CLEAN_AT_PLANT
    stack = []
    for p in ("clean",) + PLANTS:
        x = xw.clone()
        if p != "clean":
            for i, at in enumerate(plants):
                x[at] = NAN if p == "nan" else (INF if i == 0 else -INF)
        stack.append(x)
    with torch.no_grad():
        y = inner._conv(torch.cat(stack).double(), w.double(), True)
    return w, xw, plants, dict(zip(("clean",) + PLANTS, y.split(g.B)))


class ConvCase(Case):
    """exact_util.ConvLayerCase's geometry, windows, bias, BatchNorm, residual and epilogue order, on N(0, 2) activations and dense weights."""

    def __init__(self, g, epilogue):
        self.g, self.epilogue = g, epilogue
        self.name = f"nonfinite {g.name} / {epilogue}"
        self.relu = epilogue in ("relu_affine_windows", "affine_residual_relu")
        c = self.inner = E.ConvLayerCase(g, "A", epilogue)
        c.w, xw, plants, _ = _conv_products(g)
        x = c.x.clone()
        x[:, c.in_off:c.in_off + g.cin] = xw
        c.x = self.x = x
        self.plants = [(b, c.in_off + ch, y, xx) for b, ch, y, xx in plants]

    def outputs(self, relu=torch.relu, pool=None):
        c = self.inner
        out = {}
        for p, y in _conv_products(self.g)[3].items():
            if c.bias is not None:
                y = y + c.bias.double()[None, :, None, None]
            if c.relu_pre:
                y = relu(y)
            if c.bn is not None:
                y = E.affine(y, c._scale, c._shift)
            if c.residual is not None:
                y = y + c.residual.double()
            if c.relu_post:
                y = relu(y)
            out[p] = (y,)
        return out


# ---------------------------------------------------------------------------------------------- runs, pairs, chains
class RunCase(Case):
    """exact_util.RunCase's operation - L x (conv3x3 -> ReLU -> affine) on a (1, C, H, W) map - with dense weights (sum |w| <= 1 / 8 per
    output) and a dominant channel."""

    def __init__(self, C, H, W, L):
        self.name = f"nonfinite run C {C} {H}x{W} L {L}"
        rng = E.rng_of("nonfinite run", C, H, W, L)
        self.x = _dominant_input(rng, (1, C, H, W))
        self.plants = spatial_plants(1, 1, C - 1, H, W, radius=L)
        self.place()
        self.layers = []          # (weight f32, bn tuple, scale f64, shift f64): exact_util.RunCase's layout
        for _ in range(L):
            bn, scale, shift = _dominant_bn(rng, C)
            self.layers.append((dense(rng, (C, C, 3, 3), 1.0 / (72.0 * C)), bn, scale, shift))

    def forward_maps(self, x, relu=torch.relu, pool=None):
        maps = [x]
        for w, _, scale, shift in self.layers:
            maps.append(E.affine(relu(F.conv2d(maps[-1], w.double(), None, 1, 1)), scale, shift))
        return maps

    def forward(self, x, relu=torch.relu, pool=None):
        return (self.forward_maps(x, relu)[-1],)


class PairsCase(Case):
    """exact_util.PairsCase's operation - conv3x1 + bias -> ReLU -> conv1x3 + bias -> affine (+ residual) -> ReLU, pair after pair - with
    dense weights (sum |w| <= 1 / 8) and a dominant channel: shift 768 on the pairs without a residual, 0 where the block's input (which
    already holds it) is added."""

    def __init__(self, C, H, W, dils, residual, own_residual=False, B=2):
        self.name = f"nonfinite pairs C {C} {H}x{W} dilations {dils} residual {residual} own {own_residual}"
        rng = E.rng_of("nonfinite pairs", C, H, W, tuple(dils), tuple(residual), own_residual)
        self.C, self.dils, self.residual, self.own_residual = C, list(dils), list(residual), own_residual
        self.x = _dominant_input(rng, (B, C, H, W))
        self.plants = spatial_plants(B, 1, C - 1, H, W)
        self.place()
        self.pairs = []          # (wa, ba, wb, bb, bn tuple, scale, shift): exact_util.PairsCase's layout
        for res in residual:
            bn, scale, shift = _dominant_bn(rng, C, 0.0 if (res or own_residual) else DOMINANT)
            self.pairs.append((dense(rng, (C, C, 3, 1), 1.0 / (24.0 * C)), E.integers(rng, (C,), 1).float(),
                               dense(rng, (C, C, 1, 3), 1.0 / (24.0 * C)), E.integers(rng, (C,), 1).float(), bn, scale, shift))

    def forward_maps(self, x, relu=torch.relu, pool=None):
        ins = [x]
        for (wa, ba, wb, bb, _, scale, shift), (da, db), res in zip(self.pairs, self.dils, self.residual):
            x = ins[-1]
            mid = relu(F.conv2d(x, wa.double(), ba.double(), 1, (da, 0), (da, 1)))
            y = E.affine(F.conv2d(mid, wb.double(), bb.double(), 1, (0, db), (1, db)), scale, shift)
            if res:
                y = y + ins[-2]
            elif self.own_residual:
                y = y + x
            ins.append(relu(y))
        return ins

    def forward(self, x, relu=torch.relu, pool=None):
        return (self.forward_maps(x, relu)[-1],)


def pair_case(C, H, W, d, with_res):
    return PairsCase(C, H, W, [(d, d)], [False], own_residual=with_res)


def chain_case(C, H, W, dils):
    d2, res = [], []
    for d in dils:
        d2 += [(1, 1), (d, d)]
        res += [False, True]
    return PairsCase(C, H, W, d2, res)


# ---------------------------------------------------------------------------------------------- up-convolution, grouped deconvolution
class UpconvCase(Case):
    """ops.PointwiseUpconv: ConvTranspose2d(cin, cout, k, stride k, pad, out_pad, no bias) -> ReLU -> affine."""

    def __init__(self, cin, cout, k, pad, opad, H, W, B=2):
        self.name = f"nonfinite upconv {cin}->{cout} k {k} pad {pad} out_pad {opad} {H}x{W}"
        rng = E.rng_of("nonfinite upconv", cin, cout, k, pad, opad, H, W)
        self.geom = (cin, cout, k, pad, opad)
        self.x = normal(rng, (B, cin, H, W), 2.0)
        self.plants = spatial_plants(B, cin // 2, cin - 1, H, W)
        self.place()
        self.w = dense(rng, (cin, cout, k, k), 1.0 / np.sqrt(cin))
        self.bn, self.scale, self.shift = E.pow2_bn(rng, cout, scales=(0.5, 1.0, 2.0))

    def forward(self, x, relu=torch.relu, pool=None):
        cin, cout, k, pad, opad = self.geom
        return (E.affine(relu(F.conv_transpose2d(x, self.w.double(), None, k, pad, opad)), self.scale, self.shift),)


DECONV_EPILOGUES = ("plain", "sigmoid", "softmax")


class DeconvCase(Case):
    """ops.GroupedDeconv: ConvTranspose2d(cin_g, o, 3, 2, 1, 1) + bias per group; plain, sigmoid on the channels from 1 on, or a soft-max
    over each group's channels.  No ReLU, no pooling: nothing for an emulation to break."""
    relu = False

    def __init__(self, outs, cin_g, H, W, B, epilogue):
        self.name = f"nonfinite grouped deconv outs {outs} cin {cin_g} {H}x{W} B {B} / {epilogue}"
        rng = E.rng_of("nonfinite deconv", tuple(outs), cin_g, H, W, B)
        self.outs, self.cin_g, self.epilogue = outs, cin_g, epilogue
        C = cin_g * len(outs)
        self.x = normal(rng, (B, C, H, W), 2.0)
        self.plants = spatial_plants(B, cin_g // 2, C - 1, H, W)     # the first and the last group
        self.place()
        self.ws = [dense(rng, (cin_g, o, 3, 3), 1.0 / np.sqrt(cin_g)) for o in outs]
        self.biases = [normal(rng, (o,)) for o in outs]

    def forward(self, x, relu=None, pool=None):
        ys = []
        for i, (w, b) in enumerate(zip(self.ws, self.biases)):
            y = F.conv_transpose2d(x[:, i * self.cin_g:(i + 1) * self.cin_g], w.double(), b.double(), 2, 1, 1)
            ys.append(torch.softmax(y, dim=1) if self.epilogue == "softmax" else y)
        y = torch.cat(ys, dim=1)
        if self.epilogue == "sigmoid":
            y = torch.cat([y[:, :1], torch.sigmoid(y[:, 1:])], dim=1)
        return (y,)


# ---------------------------------------------------------------------------------------------- ERFNet's entry, the pooled branch
ERFNET_GEOMS = [(1, 4, 4), (3, 36, 68)]
ERFNET_PLANTS = ("corner", "window maximum", "not the window maximum")


class ErfnetCase(Case):
    """ops.erfnet_entry: two DownsamplerBlocks - cat(conv3x3 s2, max-pool 2x2) -> BatchNorm (eval) -> ReLU - on s x + t, the blocks and
    inputs of tests/test_gpu_erfnet_edge.py.  where: "corner" - the last pixel of the last image (the convolution branch reads it at
    its border only) together with an interior pixel; or ONE interior pixel that is / is not the largest of its 2x2 pooling window in the
    clean input (an fmaxf pooling drops the first into the window's second value and the second without a trace)."""
    pool = True

    def __init__(self, B, H, W, affine, where):
        from tests import test_gpu_erfnet_edge as T
        self.name = f"nonfinite erfnet entry {B}x{H}x{W} affine {affine} / {where}"
        self.geom, self.affine, self.where = (B, H, W), affine, where
        self.blocks = T.blocks()
        self.x = T.raw_input(B, H, W, affine).clone()
        iy, ix = (H // 2) | 1, (W // 2) | 1                    # odd row and column: the last element of its pooling window
        self.plants = [(0, 1, iy, ix)] + ([(B - 1, 2, H - 1, W - 1)] if where == "corner" else [])
        if where == "window maximum":        # (the input affine has a positive scale: the order of a window is the raw values')
            self.x[0, 1, iy - 1:iy + 1, ix - 1:ix + 1] = torch.tensor([[0.0, 0.125], [0.0625, 0.0]])
        elif where == "not the window maximum":
            self.x[0, 1, iy - 1:iy + 1, ix - 1:ix + 1] = torch.tensor([[3.0, 1.0], [2.0, 0.0]])
        for at in self.plants:
            self.x[at] = CLEAN_AT_PLANT

    def forward(self, x, relu=torch.relu, pool=F.max_pool2d):
        if self.affine is not None:
            x = x * self.affine[0] + self.affine[1]
        for b in self.blocks:
            b = copy.deepcopy(b).double()
            y = torch.cat([b.conv(x), pool(x, 2)], 1)
            x = relu(F.batch_norm(y, b.bn.running_mean, b.bn.running_var, b.bn.weight, b.bn.bias, False, 0.0, b.bn.eps))
        return (x,)


class PoolAffineCase(Case):
    """ops.pool_affine: 2x2 max pooling -> per-channel affine (-> ReLU) of (2, 3, 6, 8) into channels [off, off + 3) of a wider buffer."""
    pool = True

    def __init__(self, relu):
        self.name = f"nonfinite pool_affine relu {relu}"
        self.relu = relu
        rng = E.rng_of("nonfinite pool_affine")
        self.x = normal(rng, (2, 3, 6, 8), 2.0)
        self.plants = [(0, 1, 3, 3), (1, 2, 5, 7)]
        self.x[0, 1, 2:4, 2:4] = torch.tensor([[-1.0, -2.0], [-3.0, 0.0]])      # the interior plant is its window's maximum ...
        self.x[1, 2, 4:6, 6:8] = torch.tensor([[1.0, 2.0], [3.0, 0.0]])         # ... the corner plant is not
        self.place()
        self.scale, self.shift = E.t64([2.0, 0.5, -1.0]), E.t64([1.0, -2.0, 0.5])      # (+Inf in channel 1 stays +Inf)
        self.total, self.off = 7, 2

    def forward(self, x, relu=torch.relu, pool=F.max_pool2d):
        y = E.affine(pool(x, 2), self.scale, self.shift)
        return (relu(y) if self.relu else y,)


# ---------------------------------------------------------------------------------------------- heads at the peaks, attention pooling
class HeadsCase(Case):
    """ops.heads_at_peaks at the smallest case of tests/test_gpu_heads_at_peaks.py: Conv2d 3x3 -> ReLU -> BatchNorm (eval) ->
    ConvTranspose2d 3x3 s2 per head, gathered at hand-placed rows; the feature map planted under the peak rows at (2, 2) ... (3, 3) and
    at its last pixel, under the corner row.  Output: the head columns (3 ...) of every row."""

    def __init__(self, cin=20, H=5, W=7, hidden=8, outs=(2, 2)):
        from tests import heads_peaks_util as hp
        self.name = f"nonfinite heads at peaks cin {cin} {H}x{W} hidden {hidden} outs {outs}"
        self.hw = (H, W)
        self.x = torch.randn((cin, H, W), generator=torch.Generator().manual_seed(cin + hidden)).clone()
        self.x[0, 0, 0] = 5.0
        self.heads = [hp.make_head(cin, hidden, o, 10 * g + o) for g, o in enumerate(outs)]
        self.rows, _ = hp.hand_rows(H, W)
        self.plants = [(3, 1, 1), (cin - 1, H - 1, W - 1)]
        self.place()

    def forward(self, x, relu=torch.relu, pool=None):
        from tests import heads_peaks_util as hp
        maps = []
        for head in self.heads:
            conv, bn, ct = (copy.deepcopy(m).double() for m in head)
            maps.append(ct(bn(relu(conv(x[None]))))[0].numpy())
        with np.errstate(invalid="ignore"):
            return (torch.from_numpy(hp.gather(self.rows, maps, *self.hw)),)


class AttnCase(Case):
    """ops.attn_pool through rgb.Attention.eval() at (3, 512, 8, 6, 15): one token of image 1 planted, so that image's whole row is
    non-finite and the other rows keep their bits.  No ReLU, no pooling."""
    relu = False

    def __init__(self, B=3, C=512, heads=8, h=6, w=15):
        from tests import test_gpu_kernel_size_paths as T
        self.name = f"nonfinite attn_pool {B}x{C}x{h}x{w} heads {heads}"
        self.module = T._attention(C, heads, seed=B * 1000 + h)
        self.x = T._attn_input(B, C, h, w)[0].clone()
        self.plants = [(1, C // 2, h // 2, w // 2), (1, C - 1, h - 1, w - 1)]
        self.place()

    def forward(self, x, relu=None, pool=None):
        return (copy.deepcopy(self.module).double().train()(x),)


# ---------------------------------------------------------------------------------------------- the training kernels
BN_SHAPES = [(3, 5, 7, 9), (3, 3, 52, 56)]          # the second one is tests/test_gpu_kernel_size_paths.BN_VEC_S2 (asserted by the GPU test)
BN_MODES = ("plain", "relu_pre", "relu_post", "residual")
BN_MOMENTUM, BN_EPS = 0.01, 1e-3


class BnCase(Case):
    """hipnn.bn_act (modes plain / relu_pre / relu_post / residual) and hipnn.bn_mask_act (mode "mask": relu(m * BN(z) + residual)) in train
    mode: outputs (y, running_mean, running_var).  Both plants lie in channel 1 - the planted channel is non-finite everywhere, its
    running statistics too, as in torch - and every other channel and statistic keeps its bits."""

    def __init__(self, shape, mode):
        self.name = f"nonfinite bn {shape} / {mode}"
        self.shape, self.mode = shape, mode
        self.relu = mode != "plain"
        B, C, H, W = shape
        rng = E.rng_of("nonfinite bn", shape, mode)
        self.x = normal(rng, shape, 1.5) + 0.3
        self.plants = [(0, 1, H // 2, W // 2), (B - 1, 1, H - 1, W - 1)]
        self.place()
        self.res = normal(rng, shape) if mode in ("residual", "mask") else None
        self.gamma = torch.linspace(0.5, 1.5, C)
        self.beta = torch.linspace(-0.3, 0.3, C)
        self.m = None
        if mode == "mask":
            self.m = torch.from_numpy(rng.integers(0, 2, size=(B, C)) * 1.25).float()
            self.m[0, 1], self.m[B - 1, 1], self.m[0, 0] = 1.25, 0.0, 0.0      # the planted channel: kept in image 0, dropped in the last one

    def forward(self, x, relu=torch.relu, pool=None):
        C = self.shape[1]
        rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        t = relu(x) if self.mode == "relu_pre" else x
        y = F.batch_norm(t, rm, rv, self.gamma.double(), self.beta.double(), True, BN_MOMENTUM, BN_EPS)
        if self.m is not None:
            y = self.m.double()[:, :, None, None] * y
        if self.res is not None:
            y = y + self.res.double()
        if self.mode in ("relu_post", "residual", "mask"):
            y = relu(y)
        return (y, rm, rv)


PAIR_TRAIN_GEOMS = [(16, 128, 1), (128, 32, 4)]          # C, W, dilation (tests/test_gpu_train_seg.py), on 3 images of 7 rows


class PairTrainCase(Case):
    """hipnn.pair_train's forward: z = conv1x3_d(relu(conv3x1_d(x) + ba)) + bb."""

    def __init__(self, C, W, d, B=3, H=7):
        self.name = f"nonfinite pair_train C {C} W {W} d {d}"
        self.d = d
        rng = E.rng_of("nonfinite pair_train", C, W, d)
        self.x = normal(rng, (B, C, H, W), 2.0)
        self.plants = spatial_plants(B, 1, C - 1, H, W)
        self.place()
        self.wa, self.ba = dense(rng, (C, C, 3, 1), 1.0 / np.sqrt(3 * C)), normal(rng, (C,), 0.3)
        self.wb, self.bb = dense(rng, (C, C, 1, 3), 1.0 / np.sqrt(3 * C)), normal(rng, (C,), 0.3)

    def forward(self, x, relu=torch.relu, pool=None):
        d = self.d
        t = relu(F.conv2d(x, self.wa.double(), self.ba.double(), 1, (d, 0), (d, 1)))
        return (F.conv2d(t, self.wb.double(), self.bb.double(), 1, (0, d), (1, d)),)


# ---------------------------------------------------------------------------------------------- the parametrisation both files share
def conv_cases():
    return [(g, ep) for g in E.conv_geometries() for ep in E.EPILOGUES]


def other_cases():
    """name -> constructor of every case that is not an ops.ConvLayer launch."""
    out = {}

    def add(make, *a):
        out[f"{make.__name__}{a}"] = functools.partial(make, *a)
    for geom in E.RUN_GEOMS:
        add(RunCase, *geom)
    for H, W, L in E.TILE_GEOMS:
        add(RunCase, 64, H, W, L)
    for C, H, W, d in E.PAIR_GEOMS:
        for with_res in (False, True):
            add(pair_case, C, H, W, d, with_res)
    for C, H, W, dils in E.CHAIN_GEOMS:
        add(chain_case, C, H, W, dils)
    for geom in E.UPCONV_GEOMS:
        add(UpconvCase, *geom)
    for outs, cin_g, H, W, B in E.DECONV_GEOMS:
        for ep in DECONV_EPILOGUES:
            add(DeconvCase, outs, cin_g, H, W, B, ep)
    for B, H, W in ERFNET_GEOMS:
        for affine in (None, (2.0 / 255.0, -1.0)):
            for where in ERFNET_PLANTS:
                add(ErfnetCase, B, H, W, affine, where)
    for relu in (True, False):
        add(PoolAffineCase, relu)
    add(HeadsCase)
    add(AttnCase)
    for shape in BN_SHAPES:
        for mode in BN_MODES + ("mask",):
            add(BnCase, shape, mode)
    for geom in PAIR_TRAIN_GEOMS:
        add(PairTrainCase, *geom)
    return out
