"""LAV_CONV_F16X3's contract: each operand of a split-kernel convolution is two fp16 pieces scaled by one power of two per tensor,
and the activations' scale comes from maxima that the producing layer left in an ops.Amax (lav_conv2d_amax) instead of a measurement.

A. The arithmetic at the edges of its range, against float64: magnitudes up to FLT_MAX, a scale product beyond FLT_MAX, degenerate
   scales, fp32 subnormals, Inf / NaN, and the per-element error of tensors whose values span many decades (the two-term bound that
   include/lav_amd.h states).
B. Stale bounds on the eval path: a bound handed on with a tensor is void once the tensor changes in place or its Amax is rewritten
   by a later call (ops.amax_of then returns None and the consumer measures its input); valid hand-offs stay on.
C. One bound per stream: graphs that run concurrently never share an Amax.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lav_amd import _lib, ops, synth
from tests.util import CFG, build_models

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FLT_MAX = torch.finfo(torch.float32).max
# The per-element floor of the two-term bound: |y - ref| <= 2e-6 sum|w||x| + FLOOR_C (q_x sum|w| + q_w sum|x|) over the receptive field,
# q = 2^-25 of the tensor's fp16 scale (half the fp16 subnormal quantum 2^-24 of a scaled value).  Rounding alone gives FLOOR_C = 1;
# measured: at most 0.21 of that floor where it dominates (test_f16x3_dynamic_range); held at 2 for margin.
FLOOR_C = 2.0


def f16_scale(m: float) -> float:
    """The power of two the kernels divide a tensor by (conv_split_kernel.hpp, common.hpp f16_scale_of): max |t| into [2^14, 2^15),
    exponent floored at -100; 1 for an all-zero tensor."""
    if not m > 0:
        return 1.0
    e = math.frexp(m)[1]
    return math.ldexp(1.0, max(e, -100) - 15)


def piece_quantum(t: torch.Tensor) -> float:
    """Largest error of one element's two fp16 pieces, in the tensor's own units: 2^-25 x its scale."""
    finite = t[torch.isfinite(t)]
    return math.ldexp(f16_scale(finite.abs().max().item() if finite.numel() else 0.0), -25)


def f16_layer(w, monkeypatch=None, force="", B=1, H=24, W=24, **kw):
    """A LAV_CONV_F16X3 ConvLayer whose plan on (B, ., H, W) is the fp16 three-product split kernel (asserted)."""
    if force:
        monkeypatch.setenv("LAV_CONV_SPLIT", "2")
        monkeypatch.setenv("LAV_SPLIT_FORCE", force)
    layer = ops.ConvLayer(w, precision=_lib.CONV_F16X3, device=DEV, **kw)
    d = _lib.Conv.from_buffer_copy(layer.desc)
    d.batch, d.h, d.w = B, H, W
    info = (ctypes.c_int * 9)()
    assert _lib.load().lav_conv_tile_info(ctypes.byref(d), info) == 0
    assert info[0] == -1 and info[7] >= 200, f"expected the fp16 three-product split plan, got {list(info)}"
    return layer


def conv64(x, w, stride=1, padding=1, transposed=False, output_padding=0):
    """float64 reference (+ sum |w||x|) of the layer on the device."""
    f = (lambda a, b: F.conv_transpose2d(a, b, None, stride, padding, output_padding)) if transposed else \
        (lambda a, b: F.conv2d(a, b, None, stride, padding))
    xd, wd = x.to(DEV).double(), w.to(DEV).double()
    return f(xd, wd), f(xd.abs(), wd.abs()), f


def two_term_bound(x, w, f):
    """2e-6 sum|w||x| + FLOOR_C (q_x sum|w| + q_w sum|x|) over every output's receptive field."""
    xd, wd = x.to(DEV).double(), w.to(DEV).double()
    mag = f(xd.abs(), wd.abs())
    sum_w = f(torch.ones_like(xd), wd.abs())
    sum_x = f(xd.abs(), torch.ones_like(wd))
    return 2e-6 * mag + FLOOR_C * (piece_quantum(x) * sum_w + piece_quantum(w) * sum_x), mag


# ---------------------------------------------------------------------------------------------------------------- A. arithmetic
def test_f16x3_magnitudes_up_to_flt_max(monkeypatch):
    """Activations up to +-FLT_MAX through weights small enough to keep the sums finite (the bf16x6 edge test's case,
    tests/test_gpu_glue.py): finite, 2e-6 of sum |w||x| against float64, and - the scales being powers of two - the same bits as the
    layer on x * 2^-100 scaled back.  The activation scale is 2^113 there and the accumulators reach ~2^32: an epilogue that
    multiplied by the activation scale first overflowed to Inf.  The same through a pad value of -3e38."""
    monkeypatch.setenv("LAV_CONV_SPLIT", "2")
    torch.manual_seed(11)
    cin, cout, H = 64, 64, 24
    w = torch.randn(cout, cin, 3, 3) * 1e-3 / (cin * 9) ** 0.5
    big = torch.empty(1, cin, H, H).uniform_(2.0e38, 3.4e38) * torch.where(torch.rand(1, cin, H, H) < 0.5, -1.0, 1.0)
    big[0, 0, 0, 0], big[0, 1, 3, 3] = FLT_MAX, -FLT_MAX
    layer = f16_layer(w, padding=(1, 1))
    want, mag, _ = conv64(big, w)
    y = layer(big.to(DEV))
    assert torch.isfinite(y).all(), f"{int((~torch.isfinite(y)).sum())} non-finite outputs"
    err = ((y.double() - want).abs() / mag).max().item()
    assert err < 2e-6, f"max |y - ref| / sum|w||x| = {err:.3e}"
    assert torch.equal(y, torch.ldexp(layer((big * 2.0 ** -100).to(DEV)), torch.tensor(100.0, device=DEV)))
    pad = f16_layer(w, padding=(1, 1), pad_value=-3.0e38)
    y_pad = pad(big.to(DEV))
    want_pad = F.conv2d(F.pad(big.double(), (1, 1, 1, 1), value=-3.0e38), w.double(), None, 1, 0).to(DEV)
    mag_pad = F.conv2d(F.pad(big.double().abs(), (1, 1, 1, 1), value=3.0e38), w.double().abs(), None, 1, 0).to(DEV)
    assert torch.isfinite(y_pad).all()
    err = ((y_pad.double() - want_pad).abs() / mag_pad).max().item()
    assert err < 2e-6, f"pad_value -3e38: max |y - ref| / sum|w||x| = {err:.3e}"


def test_f16x3_scale_product_beyond_flt_max(monkeypatch):
    """Activation scale x weight scale = 2^104 x 2^26 > FLT_MAX while every output is finite: the channel near 2^120 meets only
    small weights, the weights near 2^40 read only small activations.  The scales are applied as two factors (never their product):
    the outputs are finite, within the two-term bound of float64, and bit-identical to the same layer on x * 2^-60 scaled back."""
    monkeypatch.setenv("LAV_CONV_SPLIT", "2")
    g = torch.Generator().manual_seed(5)
    cin, cout, H = 16, 32, 24
    sgn = lambda *s: torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)
    x = torch.empty(1, cin, H, H)
    x[:, 0] = torch.empty(1, H, H).uniform_(1.0, 2.0, generator=g) * 2.0 ** 118 * sgn(1, H, H)
    x[:, 1:] = torch.empty(1, cin - 1, H, H).uniform_(1.0, 2.0, generator=g) * 2.0 ** 84 * sgn(1, cin - 1, H, H)
    w = torch.empty(cout, cin, 3, 3)
    w[:, 0] = torch.empty(cout, 3, 3).uniform_(1.0, 2.0, generator=g) * sgn(cout, 3, 3)
    w[:, 1:] = torch.empty(cout, cin - 1, 3, 3).uniform_(0.5, 1.0, generator=g) * 2.0 ** 30 * sgn(cout, cin - 1, 3, 3)
    w[0, 1, 1, 1] = 2.0 ** 40
    assert f16_scale(x.abs().max().item()) * f16_scale(w.abs().max().item()) > FLT_MAX
    layer = f16_layer(w, padding=(1, 1))
    want, _, f = conv64(x, w)
    assert want.abs().max().item() < FLT_MAX / 4
    y = layer(x.to(DEV))
    assert torch.isfinite(y).all(), f"{int((~torch.isfinite(y)).sum())} non-finite outputs"
    bound, _ = two_term_bound(x, w, f)
    excess = ((y.double() - want).abs() / bound).max().item()
    assert excess <= 1.0, f"beyond the two-term bound by x{excess:.3f}"
    assert torch.equal(y, torch.ldexp(layer((x * 2.0 ** -60).to(DEV)), torch.tensor(60.0, device=DEV)))


def test_f16x3_degenerate_scales(monkeypatch):
    """All-zero weights (their scale word is 1) give exactly the epilogue of a zero sum; weights whose maximum is below 2^-100 and
    activations whose maximum is below 2^-100 or subnormal take the exponent floor (scale 2^-115): finite, no Inf from the
    reciprocal, within the two-term bound of float64 (the 2e-6 bar where the floor costs no bits)."""
    monkeypatch.setenv("LAV_CONV_SPLIT", "2")
    g = torch.Generator().manual_seed(7)
    cin, cout, H = 64, 64, 24
    x = torch.randn(1, cin, H, H, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / 24
    bias = torch.randn(cout, generator=g)
    # all-zero weights: y = bias exactly
    zl = f16_layer(torch.zeros(cout, cin, 3, 3), padding=(1, 1), bias=bias)
    yz = zl(x.to(DEV))
    assert torch.equal(yz, bias.to(DEV)[None, :, None, None].expand_as(yz))
    # weights below 2^-100 (largest ~2^-108): scale floored at 2^-115, values scaled to ~2^7 - no bits lost
    wt = w * 2.0 ** -110
    want, mag, f = conv64(x, wt)
    y = f16_layer(wt, padding=(1, 1))(x.to(DEV))
    assert torch.isfinite(y).all()
    err = ((y.double() - want).abs() / mag).max().item()
    assert err < 2e-6, f"weights below 2^-100: {err:.3e} of sum|w||x|"
    # activations below 2^-100 (largest ~2^-108), weights large enough for normal outputs
    wl = w * 2.0 ** 20
    for label, xs in (("below 2^-100", x * 2.0 ** -110),
                      ("subnormal", torch.empty(1, cin, H, H).uniform_(1e-45, 1.1e-38, generator=g) * torch.sign(x))):
        assert torch.isfinite(xs).all() and xs.abs().max().item() < 2.0 ** -100
        want, mag, f = conv64(xs, wl)
        y = f16_layer(wl, padding=(1, 1))(xs.to(DEV))
        assert torch.isfinite(y).all(), label
        bound, _ = two_term_bound(xs, wl, f)
        excess = ((y.double() - want).abs() / bound).max().item()
        assert excess <= 1.0, f"activations {label}: beyond the two-term bound by x{excess:.3f}"
    # all-zero activations
    y0 = f16_layer(w, padding=(1, 1), bias=bias)(torch.zeros(1, cin, H, H, device=DEV))
    assert torch.equal(y0, bias.to(DEV)[None, :, None, None].expand_as(y0))


def test_f16x3_keeps_subnormal_activations(monkeypatch):
    """What f16x3 does with fp32 subnormals (bf16x6 flushes them: tests/test_gpu_glue.py): the activations are divided by their
    power-of-two scale on the vector ALU, which keeps subnormals, so they survive wherever the scaled value is above fp16's subnormal
    quantum - i.e. when the tensor's largest value is small.  Here the tensor's maximum is ~2^-110 (normal), a band of the image holds
    only subnormals: the outputs that read only that band are those of the unflushed input (two-term bound), not zero."""
    monkeypatch.setenv("LAV_CONV_SPLIT", "2")
    g = torch.Generator().manual_seed(9)
    cin, cout, H = 64, 64, 24
    x = torch.empty(1, cin, H, H).uniform_(0.5, 1.0, generator=g) * 2.0 ** -110
    x[..., 12:] = torch.empty(1, cin, H, 12).uniform_(2.0 ** -140, 2.0 ** -127, generator=g)
    x *= torch.where(torch.rand(x.shape, generator=g) < 0.5, -1.0, 1.0)
    assert (x[..., 12:].abs() < torch.finfo(torch.float32).tiny).all()
    w = torch.randn(cout, cin, 3, 3, generator=g) * 2.0 ** 40
    want, mag, f = conv64(x, w)
    flushed = torch.where(x.abs() < torch.finfo(torch.float32).tiny, torch.zeros_like(x), x)
    want_flushed, _, _ = conv64(flushed, w)
    y = f16_layer(w, padding=(1, 1))(x.to(DEV)).double()
    assert torch.isfinite(y).all()
    sub = y[..., 14:]                 # outputs that read only subnormal inputs
    assert (want_flushed[..., 14:] == 0).all()
    assert (sub != 0).float().mean().item() > 0.99, "subnormal activations were flushed"
    bound, _ = two_term_bound(x, w, f)
    excess = ((y - want).abs() / bound).max().item()
    assert excess <= 1.0, f"beyond the two-term bound of the unflushed input by x{excess:.3f}"


# the 3x3 stride-1, split-K and transposed plans of tests/test_gpu_conv.py F16_CASES
PLAN_CASES = [
    # name, B, cin, cout, k, stride, pad, transposed, out_pad, H, W, LAV_SPLIT_FORCE
    ("BEV 128->128 80x80", 1, 128, 128, 3, 1, 1, False, 0, 80, 80, ""),
    ("brake 512->512 9x24 (split-K)", 1, 512, 512, 3, 1, 1, False, 0, 9, 24, ""),
    ("up-convolution 4x4 s2 (four parity classes)", 1, 128, 128, 4, 2, 1, True, 0, 80, 80, ""),
]


def _plan_layer(case, w, monkeypatch, **kw):
    name, B, cin, cout, k, s_, p_, tr, op, H, W, force = case
    return f16_layer(w, monkeypatch, force, B, H, W, stride=s_, padding=(p_, p_), transposed=tr, output_padding=op, **kw)


def _reach(case, mask):
    """Outputs whose receptive field touches `mask` (B, 1, H, W) - float64 convolution with an all-ones kernel."""
    name, B, cin, cout, k, s_, p_, tr, op, H, W, force = case
    ones = torch.ones(1, 1, k, k, dtype=torch.float64, device=DEV)
    m = mask.to(DEV).double()
    r = F.conv_transpose2d(m, ones, None, s_, p_, op) if tr else F.conv2d(m, ones, None, s_, p_)
    return r[:, 0] > 0


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_f16x3_nan_and_inf_stay_local(case, monkeypatch):
    """A NaN and an Inf activation make every output they reach non-finite; neither changes the activation scale (the maxima are
    of the FINITE values), so every other output keeps the bits of a run where both are zero."""
    name, B, cin, cout, k, s_, p_, tr, op, H, W, force = case
    g = torch.Generator().manual_seed(13)
    w = torch.randn((cin, cout, k, k) if tr else (cout, cin, k, k), generator=g) / (cin * k * k) ** 0.5
    layer = _plan_layer(case, w, monkeypatch)
    x = torch.randn(B, cin, H, W, generator=g)
    bad = [(0, 3, H // 3, W // 4, float("inf")), (0, cin - 2, 2 * H // 3, 3 * W // 4, float("nan"))]
    xb, clean = x.clone(), x.clone()
    mask = torch.zeros(B, 1, H, W)
    for b, c, i, j, v in bad:
        xb[b, c, i, j], clean[b, c, i, j] = v, 0.0
        mask[b, 0, i, j] = 1.0
    y, y0 = layer(xb.to(DEV)), layer(clean.to(DEV))
    reach = _reach(case, mask)[:, None].expand_as(y)
    assert reach.any() and (~reach).any()
    assert not torch.isfinite(y[reach]).any(), f"{name}: a NaN / Inf input came out as a finite number"
    assert torch.equal(y[~reach], y0[~reach]), f"{name}: outputs the non-finite inputs do not reach changed"


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_f16x3_dynamic_range(case, monkeypatch):
    """Per-element error when a tensor spans many decades.  One scale per tensor puts its largest value at 2^14..2^15 in fp16 units,
    so a value loses what lies below fp16's subnormal quantum: absolute error 2^-25 x scale ~ 2^-40..2^-39 of the tensor's maximum.
    Outputs that read only values far below the maximum therefore miss the 2e-6 of sum |w||x| bar; they keep the two-term bound
    2e-6 sum|w||x| + C (q_x sum|w| + q_w sum|x|).  Measured here: activations in bands at 2^0, 2^-10, 2^-20, 2^-30 of the maximum
    (the bands down to 2^-20 keep the 2e-6 bar, the 2^-30 band does not); then weights with one large entry and the rest 2^-30 of it."""
    name, B, cin, cout, k, s_, p_, tr, op, H, W, force = case
    g = torch.Generator().manual_seed(17)
    levels = [0, -10, -20, -30]
    edges = np.linspace(0, W, len(levels) + 1).astype(int)
    lvl = torch.zeros(W)
    for i, lv in enumerate(levels):
        lvl[edges[i]:edges[i + 1]] = 2.0 ** lv
    sgn = lambda *s: torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)
    x = torch.empty(B, cin, H, W).uniform_(0.5, 1.0, generator=g) * lvl * sgn(B, cin, H, W)
    wshape = (cin, cout, k, k) if tr else (cout, cin, k, k)
    w = torch.randn(wshape, generator=g) / (cin * k * k) ** 0.5
    want, mag, f = conv64(x, w, s_, p_, tr, op)
    y = _plan_layer(case, w, monkeypatch)(x.to(DEV)).double()
    bound, _ = two_term_bound(x, w, f)
    report = []
    for i, lv in enumerate(levels):
        m = torch.zeros(B, 1, H, W); m[..., edges[i]:edges[i + 1]] = 1.0
        others = _reach(case, 1.0 - m)                         # outputs that read any other band
        pure = (_reach(case, m) & ~others)[:, None].expand_as(y)
        assert pure.any()
        e = (y - want).abs()[pure]
        rel = (e / mag[pure]).max().item()
        fl = (e / bound[pure]).max().item()
        report.append((lv, rel, fl))
        assert fl <= 1.0, f"{name}: band 2^{lv} beyond the two-term bound: {rel:.3e} of sum|w||x|, x{fl:.3f} of the bound"
        if lv >= -20:
            assert rel < 2e-6, f"{name}: band 2^{lv} (within 2^-20 of the maximum) must keep the 2e-6 bar: {rel:.3e}"
    print(name, "activation bands (level, err / sum|w||x|, err / two-term bound):", [(a, f"{b:.2e}", f"{c:.3f}") for a, b, c in report])
    assert report[-1][1] > 2e-6, f"{name}: 2^-30 band within 2e-6 ({report[-1][1]:.2e}): the precision text overstates the loss"
    # the weights: one large entry, every other 2^-30 of it
    x1 = torch.randn(B, cin, H, W, generator=g)
    w1 = torch.randn(wshape, generator=g) * 2.0 ** -30 / (cin * k * k) ** 0.5
    w1.view(-1)[7] = 1.0
    want, mag, f = conv64(x1, w1, s_, p_, tr, op)
    y = _plan_layer(case, w1, monkeypatch)(x1.to(DEV)).double()
    bound, _ = two_term_bound(x1, w1, f)
    e = (y - want).abs()
    fl = (e / bound).max().item()
    print(name, f"one large weight: err / sum|w||x| {(e / mag).max().item():.2e}, err / two-term bound {fl:.3f}")
    assert fl <= 1.0, f"{name}: one large weight: beyond the two-term bound (x{fl:.3f})"


def test_f16x3_weight_gradient_dynamic_range():
    """lav_conv_wgrad_amax (the weight gradient on two fp16 pieces per operand) with dy spanning eight decades: dy in bands at 2^0,
    2^-10, 2^-20 .. 2^-26 of its maximum (channels), x ordinary.  Each weight's error stays within the two-term bound
    2e-6 sum|dy||x| + C (q_dy sum|x| + q_x sum|dy|); the channels within ten octaves of the maximum keep the 2e-6 bar."""
    from lav_amd.ops import _ptr, _stream, _workspace, check
    lib = _lib.load()
    B, cin, cout, H, W, S, KS = 2, 64, 64, 20, 32, 1, 3
    g = torch.Generator().manual_seed(19)
    x = torch.randn((B, cin, H, W), generator=g)
    lv = torch.tensor([0.0, -10.0, -20.0, -26.6]).repeat_interleave(cout // 4)     # 2^-26.6 = 1e-8: eight decades
    dy = torch.empty((B, cout, H, W)).uniform_(0.5, 1.0, generator=g) * torch.exp2(lv)[None, :, None, None]
    dy *= torch.where(torch.rand(dy.shape, generator=g) < 0.5, -1.0, 1.0)
    wg = lambda a, b: torch.nn.grad.conv2d_weight(a, (cout, cin, KS, KS), b, stride=S, padding=KS // 2)
    ref, mag = wg(x.double(), dy.double()), wg(x.double().abs(), dy.double().abs())
    sum_x = wg(x.double().abs(), torch.ones_like(dy, dtype=torch.float64))
    sum_dy = wg(torch.ones_like(x, dtype=torch.float64), dy.double().abs())
    xd, dyd = x.to(DEV), dy.to(DEV)
    ax, ay = torch.zeros(512, device=DEV), torch.zeros(512, device=DEV)
    check(lib.lav_absmax_parts(_ptr(xd), xd.numel(), _ptr(ax), _stream()), "lav_absmax_parts")
    check(lib.lav_absmax_parts(_ptr(dyd), dyd.numel(), _ptr(ay), _stream()), "lav_absmax_parts")
    nbytes = lib.lav_conv_wgrad_workspace_bytes(B, cin, cout, H, W, KS, S)
    assert nbytes > 0
    ws = _workspace("conv_wgrad_test", nbytes, DEV)
    dw = torch.full((cout, cin, KS, KS), float("nan"), device=DEV)
    check(lib.lav_conv_wgrad_amax(_ptr(xd), _ptr(dyd), B, cin, cout, H, W, KS, S, _ptr(dw), _ptr(ws), ws.numel(), _ptr(ax), 512, _ptr(ay), 512,
                                  _stream()), "lav_conv_wgrad_amax")
    e = (dw.cpu().double() - ref).abs()
    floor = FLOOR_C * (piece_quantum(dy) * sum_x + piece_quantum(x) * sum_dy)
    rel = [(e[i * 16:(i + 1) * 16] / mag[i * 16:(i + 1) * 16]).max().item() for i in range(4)]
    fl = (e / (2e-6 * mag + floor)).max().item()
    print("weight gradient, dy bands 2^0 / 2^-10 / 2^-20 / 2^-26.6: err / sum|dy||x|", [f"{r:.2e}" for r in rel], f"err / two-term bound {fl:.3f}")
    assert fl <= 1.0, f"beyond the two-term bound (x{fl:.3f})"
    assert rel[0] < 2e-6 and rel[1] < 2e-6, rel


# ---------------------------------------------------------------------------------------------------------------- B. stale bounds
def _homogeneous_lidar_model(seed=3):
    """A LiDARModel whose eval network is positively homogeneous: bias-free convolutions, BatchNorm at its initial statistics
    (identity up to 1/sqrt(1 + eps)), so the feature map of x * 2^-k is the feature map of x times 2^-k.  Its PointNet reads only the
    intensity column, without biases: the canvas scales with the intensities."""
    torch.manual_seed(seed)
    import lav_amd
    lm = lav_amd.LiDARModel(num_input=16, backbone="cnn", num_features=[64, 64], **CFG)
    with torch.no_grad():
        for m in lm.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                torch.nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
        lins = [m for m in lm.point_pillar_net.point_net.net if isinstance(m, torch.nn.Linear)]
        lins[0].weight.zero_(); lins[0].weight[:, 3] = torch.rand(lins[0].weight.shape[0]) + 0.5
        lins[1].weight.abs_()
        for lin in lins:
            lin.bias.zero_()
    return lm.eval().to(DEV)


def _heads64(lm, f):
    """float64 reference of the four heads on the feature map f (the nn modules' arithmetic), with the largest |pre-activation|."""
    out = []
    fd = f.double()
    for n in lm.ALL_HEADS:
        h = getattr(lm, n)
        conv, bn, ct = h.net[0], h.net[2], h.net[3]
        t = F.relu(F.conv2d(fd, conv.weight.double(), None, 1, 1))
        t = F.batch_norm(t, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.0, bn.eps)
        t = F.conv_transpose2d(t, ct.weight.double(), ct.bias.double(), 2, 1, 1)
        out.append((torch.sigmoid(t) if h._sigmoid else t, t.abs().max().item()))
    return out


def _assert_heads(lm, heads, f, what):
    for n, y, (r, zmax) in zip(lm.ALL_HEADS, heads, _heads64(lm, f)):
        assert torch.isfinite(y).all(), f"{what}: {n} holds {int((~torch.isfinite(y)).sum())} non-finite values"
        # 1e-4 of the largest pre-activation, through the sigmoid's slope (at most 1/4) for the segmentation head
        tol = 1e-4 * (0.25 * zmax if getattr(lm, n)._sigmoid else zmax) + 1e-4 * r.abs()
        assert ((y.double() - r).abs() <= tol).all(), f"{what}: {n} differs from float64 by {(y.double() - r).abs().max().item():.3e}"


def test_stale_backbone_bound_is_not_trusted():
    """f1 = backbone(x); backbone(x * 2^-12) of the same shape rewrites the Amax f1 was tagged with (its maxima now 2^12 too small
    for f1): the heads on f1 must measure f1 instead - finite, the bits of the heads on an untagged copy, float64 within 1e-4."""
    lm = _homogeneous_lidar_model()
    x = torch.rand((1, 64, lm.point_pillar_net.ny, lm.point_pillar_net.nx), device=DEV)
    with torch.no_grad(), ops.precision(_lib.CONV_F16X3):
        e = lm.backbone._engine(DEV)
        assert e["s1"][0].uses_amax(1, x.shape[2], x.shape[3])
        f1 = lm.backbone(x)
        ref = lm.heads(f1.clone())
        assert ops.amax_of(f1) is not None, "a fresh feature map must carry its bound"
        f2 = lm.backbone(x * 2.0 ** -12)
        assert ops.amax_of(f2) is not None
        heads = lm.heads(f1)
    _assert_heads(lm, heads, f1, "heads on a feature map whose bound was rewritten")
    for a, b in zip(heads, ref):
        assert torch.equal(a, b)


def test_in_place_change_voids_the_bound():
    """f1.mul_(2^12) after the backbone: f1's bound is 2^12 too small; the heads must measure f1."""
    lm = _homogeneous_lidar_model()
    x = torch.rand((1, 64, lm.point_pillar_net.ny, lm.point_pillar_net.nx), device=DEV)
    with torch.no_grad(), ops.precision(_lib.CONV_F16X3):
        f1 = lm.backbone(x)
        f1.mul_(2.0 ** 12)
        heads = lm.heads(f1)
        ref = lm.heads(f1.clone())
    _assert_heads(lm, heads, f1, "heads on a feature map changed in place")
    for a, b in zip(heads, ref):
        assert torch.equal(a, b)


def test_stale_canvas_bound_is_not_trusted():
    """Two PointPillarNet calls of the same batch size share one Amax: the first canvas's bound is rewritten by the second (whose
    intensities, and so canvas, are 2^12 smaller); the backbone on the first canvas must measure it."""
    lm = _homogeneous_lidar_model()
    pts = torch.from_numpy(synth.stacked_lidar(8192)).to(DEV)
    pts[:, 3] = pts[:, 3].abs() + 0.25
    dim = pts.clone(); dim[:, 3] *= 2.0 ** -12
    with torch.no_grad(), ops.precision(_lib.CONV_F16X3):
        c1 = lm.point_pillar_net([pts], [len(pts)])
        assert ops.amax_of(c1) is not None
        ref = lm.backbone(c1.clone())
        c2 = lm.point_pillar_net([dim], [len(dim)])
        assert c2.max().item() < c1.max().item() * 2.0 ** -11
        f = lm.backbone(c1)
    assert torch.isfinite(f).all(), f"backbone on a canvas whose bound was rewritten: {int((~torch.isfinite(f)).sum())} non-finite values"
    assert torch.equal(f, ref)


def test_crop_of_a_stale_feature_map_is_measured():
    """A crop taken from a feature map whose bound has since been rewritten carries no bound: the ResNet stem measures it."""
    lm = _homogeneous_lidar_model()
    _, up = build_models(DEV)
    x = torch.rand((1, 64, lm.point_pillar_net.ny, lm.point_pillar_net.nx), device=DEV)
    trunk = up.lidar_conv_emb[0]
    locs, oris = torch.tensor([[3.0, -8.0]], device=DEV), torch.tensor([0.4], device=DEV)
    with torch.no_grad(), ops.precision(_lib.CONV_F16X3):
        f1 = lm.backbone(x)
        lm.backbone(x * 2.0 ** -12)
        crops = up.crop_feature(f1, locs, oris, up.pixels_per_meter / 2, up.crop_size, amax=ops.amax_of(f1))
        y = trunk(crops)
        ref = trunk(crops.clone())
    assert torch.isfinite(y).all(), f"ResNet on the crop of a stale feature map: {int((~torch.isfinite(y)).sum())} non-finite values"
    assert torch.equal(y, ref)


def test_amax_generation_and_version_stamps():
    """ops.tag_amax / amax_of: a tag holds until the tensor changes in place or its Amax is reset; untagged tensors have none."""
    am = ops.Amax(DEV, capacity=16)
    t = torch.zeros(4, device=DEV)
    assert ops.amax_of(t) is None
    ops.tag_amax(t, am.reset())
    assert ops.amax_of(t) is am
    t.add_(1.0)
    assert ops.amax_of(t) is None
    ops.tag_amax(t, am)
    assert ops.amax_of(t) is am
    am.reset()
    assert ops.amax_of(t) is None


def _spy_amax_of(monkeypatch):
    calls = []
    real = ops.amax_of

    def spy(t):
        r = real(t)
        calls.append((getattr(t, "_lav_amax", None) is not None, r is not None))
        return r
    monkeypatch.setattr(ops, "amax_of", spy)
    return calls


def test_hand_off_stays_on_in_infer_model(monkeypatch):
    """InferModel.forward: every consumer handed a tagged tensor (backbone <- canvas, heads <- feature map, crops <- feature map,
    ResNet stems <- crops) still receives its bound."""
    import lav_amd
    lm, up = build_models(DEV)
    im = lav_amd.InferModel(lm, up, 1.5, 2.4, device=DEV)
    assert im.precision == _lib.CONV_F16X3
    pts = torch.from_numpy(synth.stacked_lidar(8192)).to(DEV)
    calls = _spy_amax_of(monkeypatch)
    out = im(pts, torch.tensor([0.0, -10.0], device=DEV), 3)
    torch.cuda.synchronize()
    assert torch.isfinite(out[1]).all()
    tagged = [ok for has, ok in calls if has]
    assert len(tagged) >= 4, f"expected the canvas, the feature map (twice) and the ego crop to carry bounds: {calls}"
    assert all(tagged), f"{tagged.count(False)} of {len(tagged)} tagged tensors lost their bound: {calls}"


def _frame_models():
    from lav_amd.rgb import RGBBrakePredictionModel, RGBSegmentationModel
    lm, up = build_models(DEV)
    seg = RGBSegmentationModel([4, 6, 7, 10]); seg.load_state_dict(synth.seeded_state_dict(seg, prefix="seg.")); seg.eval().to(DEV)
    bra = RGBBrakePredictionModel([4, 6, 7, 10]); bra.load_state_dict(synth.seeded_state_dict(bra, prefix="bra.")); bra.eval().to(DEV)
    cams, tel = synth.rgb_frames()
    rgbs = [c[..., :3][..., ::-1] for c in cams]
    all_rgb = torch.tensor(np.stack(rgbs, 0).copy()).permute(0, 3, 1, 2).float().to(DEV)
    wide = torch.tensor(np.concatenate(rgbs, axis=1)[None].copy()).permute(0, 3, 1, 2).float().to(DEV)
    tel_rgb = torch.tensor(tel[..., :3][..., ::-1][:-96][None].copy()).permute(0, 3, 1, 2).float().to(DEV)
    return lm, up, seg, bra, (all_rgb, wide, tel_rgb)


def test_hand_off_stays_on_in_the_graphed_frame(monkeypatch):
    """GraphedFramePipeline (device-resident others branch): while the graphs are captured every consumer handed a tagged tensor
    receives its bound - the hand-off is baked into the graphs as it was."""
    from lav_amd.frame import GraphedFramePipeline
    lm, up, seg, bra, cams = _frame_models()
    calls = _spy_amax_of(monkeypatch)
    pipe = GraphedFramePipeline(lm, up, seg, bra, 1.5, 2.4, device=DEV, points_per_tick=8192)
    nxp = torch.tensor([1.0, -9.0], device=DEV)
    for i in range(3):
        tick = torch.from_numpy(synth.lidar_sweep(8192, name=f"c{i}")).to(DEV)
        pipe.step(tick, *cams, np.array([0.3 * i, 0.05 * i]), 0.02 * i, nxp, 3)
    torch.cuda.synchronize()
    tagged = [ok for has, ok in calls if has]
    # lidar (canvas), heads, ego (feature map, crop), others (feature map, crops): each run once eagerly and once captured
    assert len(tagged) >= 12, calls
    assert all(tagged), f"{tagged.count(False)} of {len(tagged)} tagged tensors lost their bound: {calls}"


# ---------------------------------------------------------------------------------------------------------------- C. per stream
def _amax_buffers_per_call(monkeypatch, fn, streams):
    """Device addresses of the Amax buffers that fn() resets, once per stream."""
    seen = []
    real = ops.Amax.reset

    def spy(self):
        seen[-1].add(self.buf.data_ptr())
        return real(self)
    monkeypatch.setattr(ops.Amax, "reset", spy)
    for s in streams:
        seen.append(set())
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops.Amax, "reset", real)
    return seen


def _disjoint_lists(amax_lists):
    """The engine's Amax lists (one per input shape and stream): two of them, no buffer in both."""
    lists = list(amax_lists.values())
    assert len(lists) == 2, f"{len(lists)} Amax list(s) for two streams"
    a, b = ({am.buf.data_ptr() for am in lst} for lst in lists)
    assert not (a & b), f"{len(a & b)} Amax buffers shared by the two streams"


def test_resnet_trunk_keeps_one_bound_per_stream(monkeypatch):
    """The ego graph (s_ego) and a one-vehicle others graph (s_cap) run the ResNet trunk concurrently on crop batches of the same
    shape (1, 384, 96, 96): the buffers its layers leave maxima in for each other are allocated per stream.  (At this shape only the
    stem runs on the fp16 split plan and it reads the crops' bound, so no layer of the trunk writes them yet.)"""
    _, up = build_models(DEV)
    trunk = up.lidar_conv_emb[0]
    x = torch.rand((1, 384, 96, 96), device=DEV)
    with torch.no_grad(), ops.precision(_lib.CONV_F16X3):
        _amax_buffers_per_call(monkeypatch, lambda: trunk(x), [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)])
        _disjoint_lists(trunk._eng[("trunk", _lib.CONV_F16X3)]["amax"])


def test_backbone_keeps_one_bound_per_stream(monkeypatch):
    """The BEV backbone on one input shape under two streams: every layer's maxima go to buffers of the stream's own."""
    lm, _ = build_models(DEV)
    x = torch.rand((1, 64, lm.point_pillar_net.ny, lm.point_pillar_net.nx), device=DEV)
    with torch.no_grad(), ops.precision(_lib.CONV_F16X3):
        a, b = _amax_buffers_per_call(monkeypatch, lambda: lm.backbone(x), [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)])
        _disjoint_lists(lm.backbone._eng[("backbone", _lib.CONV_F16X3)]["amax"])
    assert a and b, "the backbone's layers leave maxima for each other"
    assert not (a & b), f"{len(a & b)} Amax buffers written on both streams"


def test_concurrent_ego_and_one_vehicle_graphs_match_serial_replays():
    """device_others=False: the ego graph and the ("others", 1) graph - whose crop batch has the ego's shape - replayed concurrently
    on s_ego and s_cap, as step() does, give the ego outputs of serial replays bit for bit, over 8 frames with different inputs.
    (Timing dependent: the white-box tests above are the ones that must fail when the two share their bounds.)"""
    from lav_amd.frame import GraphedFramePipeline
    lm, up, seg, bra, cams = _frame_models()
    pipe = GraphedFramePipeline(lm, up, seg, bra, 1.5, 2.4, device=DEV, points_per_tick=8192, device_others=False)
    assert not pipe.device_others
    nxp = torch.tensor([1.0, -9.0], device=DEV)
    main = torch.cuda.current_stream()
    keys = ("ego_embd", "ego_cast_locs", "ego_plan_locs")

    def one_vehicle():
        pipe.hn_actors[:] = 0
        pipe.hn_actors[:2] = (5.0, -10.0)
        pipe.hn_actors[30] = 0.3
        pipe.d_actors.copy_(pipe.h_actors)
        torch.cuda.synchronize()
    with torch.no_grad():
        for i in range(10):
            tick = torch.from_numpy(synth.lidar_sweep(8192, name=f"s{i}")).to(DEV)
            pipe.step(tick, *cams, np.array([0.3 * i, 0.05 * i]), 0.02 * i, nxp, 3)
            torch.cuda.synchronize()
            if i < 2:
                continue
            one_vehicle()
            with ops.precision(pipe.precision):
                with torch.cuda.stream(pipe.s_ego):
                    pipe._replay(("ego", 3), pipe._g_ego, pipe.s_ego, 3)
                pipe._replay(("others", 1), pipe._g_others, pipe.s_cap, 1)
            torch.cuda.synchronize()
            g_ego, g_oth = pipe.graphs[("ego", 3)], pipe.graphs[("others", 1)]
            out = pipe.outs[("ego", 3)]
            with torch.cuda.stream(pipe.s_ego):
                g_ego.replay()
            torch.cuda.synchronize()
            serial = {k: out[k].clone() for k in keys}
            with torch.cuda.stream(pipe.s_cap):
                g_oth.replay()
            torch.cuda.synchronize()
            ev = torch.cuda.Event()
            ev.record(main)
            pipe.s_ego.wait_event(ev); pipe.s_cap.wait_event(ev)
            with torch.cuda.stream(pipe.s_ego):
                g_ego.replay()
            with torch.cuda.stream(pipe.s_cap):
                g_oth.replay()
            torch.cuda.synchronize()
            for k in keys:
                assert torch.equal(out[k], serial[k]), f"frame {i}: {k} of the concurrent replay differs from the serial one"
