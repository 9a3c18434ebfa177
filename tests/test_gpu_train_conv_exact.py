"""The training convolutions bit for bit: one autograd step of lav_amd.train.hipnn.conv2d - forward on lav_conv2d over the live
parameter, data gradient on the transposed lav_conv2d plan over the same weight tensor, weight gradient on lav_conv_wgrad /
lav_conv_wgrad_amax - on class-A data of tests/exact_util.py (integers on every side, partial sums below 2^24; checked on the host by
tests/test_conv_exact_host.py), where the float64 result is the only correct answer at both training precisions.  Every leg the
library computes is held to torch.equal with float64; a leg the glue hands to torch (E.TRAIN_CONV_GEOMS says which, by the conditions
of _Conv2d.backward and _wgrad_hip) keeps the bar of tests/test_gpu_train.py - 1e-4 of the largest reference value: MIOpen's Winograd
solvers need not be exact on integers - and the test checks that each leg ran where the geometry says.

What a failing leg points at: y the forward plan or the repack; dx the transposed plan (parity classes, output padding, borders) or
the torch fall-backs of the glue; dw the weight-gradient kernels or the am_x / am_dy hand-off between the three legs."""
import ctypes

import pytest
import torch

from lav_amd import _lib, ops
from lav_amd.train import hipnn
from tests import exact_util as E
from tests.exact_util import BF16X6, F16X3, assert_exact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PREC = {BF16X6: _lib.CONV_BF16X6, F16X3: _lib.CONV_F16X3}
SPLITS = (None, "2")
KNOBS = ("LAV_TRAIN_CONV", "LAV_TRAIN_CONVT", "LAV_TRAIN_DGRAD", "LAV_TRAIN_DGRAD_STRIDED", "LAV_TRAIN_WGRAD", "LAV_TRAIN_WGRAD_STRIDED",
         "LAV_TRAIN_WGRAD_STEM", "LAV_TRAIN_WGRAD_F16", "LAV_SPLIT_FORCE", "LAV_CONV_SPLIT")
_cases: dict = {}


def cached(make, *key):
    """(case, float64 references), computed once and shared by the precisions and plans."""
    if key not in _cases:
        case = make(*key)
        _cases[key] = (case, case.forward(E.Plain()))
    return _cases[key]


def set_knobs(monkeypatch, precision, split, env=()):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setenv("LAV_TRAIN_PRECISION", precision)
    monkeypatch.setenv("LAV_TRAIN_WGRAD_MINPIX", "1")
    if split is not None:
        monkeypatch.setenv("LAV_CONV_SPLIT", split)
    for name, value in env:
        monkeypatch.setenv(name, value)
    hipnn._CONV_ENGINES.clear()


def handed_in(t, factor):
    """An Amax as a producer leaves it (test_gpu_conv_exact.py's): parts whose maximum is factor * max |t|."""
    am = ops.Amax(DEV)
    parts = am.take(7)
    parts.zero_()
    parts[3] = float(t.detach().abs().max()) * factor
    parts[5] = 2.0 ** -30
    return am


def within_the_torch_bar(got, want, what):
    """tests/test_gpu_train.py's bar for a leg torch computes: 1e-4 of the largest reference value."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    err, tol = float((got - want).abs().max()), 1e-4 * float(want.abs().max())
    assert err < tol, f"{what} (torch): worst |difference| {err:.6g} >= {tol:.6g}"


def check_leg(got, want, who, what):
    if who == "lib":
        assert_exact(got, want, what)
    else:
        within_the_torch_bar(got, want, what)


def plan_of(desc, B, h, w):
    """lav_conv_tile_info of a layer descriptor on a (B, ., h, w) input."""
    d = _lib.Conv.from_buffer_copy(desc)
    d.batch, d.h, d.w = B, h, w
    info = (ctypes.c_int * 9)()
    assert _lib.load().lav_conv_tile_info(ctypes.byref(d), info) == 0, _lib.load().lav_last_error().decode()
    return list(info)


def dgrad_plan(g, case, precision):
    """The plan of the data gradient's transposed layer, from the geometry alone (under the knobs of the moment)."""
    B, cout, oh, ow = case.dy.shape
    d = _lib.Conv(B, cout, 0, cout, oh, ow, g.cin, g.kh, g.kw, g.stride, g.ph, g.pw, 1, 1, 1, case.out_pad[0], g.cin, 0, 0, 0, 0, 0, 0.0, PREC[precision])
    return plan_of(d, B, oh, ow)


def engines(kind):
    return [eng for key, eng in hipnn._CONV_ENGINES.items() if key[0] == kind]


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: f"split {s}")
@pytest.mark.parametrize("precision", [BF16X6, F16X3])
@pytest.mark.parametrize("g", E.TRAIN_CONV_GEOMS, ids=lambda g: g.name)
def test_training_convolution_step_is_exact(g, precision, split, monkeypatch):
    """y, dx and dw of one step; who took each leg; a second step after the weight doubled in place (the repack sees the live weights);
    at f16x3 the measurements - at most one per tensor and step - and a third step on handed-in bounds 4x above the maxima: the same
    bits, nothing measured."""
    set_knobs(monkeypatch, precision, split, g.env)
    case, (y64, dx64, dw64) = cached(E.TrainConvCase, g)
    x = case.x.to(DEV).requires_grad_(g.x_grad)
    w = case.w.to(DEV).requires_grad_(True)
    dy = case.dy.to(DEV)

    def step(x, dy, scale, what):
        """One step; the references are those of the drawn weights times `scale` (dw does not depend on w)."""
        flops, measured = ops.train_work.get("conv_wgrad_flops", 0), ops.train_work.get("absmax_launches", 0)
        y = hipnn.conv2d(x, w, g.stride, (g.ph, g.pw), (g.dh, g.dw))
        assert type(y.grad_fn).__name__.startswith(hipnn._Conv2d.__name__), "the liblav_amd function must be the one that ran"
        grads = torch.autograd.grad(y, (x, w) if g.x_grad else (w,), dy)
        torch.cuda.synchronize()
        assert_exact(y, y64 * scale, f"{what}: y")
        if g.x_grad:
            check_leg(grads[0], dx64 * scale, g.dgrad, f"{what}: dx")
        check_leg(grads[-1], dw64, g.wgrad, f"{what}: dw")
        assert (ops.train_work.get("conv_wgrad_flops", 0) > flops) == (g.wgrad == "lib"), f"{what}: the weight gradient did not run on {g.wgrad}"
        assert {key[0] for key in hipnn._CONV_ENGINES} == {"fwd"} | ({"dgrad"} if g.dgrad == "lib" else set()), f"{what}: the data gradient did not run on {g.dgrad}"
        return ops.train_work.get("absmax_launches", 0) - measured

    what = f"{case.name} at {precision}, LAV_CONV_SPLIT {split}"
    measured = step(x, dy, 1.0, what)
    if g.dgrad == "lib":
        eng, = engines("dgrad")
        assert plan_of(eng.desc, *dy.shape[:1], *dy.shape[2:]) == dgrad_plan(g, case, precision), f"{what}: the data gradient's layer is not the geometry's"
    with torch.no_grad():
        w.mul_(2.0)
    measured2 = step(x, dy, 2.0, what + ", the weight doubled in place")
    if precision != F16X3:
        assert measured == measured2 == 0
        return
    assert 0 <= measured <= 2 and 0 <= measured2 <= 2, f"{what}: {measured}, {measured2} measurements for two tensors per step"
    x3, dy3 = x.detach().clone().requires_grad_(g.x_grad), dy.clone()
    ops.tag_amax(x3, handed_in(x3, 4.0))
    ops.tag_amax(dy3, handed_in(dy3, 4.0))
    assert step(x3, dy3, 2.0, what + ", bounds 4x above the maxima handed in") == 0, f"{what}: a tensor with a handed-in bound was measured"


@pytest.mark.parametrize("precision", [BF16X6, F16X3])
def test_data_gradients_reach_the_split_kernel_and_another_plan(precision, monkeypatch):
    """Over the list and the two LAV_CONV_SPLIT settings of the step test, the transposed layers of the data gradients take the split
    kernel (info[0] == -1) in some runs and another plan in others: both kernels are behind the exact comparisons above
    (lav_conv_tile_info is the plan lav_conv2d takes; the step test holds every engine's plan to the one computed here)."""
    plans = {}
    for split in SPLITS:
        set_knobs(monkeypatch, precision, split)
        plans.update({(g.name, split): dgrad_plan(g, cached(E.TrainConvCase, g)[0], precision)[0] for g in E.TRAIN_CONV_GEOMS if g.dgrad == "lib"})
    assert any(v == -1 for v in plans.values()) and any(v != -1 for v in plans.values()), plans


@pytest.mark.parametrize("precision", [BF16X6, F16X3])
def test_split_kernel_with_one_step_per_chunk_is_exact(precision, monkeypatch):
    """A 1x1 layer pinned to the split kernel: one tap per 16-channel chunk, eight chunks.  With one step per chunk the kernel's
    loaders stage chunk 2 into chunk 0's buffer during the first group of steps, in which the compute waves still fetch tap 0; the
    kernel orders the two with a barrier of its own (conv_split_kernel.hpp, one_step_chunks).  Without it the one-tap parity class of
    the 3x3 stride-2 data gradients (cases b and c above, f16x3, pinned to the split kernel) returned chunk 2's products in chunk
    0's place at some staged positions - in some processes, not in others: a race, which an exact comparison catches only when it
    is lost.  This is the same path at its plainest, a few launches in a row."""
    set_knobs(monkeypatch, precision, "2")
    g = E.ONE_STEP_GEOM
    case, ref = cached(lambda *key: E.ConvLayerCase(g, "A"), "one step per chunk")
    layer = ops.ConvLayer(case.w, precision=PREC[precision], device=DEV, **case.layer_kwargs())
    assert plan_of(layer.desc, g.B, g.H, g.W)[0] == -1, "the layer must run on the split kernel"
    x = case.x.to(DEV)
    for n in range(4):
        assert_exact(layer(x), ref, f"{case.name} at {precision}, launch {n}")


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: f"split {s}")
@pytest.mark.parametrize("precision", [BF16X6, F16X3])
@pytest.mark.parametrize("geom", E.TRAIN_CONVT_GEOMS, ids=lambda g: "-".join(str(v) for v in g))
def test_training_transposed_convolution_step_is_exact(geom, precision, split, monkeypatch):
    """hipnn.conv_transpose_module with LAV_TRAIN_CONVT=hip: y (the transposed plan) and dx (the ordinary convolution with the same
    tensor) are exact, twice (the weight doubled in place between); dw is torch's."""
    B, cin, cout, k, s, p, op, H, W = geom
    set_knobs(monkeypatch, precision, split, (("LAV_TRAIN_CONVT", "hip"),))
    case, (y64, dx64) = cached(E.TrainConvTCase, *geom)
    m = torch.nn.ConvTranspose2d(cin, cout, k, s, p, op, bias=False).to(DEV)
    with torch.no_grad():
        m.weight.copy_(case.w)
    x = case.x.to(DEV).requires_grad_(True)
    dy = case.dy.to(DEV)
    xr, wr = case.x.double().requires_grad_(True), case.w.double().requires_grad_(True)
    dw64, = torch.autograd.grad(torch.nn.functional.conv_transpose2d(xr, wr, None, s, p, op), wr, case.dy.double())
    for scale in (1.0, 2.0):
        what = f"{case.name} at {precision}, LAV_CONV_SPLIT {split}, weight x {scale}"
        y = hipnn.conv_transpose_module(m, x)
        assert type(y.grad_fn).__name__.startswith(hipnn._ConvT2d.__name__), "the liblav_amd function must be the one that ran"
        gx, gw = torch.autograd.grad(y, (x, m.weight), dy)
        torch.cuda.synchronize()
        assert_exact(y, y64 * scale, what + ": y")
        assert_exact(gx, dx64 * scale, what + ": dx")
        within_the_torch_bar(gw, dw64, what + ": dw")
        assert {key[0] for key in hipnn._CONV_ENGINES} == {"fwdT", "dgradT"}
        with torch.no_grad():
            m.weight.mul_(2.0)
