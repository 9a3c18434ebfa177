"""lav_conv3x3_run_f16 (ops.ConvRun): a stage's same-shape conv3x3 -> ReLU -> BatchNorm layers as ONE persistent launch, against
float64 and against the per-layer LAV_CONV_F16X3 path it replaces.

Bars.  The dot product's is the project's bar for the split kernels, 2e-6 * sum|a||b| per output value (tests/test_gpu_glue.py).  Behind
it sit a ReLU (1-Lipschitz) and v * scale + shift in fp32: the dot product's error is multiplied by |scale|; scale and shift are
themselves rounded to fp32 and the fma rounds once (2^-24 each, relative to |v scale|, |shift| and |y| <= |v scale| + |shift|; 1.2e-7
allows two roundings of each term): bound = 2e-6 * sum|a||b| * |scale| + 1.2e-7 * (|v scale| + |shift|), applied to the LAST layer of
a run with the run's own intermediate map (the output of the run of the first L-1 layers: a layer's result does not depend on what follows
it) as that layer's input.  End to end the run may be at most 2x as far from float64 as the per-layer path on the same inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lav_amd import _lib, ops, synth
from tests.util import build_models

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GEOMETRIES = [(64, 160, 160, 3), (128, 80, 80, 5), (128, 40, 40, 5), (64, 37, 53, 2)]


def make_layers(C, L, seed):
    """L seeded layers: (ConvLayers packed for LAV_CONV_F16X3, [(weight, scale, shift) in float64])."""
    g = torch.Generator().manual_seed(seed)
    layers, params = [], []
    for _ in range(L):
        w = torch.randn((C, C, 3, 3), generator=g) * (2.0 / (9 * C)) ** 0.5
        mean, var = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
        gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
        layers.append(ops.ConvLayer(w, padding=1, bn=(mean, var, gamma, beta), bn_eps=1e-3, relu_pre=True, precision=_lib.CONV_F16X3, device=DEV))
        scale = gamma.double() / torch.sqrt(var.double() + 1e-3)
        params.append((w.double(), scale, beta.double() - mean.double() * scale))
    return layers, params


def ref_layer(x64, p):
    w, scale, shift = p
    return F.relu(F.conv2d(x64, w, None, 1, 1)) * scale[None, :, None, None] + shift[None, :, None, None]


def last_layer_error_over_bound(y, mid, p):
    """max over the outputs of |y - float64(last layer on mid)| / bound (module docstring), and of |error| / (sum|a||b| |scale|)."""
    w, scale, shift = p
    sc, sh = scale[None, :, None, None], shift[None, :, None, None]
    v = F.relu(F.conv2d(mid, w, None, 1, 1))
    mag = F.conv2d(mid.abs(), w.abs(), None, 1, 1) * sc.abs()
    err = (y - (v * sc + sh)).abs()
    bound = 2e-6 * mag + 1.2e-7 * (v * sc.abs() + sh.abs())
    return (err / bound.clamp_min(1e-300)).max().item(), (err / mag.clamp_min(1e-300)).max().item()


def per_layer(layers, x):
    am = None
    for l in layers:
        nxt = ops.Amax(DEV)
        x = l(x, amax_in=am, amax_out=nxt)
        am = nxt
    return x


@pytest.mark.parametrize("C,H,W,L", GEOMETRIES)
def test_run_is_as_accurate_as_the_layers_it_replaces(C, H, W, L):
    layers, params = make_layers(C, L, seed=C + H + L)
    torch.manual_seed(11)
    x = torch.randn((1, C, H, W))
    run = ops.ConvRun(layers)
    assert run.takes(1, H, W)
    y = run(x.to(DEV))
    y2 = run(x.to(DEV))
    assert torch.equal(y, y2), "two launches on the same input differ"
    # the last layer alone, on the run's own intermediate map
    mid = ops.ConvRun(layers[:-1])(x.to(DEV)).double().cpu() if L > 1 else x.double()
    ratio, rel = last_layer_error_over_bound(y.double().cpu(), mid, params[-1])
    print(f"C {C} {H}x{W} L {L}: last layer error / bound max {ratio:.3f}, error / (sum|a||b| |scale|) max {rel:.3e}")
    assert ratio <= 1.0, f"last layer beyond 2e-6 sum|a||b|: worst error / bound {ratio:.3f}"
    # end to end against float64, next to the per-layer path
    want = x.double()
    for p in params:
        want = ref_layer(want, p)
    e_run = (y.double().cpu() - want).abs().max().item()
    e_lay = (per_layer(layers, x.to(DEV)).double().cpu() - want).abs().max().item()
    print(f"C {C} {H}x{W} L {L}: end to end max |error| run {e_run:.3e}, per layer {e_lay:.3e}, ratio {e_run / e_lay:.3f}")
    assert e_run <= 2 * e_lay, (e_run, e_lay)


@pytest.mark.parametrize("kind", ["six_decades", "zero", "tiny"])
def test_run_on_inputs_at_the_edges_of_the_scale(kind):
    """Rows spanning six decades (a per-tensor scale would flush the small rows' low pieces: here every workgroup scales by what it
    reads), an all-zero map, a map at 1e-20."""
    C, H, W, L = 64, 37, 53, 2
    layers, params = make_layers(C, L, seed=5)
    torch.manual_seed(12)
    x = torch.randn((1, C, H, W))
    if kind == "six_decades":
        x = x * (10.0 ** torch.linspace(-3, 3, H))[None, None, :, None]
    elif kind == "zero":
        x = torch.zeros_like(x)
    else:
        x = x * 1e-20
    y = ops.ConvRun(layers)(x.to(DEV)).double().cpu()
    assert torch.isfinite(y).all()
    mid = ops.ConvRun(layers[:-1])(x.to(DEV)).double().cpu()
    ratio, _ = last_layer_error_over_bound(y, mid, params[-1])
    print(kind, "last layer error / bound max", ratio)
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("C,H,W,L", [(128, 40, 40, 5), (64, 37, 53, 2)])
def test_run_leaves_its_workgroups_maxima_for_the_next_layer(C, H, W, L):
    layers, _ = make_layers(C, L, seed=7)
    nxt_layer = make_layers(C, 1, seed=8)[0][0]
    torch.manual_seed(13)
    x = torch.randn((1, C, H, W), device=DEV)
    am = ops.Amax(DEV)
    y = ops.ConvRun(layers)(x, amax_out=am)
    n = _lib.load().lav_conv3x3_run_f16_amax_count(C, H, W)
    assert am.count == n and n % H == 0
    ns = n // H
    want = y[0].abs().reshape(ns, C // ns, H, W).amax((1, 3)).t().reshape(-1)      # workgroup = row * slices + slice
    assert torch.equal(am.buf[:n], want)
    assert torch.equal(nxt_layer(y, amax_in=am), nxt_layer(y))


def test_run_timeout_is_counted_and_never_hangs(monkeypatch):
    """With the spin limit at 0 every wait that is not satisfied at once gives up: the launch returns, the sticky counter is raised,
    the rows of the workgroups that gave up are NaN; the next launch with the default limit is clean.  (A bounded exit, not a hang.)"""
    C, H, W, L = 128, 40, 40, 5
    layers, _ = make_layers(C, L, seed=9)
    torch.manual_seed(14)
    x = torch.randn((1, C, H, W), device=DEV)
    run = ops.ConvRun(layers)
    good = run(x)
    t0, l0 = ops.bev_run_status(DEV)
    monkeypatch.setenv("LAV_CHAIN_SPIN_LIMIT", "0")
    bad = run(x)
    torch.cuda.synchronize()
    monkeypatch.delenv("LAV_CHAIN_SPIN_LIMIT")
    t1, l1 = ops.bev_run_status(DEV)
    assert l1 == l0 + 1 and t1 > t0
    rows_nan = torch.isnan(bad[0]).all(2)            # [channel][row]
    assert rows_nan.any()
    ok = ~torch.isnan(bad)
    assert torch.equal(bad[ok], good[ok]), "a row that is not NaN must be the complete result"
    again = run(x)
    t2, l2 = ops.bev_run_status(DEV)
    assert (t2, l2) == (t1, l1 + 1) and torch.equal(again, good)


def test_backbone_with_runs_matches_the_per_layer_backbone(monkeypatch):
    """ConvBackbone on the bev.npz input (synth.stacked_lidar(8192)): LAV_BEV_RUN=0, the default and every stage as a run within 3e-5
    of each other - the tolerance test_backbone_heads_vs_reference_golden holds the features to against the reference."""
    pts = synth.stacked_lidar(8192)
    gave_up = ops.bev_run_status(DEV)[0]        # (sticky per workspace: what earlier tests of this process left)
    feats = {}
    for mode in ("0", None, "1"):
        if mode is None:
            monkeypatch.delenv("LAV_BEV_RUN", raising=False)
        else:
            monkeypatch.setenv("LAV_BEV_RUN", mode)
        lm, _ = build_models(DEV)
        with torch.no_grad(), ops.precision(_lib.CONV_F16X3):
            canvas = lm.point_pillar_net([torch.from_numpy(pts).to(DEV)], [len(pts)])
            feats[mode] = lm.backbone(canvas).clone()
            if mode == "1":
                assert all(r is not None for r in lm.backbone._engine(canvas.device)["runs"])
    for mode in (None, "1"):
        d = (feats[mode] - feats["0"]).abs().max().item()
        print(f"LAV_BEV_RUN={mode}: max |features - per-layer features| {d:.3e} (|features| max {feats['0'].abs().max().item():.3e})")
        assert d <= 3e-5, (mode, d)
    assert ops.bev_run_status(DEV)[0] == gave_up
