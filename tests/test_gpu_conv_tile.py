"""lav_conv3x3_tile_f16 (ops.ConvTileRun): a 64-channel stage's same-shape conv3x3 -> ReLU -> BatchNorm layers as ONE launch on halo
tiles, against float64 and against the per-layer LAV_CONV_F16X3 path it replaces.

Bars.  The last layer is held to tests/test_gpu_conv_run.py's bound, 2e-6 * sum|a||b| * |scale| + 1.2e-7 * (|v scale| + |shift|), with
`mid` - the output of the tile run of the first L-1 layers - as its input.  One term more, derived: a workgroup recomputes the halo of
`mid` under its own activation scale, so the value it multiplies can differ from the owner tile's (the one `mid` holds) by at most
twice that same bound evaluated for the layer that produced `mid` (each of the two is within one bound of the float64 value of their
common input).  That difference enters the last layer multiplied by sum|w| and |scale|:
    bound += conv(2 * bound_of_the_layer_before, |w|) * |scale|.
End to end the run may be at most 2x as far from float64 as the per-layer path on the same inputs."""
import pytest
import torch
import torch.nn.functional as F

from lav_amd import _lib, ops, synth
from tests.test_gpu_conv_run import DEV, make_layers, per_layer, ref_layer
from tests.util import build_models

pytestmark = pytest.mark.gpu
C = 64
GEOMETRIES = [(8, 16, 3), (9, 17, 3), (5, 7, 3), (37, 53, 2), (37, 53, 3), (16, 32, 1), (160, 160, 3)]


def layer_bound(inp, p):
    """(float64 output, bound, sum|a||b| |scale|) of one layer on the float64 input `inp`: the bound of test_gpu_conv_run.py."""
    w, scale, shift = p
    sc, sh = scale[None, :, None, None], shift[None, :, None, None]
    v = F.relu(F.conv2d(inp, w, None, 1, 1))
    mag = F.conv2d(inp.abs(), w.abs(), None, 1, 1) * sc.abs()
    return v * sc + sh, 2e-6 * mag + 1.2e-7 * (v * sc.abs() + sh.abs()), mag


def last_layer_error_over_bound(y, layers, params, x):
    """max |y - float64(last layer on the tile run's own mid)| / bound (module docstring).  y: float64 on the host, x: on the device."""
    L = len(layers)
    mid = ops.ConvTileRun(layers[:-1])(x).double().cpu() if L > 1 else x.double().cpu()
    want, bound, _ = layer_bound(mid, params[-1])
    if L > 1:
        before = ops.ConvTileRun(layers[:-2])(x).double().cpu() if L > 2 else x.double().cpu()
        _, bound_before, _ = layer_bound(before, params[-2])
        w, scale, _ = params[-1]
        bound = bound + F.conv2d(2 * bound_before, w.abs(), None, 1, 1) * scale.abs()[None, :, None, None]
    return ((y - want).abs() / bound.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("H,W,L", GEOMETRIES)
def test_tile_run_is_as_accurate_as_the_layers_it_replaces(H, W, L):
    layers, params = make_layers(C, L, seed=C + H + L)
    torch.manual_seed(11)
    x = torch.randn((1, C, H, W))
    run = ops.ConvTileRun(layers)
    assert run.takes(1, H, W)
    y = run(x.to(DEV))
    y2 = run(x.to(DEV))
    assert torch.equal(y, y2), "two launches on the same input differ"
    ratio = last_layer_error_over_bound(y.double().cpu(), layers, params, x.to(DEV))
    print(f"{H}x{W} L {L}: last layer error / bound max {ratio:.3f}")
    assert ratio <= 1.0, f"last layer beyond its bound: worst error / bound {ratio:.3f}"
    want = x.double()
    for p in params:
        want = ref_layer(want, p)
    e_run = (y.double().cpu() - want).abs().max().item()
    e_lay = (per_layer(layers, x.to(DEV)).double().cpu() - want).abs().max().item()
    print(f"{H}x{W} L {L}: end to end max |error| tile run {e_run:.3e}, per layer {e_lay:.3e}, ratio {e_run / e_lay:.3f}")
    assert e_run <= 2 * e_lay, (e_run, e_lay)


@pytest.mark.parametrize("H,W,L", [(37, 53, 2), (9, 17, 3)])
@pytest.mark.parametrize("kind", ["six_decades_rows", "six_decades_columns", "zero", "tiny", "one_pixel"])
def test_tile_run_on_inputs_at_the_edges_of_the_scale(kind, H, W, L):
    """Magnitudes spanning six decades along rows / along columns (tiles of very different scale next to each other), an all-zero
    map, a map at 1e-20, a map that is zero except for one pixel at a tile corner."""
    layers, params = make_layers(C, L, seed=5)
    torch.manual_seed(12)
    x = torch.randn((1, C, H, W))
    if kind == "six_decades_rows":
        x = x * (10.0 ** torch.linspace(-3, 3, H))[None, None, :, None]
    elif kind == "six_decades_columns":
        x = x * (10.0 ** torch.linspace(-3, 3, W))[None, None, None, :]
    elif kind == "zero":
        x = torch.zeros_like(x)
    elif kind == "tiny":
        x = x * 1e-20
    else:
        one = torch.zeros_like(x)
        one[:, :, 8, 16] = x[:, :, 8, 16]      # the first pixel of the tile right of and below the first one (8 x 16 and 16 x 8 tiles alike)
        x = one
    y = ops.ConvTileRun(layers)(x.to(DEV)).double().cpu()
    assert torch.isfinite(y).all()
    ratio = last_layer_error_over_bound(y, layers, params, x.to(DEV))
    print(kind, f"{H}x{W} L {L}: last layer error / bound max {ratio:.3f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("H,W,L", [(37, 53, 2), (9, 17, 3)])
def test_tile_run_leaves_its_workgroups_maxima_for_the_next_layer(H, W, L):
    layers, _ = make_layers(C, L, seed=7)
    nxt_layer = make_layers(C, 1, seed=8)[0][0]
    torch.manual_seed(13)
    x = torch.randn((1, C, H, W), device=DEV)
    am = ops.Amax(DEV)
    y = ops.ConvTileRun(layers)(x, amax_out=am)
    n = _lib.load().lav_conv3x3_tile_f16_amax_count(C, H, W, L)
    assert n > 0 and am.count == n
    assert am.buf[:n].max().item() == y.abs().max().item()
    assert torch.equal(nxt_layer(y, amax_in=am), nxt_layer(y))


def test_tile_run_serves_64_channels_and_three_layers_only():
    lib = _lib.load()
    assert lib.lav_conv3x3_tile_f16_lds_bytes(64, 160, 160, 3) > 0 and lib.lav_conv3x3_tile_f16_lds_bytes(64, 1, 1, 1) > 0
    assert lib.lav_conv3x3_tile_f16_lds_bytes(64, 160, 160, 3) <= 160 * 1024
    assert lib.lav_conv3x3_tile_f16_lds_bytes(128, 80, 80, 3) == 0 and lib.lav_conv3x3_tile_f16_lds_bytes(64, 160, 160, 4) == 0
    assert lib.lav_conv3x3_tile_f16_amax_count(128, 80, 80, 3) == 0
    assert not ops.ConvTileRun(make_layers(C, 4, seed=3)[0]).takes(1, 160, 160)


def test_backbone_with_the_tile_run_matches_the_per_layer_backbone(monkeypatch):
    """ConvBackbone on the bev.npz input (synth.stacked_lidar(8192)): LAV_BEV_TILE=1 and =0 within 3e-5 of each other - the tolerance
    test_backbone_heads_vs_reference_golden holds the features to against the reference.  With LAV_BEV_RUN=1, s1 stays a ConvRun."""
    pts = synth.stacked_lidar(8192)
    monkeypatch.delenv("LAV_BEV_RUN", raising=False)
    feats = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("LAV_BEV_TILE", mode)
        lm, _ = build_models(DEV)
        with torch.no_grad(), ops.precision(_lib.CONV_F16X3):
            canvas = lm.point_pillar_net([torch.from_numpy(pts).to(DEV)], [len(pts)])
            feats[mode] = lm.backbone(canvas).clone()
            s1 = lm.backbone._engine(canvas.device)["runs"][0]
            assert isinstance(s1, ops.ConvTileRun) if mode == "1" else s1 is None
    d = (feats["1"] - feats["0"]).abs().max().item()
    print(f"LAV_BEV_TILE=1: max |features - per-layer features| {d:.3e} (|features| max {feats['0'].abs().max().item():.3e})")
    assert d <= 3e-5, d
    monkeypatch.setenv("LAV_BEV_RUN", "1")
    lm, _ = build_models(DEV)
    with torch.no_grad(), ops.precision(_lib.CONV_F16X3):
        canvas = lm.point_pillar_net([torch.from_numpy(pts).to(DEV)], [len(pts)])
        lm.backbone(canvas)
        runs = lm.backbone._engine(canvas.device)["runs"]
    assert all(type(r) is ops.ConvRun for r in runs)
