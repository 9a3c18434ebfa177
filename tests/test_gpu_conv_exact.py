"""The convolution kernels bit for bit: on the exactly representable data of tests/exact_util.py (classes A, B, D, C, R - checked on the
host by tests/test_conv_exact_host.py) the float64 result is the only correct answer at every precision, dispatch, tiling, split-K plan
and hand-off, so every comparison here is torch.equal(kernel output in float64, float64 reference).  No tolerance anywhere.

What a failing class points at: A indexing (taps, halos, borders, strides, channel windows, split-K); B and D the activation-side pieces;
C the weight-side pieces or the packers; R halos, hand-offs or per-workgroup scales of the kernels that keep intermediate maps."""
import ctypes

import pytest
import torch
from torch import nn

from lav_amd import _lib, ops
from tests import exact_util as E
from tests.exact_util import BF16X6, F16X3, F32, PRECISIONS, assert_exact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PREC = {F32: _lib.CONV_F32, BF16X6: _lib.CONV_BF16X6, F16X3: _lib.CONV_F16X3}
GEOMS = E.conv_geometries() + E.conv_geometries(own_batch=True)
STEMS = [g for g in GEOMS if (g.kh, g.stride) == (7, 2) and not g.transposed and g.cin >= 32 and g.H <= 50]      # (the stems: not the 7x7 data-gradient plans)
_cases: dict = {}


def cached_case(g, key, epilogue="none", batch=None):
    """(case, float64 reference), computed once per geometry and shared by the three precisions' tests."""
    if _cases and next(iter(_cases))[0] != tuple(g):
        _cases.clear()
    k = (tuple(g), key, epilogue, batch)
    if k not in _cases:
        case = E.ConvLayerCase(g, key, epilogue, batch)
        _cases[k] = (case, case.forward(E.Plain()))
    return _cases[k]


def assert_folded(layer, scale, shift, what):
    """The host side of class R's promise: the folded BatchNorm IS the power-of-two scale and the integer shift the reference uses."""
    assert torch.equal(layer.scale.double().cpu(), scale) and torch.equal(layer.shift.double().cpu(), shift), f"{what}: folded scale / shift"


def pin_plan(monkeypatch, g, precision):
    if g.force and precision in g.force_precisions:
        monkeypatch.setenv("LAV_CONV_SPLIT", "2")
        monkeypatch.setenv("LAV_SPLIT_FORCE", g.force)
    else:
        monkeypatch.delenv("LAV_CONV_SPLIT", raising=False)
        monkeypatch.delenv("LAV_SPLIT_FORCE", raising=False)


def handed_in(x, factor):
    """An Amax as a producer leaves it: parts whose maximum is factor * max |x|."""
    am = ops.Amax(DEV)
    parts = am.take(7)
    parts.zero_()
    parts[3] = float(x.abs().max()) * factor
    parts[5] = 2.0 ** -30
    return am


def run_conv_layer(case, ref, precision, limit=None):
    g = case.g
    layer = ops.ConvLayer(case.w, precision=PREC[precision], device=DEV, **case.layer_kwargs())
    if case.bn is not None:
        assert_folded(layer, case._scale, case._shift, case.name)
    x = case.x.to(DEV)
    B = x.shape[0]
    oh, ow = case.out_hw()
    windows = case.out_total != g.cout
    res = None
    if case.residual is not None:
        res = case.residual.to(DEV)
    info = (ctypes.c_int * 9)()
    d = _lib.Conv.from_buffer_copy(layer.desc)
    d.batch, d.h, d.w = B, g.H, g.W
    assert _lib.load().lav_conv_tile_info(ctypes.byref(d), info) == 0
    what = f"{case.name} at {precision} (plan {list(info)})"

    def launch(**kw):
        out = torch.full((B, case.out_total, oh, ow), 7.0, device=DEV)
        layer(x, out=out, residual=res, **kw)
        if windows:
            assert bool((out[:, :case.out_off] == 7).all()) and bool((out[:, case.out_off + g.cout:] == 7).all()), f"{what}: channels outside the window were touched"
        return out[:, case.out_off:case.out_off + g.cout]

    if limit is not None:
        with ops.batch_limit(torch.tensor([limit], dtype=torch.int32, device=DEV)):
            y = launch()
        torch.cuda.synchronize()
        assert_exact(y[:limit], ref[:limit], what + f", rows below the batch limit {limit}")
        assert bool((y[limit:] == 7).all()), f"{what}: rows at or beyond the batch limit were written"
        return
    assert_exact(launch(), ref, what)
    if precision == F16X3 and case.epilogue == "none" and layer.uses_amax(B, g.H, g.W):
        assert_exact(launch(amax_in=handed_in(x, 1.0)), ref, what + ", handed-in maxima")
        assert_exact(launch(amax_in=handed_in(x, 4.0)), ref, what + ", a handed-in bound 4x above the maximum")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("g", GEOMS, ids=[g.name for g in GEOMS])
def test_conv_layer_is_exact(g, precision, monkeypatch):
    """ops.ConvLayer: classes A, D, C, E (f32, bf16x6) or A, B, C (f16x3: measuring its input, on handed-in maxima, on a bound 4x above them),
    and on class A an integer bias, ReLU before / after a power-of-two affine, a residual and channel windows on both sides."""
    pin_plan(monkeypatch, g, precision)
    for cls, key in E.conv_classes(precision).items():
        case, ref = cached_case(g, key)
        run_conv_layer(case, ref, precision)
    for ep in E.EPILOGUES[1:]:
        case, ref = cached_case(g, "A", ep)
        run_conv_layer(case, ref, precision)


def test_class_d_belongs_to_f32_and_bf16x6_only():
    """The other side of the classes: 23-bit activations do not fit two fp16 pieces (22 bits), so the f16x3 plan must MISS float64 on
    class D - by no more than the bits it drops - where f32 and bf16x6 return it.  Shows that the precision asked for is the one that ran."""
    g = next(g for g in GEOMS if g.name == "f16: BEV 64->64 s1 160x160")
    case, ref = cached_case(g, "D")
    layer = ops.ConvLayer(case.w, precision=_lib.CONV_F16X3, device=DEV, **case.layer_kwargs())
    assert layer.uses_amax(g.B, g.H, g.W)
    y = layer(case.x.to(DEV)).double().cpu()
    assert not torch.equal(y, ref)
    # each output is ONE product x 2^k: what is lost is x / s beyond its second piece - 2^-22 of it, or fp16's subnormal quantum 2^-24
    # with s <= 2^-14 max |x|
    slack = 2.0 ** -38 * float(case.x.abs().max()) * float(case.w.abs().max())
    assert bool(((y - ref).abs() <= 2.0 ** -21 * ref.abs() + slack).all())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("g", STEMS, ids=[g.name for g in STEMS])
def test_stem_past_its_batch_limit_is_exact(g, precision, monkeypatch):
    """The 7x7 stride-2 stem at capacity 5 with a device-resident limit of 2 rows: the live rows are the float64 result, the others untouched."""
    pin_plan(monkeypatch, g, precision)
    case, ref = cached_case(g, "A", batch=5)
    run_conv_layer(case, ref, precision, limit=2)


def run_layers(case):
    layers = []
    for w, bn, scale, shift in case.layers:
        layers.append(ops.ConvLayer(w, padding=1, bn=bn, bn_eps=0.0, relu_pre=True, precision=_lib.CONV_F16X3, device=DEV))
        assert_folded(layers[-1], scale, shift, case.name)
    return layers


@pytest.mark.parametrize("kind", E.R_KINDS)
@pytest.mark.parametrize("Cn,H,W,L", E.RUN_GEOMS)
def test_conv_run_is_exact(Cn, H, W, L, kind):
    case = E.RunCase(Cn, H, W, L, kind)
    run = ops.ConvRun(run_layers(case))
    assert run.takes(1, H, W)
    gave_up = ops.bev_run_status(DEV)[0]
    y = run(case.x.to(DEV))
    assert ops.bev_run_status(DEV)[0] == gave_up
    assert_exact(y, case.forward(E.Plain()), case.name)


@pytest.mark.parametrize("kind", E.R_KINDS)
@pytest.mark.parametrize("H,W,L", E.TILE_GEOMS)
def test_conv_tile_run_is_exact(H, W, L, kind):
    case = E.RunCase(64, H, W, L, kind)
    run = ops.ConvTileRun(run_layers(case))
    assert run.takes(1, H, W)
    assert_exact(run(case.x.to(DEV)), case.forward(E.Plain()), case.name)


def make_pairs(case):
    pairs = []
    for (wa, ba, wb, bb, (mean, var, gamma, beta), scale, shift), (da, db) in zip(case.pairs, case.dils):
        ca = nn.Conv2d(case.C, case.C, (3, 1), padding=(da, 0), dilation=(da, 1))
        cb = nn.Conv2d(case.C, case.C, (1, 3), padding=(0, db), dilation=(1, db))
        bn = nn.BatchNorm2d(case.C, eps=0.0).eval()
        with torch.no_grad():
            ca.weight.copy_(wa); ca.bias.copy_(ba); cb.weight.copy_(wb); cb.bias.copy_(bb)
            bn.running_mean.copy_(mean); bn.running_var.copy_(var); bn.weight.copy_(gamma); bn.bias.copy_(beta)
        pairs.append(ops.Conv1dPair(ca, cb, bn, device=DEV))
        assert_folded(pairs[-1], scale, shift, case.name)
    return pairs


def run_chain(case, precision):
    pairs = make_pairs(case)
    with ops.precision(PREC[precision]):
        chain = ops.Conv1dPairChain(pairs, case.residual)
    assert chain.f16 == (precision == F16X3)
    x = case.x.to(DEV)
    assert chain.supported(x)
    gave_up = ops.pair_chain_status(DEV)[0]
    y = chain(x)
    assert ops.pair_chain_status(DEV)[0] == gave_up, "a workgroup of the persistent run gave up"
    assert_exact(y, case.forward(E.Plain()), f"{case.name}, chain at {precision}")


@pytest.mark.parametrize("kind", E.R_KINDS)
@pytest.mark.parametrize("Cn,H,W,d", E.PAIR_GEOMS)
def test_conv1d_pair_is_exact(Cn, H, W, d, kind):
    """ops.Conv1dPair (one launch, bf16x6) with and without the residual; on fp16 pieces (the persistent kernel is the only one that has
    them) the same pair as a chain of one, and the residual as the non_bottleneck_1d block it belongs to.  Dilation 16 on 36 rows reaches past the map."""
    for with_res in (False, True):
        case = E.pair_case(Cn, H, W, d, with_res, kind)
        pair, = make_pairs(case)
        x = case.x.to(DEV)
        assert pair.supported(x)
        assert_exact(pair(x, residual=x if with_res else None), case.forward(E.Plain()), case.name)
    run_chain(E.pair_case(Cn, H, W, d, False, kind), F16X3)
    for precision in (BF16X6, F16X3):
        run_chain(E.block_case(Cn, H, W, d, kind), precision)


@pytest.mark.parametrize("precision", [BF16X6, F16X3])
@pytest.mark.parametrize("kind", E.R_KINDS)
@pytest.mark.parametrize("Cn,H,W,dils", E.CHAIN_GEOMS)
def test_conv1d_pair_chain_is_exact(Cn, H, W, dils, kind, precision):
    run_chain(E.chain_case(Cn, H, W, dils, kind), precision)


@pytest.mark.parametrize("key", E.FP32_CLASSES)
@pytest.mark.parametrize("outs,cin_g,H,W,B", E.DECONV_GEOMS)
def test_grouped_deconv_is_exact(outs, cin_g, H, W, B, key, monkeypatch):
    """ops.GroupedDeconv with the identity epilogue, k_deconv_tile and the gathering kernel."""
    case = E.DeconvCase(outs, cin_g, H, W, B, key)
    cts = []
    for o, w, b in zip(outs, case.ws, case.biases):
        ct = nn.ConvTranspose2d(cin_g, o, 3, stride=2, padding=1, output_padding=1)
        with torch.no_grad():
            ct.weight.copy_(w); ct.bias.copy_(b)
        cts.append(ct)
    layer = ops.GroupedDeconv(cts, sigmoid_from=-1, device=DEV)
    ref = case.forward(E.Plain())
    x = case.x.to(DEV)
    monkeypatch.delenv("LAV_DECONV_IMPL", raising=False)
    assert_exact(layer(x), ref, case.name + ", staged kernel")
    monkeypatch.setenv("LAV_DECONV_IMPL", "gather")
    assert_exact(layer(x), ref, case.name + ", gathering kernel")


@pytest.mark.parametrize("key", E.FP32_CLASSES)
@pytest.mark.parametrize("cin,cout,k,pad,opad,H,W", E.UPCONV_GEOMS)
def test_pointwise_upconv_is_exact(cin, cout, k, pad, opad, H, W, key):
    """ops.PointwiseUpconv ("exact fp32 matrix products"): held to that, into a channel slice of a wider map."""
    case = E.UpconvCase(cin, cout, k, pad, opad, H, W, key)
    ct = nn.ConvTranspose2d(cin, cout, k, k, pad, opad, bias=False)
    bn = nn.BatchNorm2d(cout, eps=0.0).eval()
    with torch.no_grad():
        ct.weight.copy_(case.w)
        for t, v in zip((bn.running_mean, bn.running_var, bn.weight, bn.bias), case.bn):
            t.copy_(v)
    ct, bn = ct.to(DEV), bn.to(DEV)
    assert ops.PointwiseUpconv.takes(ct)
    total, off = cout + 48, 16
    layer = ops.PointwiseUpconv(ct, bn, relu_pre=True, out_c_total=total, out_c_offset=off, device=DEV)
    assert_folded(layer, case.scale, case.shift, case.name)
    x = case.x.to(DEV)
    oh, ow = layer.out_hw(H, W)
    out = torch.full((x.shape[0], total, oh, ow), -7.0, device=DEV)
    layer(x, out=out)
    assert_exact(out[:, off:off + cout], case.forward(E.Plain()), case.name)
    assert bool((out[:, :off] == -7).all()) and bool((out[:, off + cout:] == -7).all()), "wrote outside its channel slice"


@pytest.mark.parametrize("geom", E.WGRAD_GEOMS, ids=lambda g: "-".join(str(v) for v in g))
def test_conv_wgrad_is_exact(geom):
    """lav_conv_wgrad (bf16x6: classes A and D) and lav_conv_wgrad_amax (two fp16 pieces per operand, scales from measured maxima: A and B),
    3x3 at strides 1 and 2 and the 7x7 stride-2 stem (one ky per task)."""
    from lav_amd.ops import _ptr, _stream, _workspace, check
    lib = _lib.load()
    (B, cin, cout, H, W, S), k = geom[:6], (geom[6] if len(geom) > 6 else 3)
    nbytes = lib.lav_conv_wgrad_workspace_bytes(B, cin, cout, H, W, k, S)
    assert nbytes > 0
    ws = _workspace("conv_wgrad_exact", nbytes, DEV)
    for key, f16 in (("A", False), ("D", False), ("A", True), ("B", True)):
        case = E.WgradCase(B, cin, cout, H, W, S, key, k)
        x, dy = case.x.to(DEV), case.dy.to(DEV)
        dw = torch.full((cout, cin, k, k), float("nan"), device=DEV)
        if f16:
            ax, ay = torch.zeros(512, device=DEV), torch.zeros(512, device=DEV)
            check(lib.lav_absmax_parts(_ptr(x), x.numel(), _ptr(ax), _stream()), "lav_absmax_parts")
            check(lib.lav_absmax_parts(_ptr(dy), dy.numel(), _ptr(ay), _stream()), "lav_absmax_parts")
            check(lib.lav_conv_wgrad_amax(_ptr(x), _ptr(dy), B, cin, cout, H, W, k, S, _ptr(dw), _ptr(ws), ws.numel(), _ptr(ax), 512, _ptr(ay), 512,
                                          _stream()), "lav_conv_wgrad_amax")
        else:
            check(lib.lav_conv_wgrad(_ptr(x), _ptr(dy), B, cin, cout, H, W, k, S, _ptr(dw), _ptr(ws), ws.numel(), _stream()), "lav_conv_wgrad")
        assert_exact(dw, case.forward(E.Plain()), case.name + (" on fp16 pieces" if f16 else " on bf16 pieces"))


@pytest.fixture(scope="module")
def backbone():
    import lav_amd
    from tests.util import CFG
    lm = lav_amd.LiDARModel(num_input=16, backbone="cnn", num_features=[64, 64], **CFG)
    params = E.fill_backbone(lm.backbone)
    return lm.eval().to(DEV).backbone, params


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_backbone_engine_is_exact(backbone, precision, B, monkeypatch):
    """LiDARModel.backbone end to end (16 convolutions, three up-convolutions into one feature map) with one-tap weights +-1, integer
    shifts and bn.eps = 0.  At batch 1 the f16x3 engine must have taken ConvTileRun for s1, ConvRun for s2 / s3 and PointwiseUpconv for
    upconv1 / upconv3 - on the smallest canvas of the list whose stage maps the runs take; the other engines are ConvLayers throughout."""
    for knob in ("LAV_BEV_RUN", "LAV_BEV_TILE", "LAV_UPCONV_POINTWISE", "LAV_CONV_SPLIT", "LAV_SPLIT_FORCE"):
        monkeypatch.delenv(knob, raising=False)
    bb, params = backbone
    device = next(bb.parameters()).device
    H, W = E.BACKBONE_CANVASES[0]
    with torch.no_grad(), ops.precision(PREC[precision]):
        e = bb._engine(device)
        runs, ups = e["runs"], [type(u).__name__ for u in e["ups"]]
        if precision == F16X3:
            assert [type(r).__name__ for r in runs] == ["ConvTileRun", "ConvRun", "ConvRun"] and ups == ["PointwiseUpconv", "ConvLayer", "PointwiseUpconv"], (runs, ups)
            if B == 1:
                fits = [(h, w) for h, w in E.BACKBONE_CANVASES if all(r.takes(1, h >> (i + 1), w >> (i + 1)) for i, r in enumerate(runs))]
                assert fits, "no canvas of the list on which every run takes its stage"
                H, W = fits[0]
            else:
                assert not any(r.takes(B, H >> (i + 1), W >> (i + 1)) for i, r in enumerate(runs))
        else:
            assert all(r is None for r in runs) and ups == ["ConvLayer"] * 3, (runs, ups)
        for st, name in (("s1", "conv1"), ("s2", "conv2"), ("s3", "conv3")):
            for layer, (_, shift, *_) in zip(e[st], params[name]):
                assert_folded(layer, torch.ones_like(shift), shift, f"backbone {name}")
        case = E.BackboneCase(params, B, H, W)
        gave_up = ops.bev_run_status(device)[0]
        y = bb(case.x.to(device))
        assert ops.bev_run_status(device)[0] == gave_up
    assert_exact(y, case.forward(E.Plain()), f"{case.name} at {precision}")
