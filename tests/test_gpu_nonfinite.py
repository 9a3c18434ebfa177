"""NaN and Inf through every ReLU and 2x2 max-pool of the library: include/lav_amd.h promises that a non-finite activation makes the
outputs it reaches non-finite and changes no other bit, epilogue included.  Every kernel family runs three times - clean, with NaN in one
interior and one corner element, with +Inf / -Inf in the same two - and tests/nonfinite_util.py's rule decides from those outputs and the
float64 torch reference of the same operation: NaN wherever the reference has NaN, the clean run's bits everywhere else.  The cases,
their references and the proof that the rule rejects a NaN-dropping ReLU or pooling are tests/test_nonfinite_host.py's.

Geometries are the exact suite's (tests/exact_util.py): the smallest that reach each launch path."""
import copy
import ctypes

import pytest
import torch
from torch import nn

from lav_amd import _lib, ops
from lav_amd.train import hipnn
from tests import exact_util as E
from tests import nonfinite_util as N
from tests.exact_util import BF16X6, F16X3, F32, PRECISIONS
from tests.test_gpu_conv_exact import PREC, assert_folded, make_pairs, pin_plan, run_layers

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GEOMS = E.conv_geometries()
RUNS = ("clean",) + N.PLANTS


def three_runs(case, launch):
    """{"clean" | "nan" | "inf": launch(input on the device) as a tuple of host tensors}"""
    got = {}
    for p in RUNS:
        out = launch(case.input(p).to(DEV))
        torch.cuda.synchronize()
        got[p] = tuple(t.detach().cpu() for t in (out if isinstance(out, tuple) else (out,)))
    return got


def holds(case, launch, what=None):
    N.check_case(three_runs(case, launch), N.references(case), what or case.name)


# ---------------------------------------------------------------------------------------------- ops.ConvLayer
def plan_of(desc, B, H, W):
    info = (ctypes.c_int * 9)()
    d = _lib.Conv.from_buffer_copy(desc)
    d.batch, d.h, d.w = B, H, W
    assert _lib.load().lav_conv_tile_info(ctypes.byref(d), info) == 0
    return list(info)


def kernel_of(info):
    """Which kernel a plan names: lav_conv_tile_info's info[0] is -2 for k_conv_smallcin, -1 for the split-operand kernel (taps per slab
    + 100 in tap-pair mode, + 200 on fp16 pieces), 0 for the direct kernel, else the fp32 matrix kernel's tile; info[6] > 1 adds the
    split-K reduce."""
    name = {-2: "small cin", -1: "split f16" if info[7] >= 200 else "split bf16", 0: "direct"}.get(info[0], "fp32 tiles")
    return name + (" + reduce" if info[6] > 1 else "")


def assert_kernel(g, precision, info):
    kernel = kernel_of(info)
    what = f"{g.name} at {precision}: plan {info} ({kernel})"
    if g.cin == 3 and not g.transposed:
        assert kernel == "small cin", what
    if g.force and precision in g.force_precisions:
        assert kernel.startswith("split f16" if precision == F16X3 else "split bf16"), what
        if int(g.force.split(",")[5]) > 1:          # (0: the plan search's split-K)
            assert info[6] == int(g.force.split(",")[5]), what
    if g.name.startswith("direct: "):
        assert kernel.startswith("direct"), what
    if precision == F32:
        assert not kernel.startswith("split"), what
    if precision == BF16X6:
        assert not kernel.startswith("split f16"), what


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("g", GEOMS, ids=[g.name for g in GEOMS])
def test_conv_layer(g, precision, monkeypatch):
    """ops.ConvLayer with no epilogue, a bias, ReLU -> affine into channel windows, and affine -> + residual -> ReLU: the plan is pinned as
    tests/test_gpu_conv_exact.py pins it, the kernel it names is the one expected, and the channels beside an output window keep their fill."""
    pin_plan(monkeypatch, g, precision)
    for ep in E.EPILOGUES:
        case = N.ConvCase(g, ep)
        c = case.inner
        layer = ops.ConvLayer(c.w, precision=PREC[precision], device=DEV, **c.layer_kwargs())
        if c.bn is not None:
            assert_folded(layer, c._scale, c._shift, case.name)
        info = plan_of(layer.desc, g.B, g.H, g.W)
        assert_kernel(g, precision, info)
        oh, ow = c.out_hw()
        res = None if c.residual is None else c.residual.to(DEV)

        def launch(x):
            out = torch.full((g.B, c.out_total, oh, ow), 7.0, device=DEV)
            layer(x, out=out, residual=res)
            beside = torch.cat([out[:, :c.out_off], out[:, c.out_off + g.cout:]], dim=1)
            assert bool((beside == 7).all()), f"{case.name}: channels outside the window were touched"
            return out[:, c.out_off:c.out_off + g.cout]
        holds(case, launch, f"{case.name} at {precision} ({kernel_of(info)}, plan {info})")


def test_conv_cases_reach_every_kernel(monkeypatch):
    """The plans of test_conv_layer's cases name every convolution kernel with an epilogue: small-cin, direct, fp32 tiles, the split
    kernel on bf16 and on fp16 pieces, and each of them (but small-cin, which is never split) in front of the split-K reduce."""
    seen = set()
    for g in GEOMS:
        for precision in PRECISIONS:
            pin_plan(monkeypatch, g, precision)
            d = _lib.Conv(g.B, g.cin, 0, g.cin, g.H, g.W, g.cout, g.kh, g.kw, g.stride, g.ph, g.pw, g.dh, g.dw, int(g.transposed), g.out_pad, g.cout,
                          0, 0, 0, 0, 0, 0.0, PREC[precision])
            info = plan_of(d, g.B, g.H, g.W)
            assert_kernel(g, precision, info)
            seen.add(kernel_of(info))
    want = {"small cin"} | {k + r for k in ("direct", "fp32 tiles", "split bf16", "split f16") for r in ("", " + reduce")}
    assert seen == want, sorted(want ^ seen)


# ---------------------------------------------------------------------------------------------- runs, pairs, chains
@pytest.mark.parametrize("Cn,H,W,L", E.RUN_GEOMS)
def test_conv_run(Cn, H, W, L):
    """ops.ConvRun (persistent, default spin limit): the plant in layer 0's input passes L ReLUs and L - 1 scale hand-offs; no workgroup
    gave up, so a NaN in the output comes from the data."""
    case = N.RunCase(Cn, H, W, L)
    run = ops.ConvRun(run_layers(case))
    assert run.takes(1, H, W)
    gave_up = ops.bev_run_status(DEV)[0]
    holds(case, run)
    assert ops.bev_run_status(DEV)[0] == gave_up, "a workgroup of the persistent run gave up"


@pytest.mark.parametrize("H,W,L", E.TILE_GEOMS)
def test_conv_tile_run(H, W, L):
    """ops.ConvTileRun: the plant in layer 0's input passes L ReLUs inside one launch, the scales taken per workgroup."""
    case = N.RunCase(64, H, W, L)
    run = ops.ConvTileRun(run_layers(case))
    assert run.takes(1, H, W)
    holds(case, run)


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("Cn,H,W,d", E.PAIR_GEOMS)
def test_conv1d_pair(Cn, H, W, d, with_res):
    """ops.Conv1dPair: the ReLU between its two convolutions and the one behind the residual."""
    case = N.pair_case(Cn, H, W, d, with_res)
    pair, = make_pairs(case)
    assert pair.supported(case.x.to(DEV))
    holds(case, lambda x: pair(x, residual=x if with_res else None))


@pytest.mark.parametrize("precision", [BF16X6, F16X3])
@pytest.mark.parametrize("Cn,H,W,dils", E.CHAIN_GEOMS)
def test_conv1d_pair_chain(Cn, H, W, dils, precision):
    """ops.Conv1dPairChain (persistent, default spin limit) on bf16 and on fp16 pieces - there the row maxima handed from pair to pair are
    the finite ones, which the bit equality outside the reach shows; no workgroup gave up."""
    case = N.chain_case(Cn, H, W, dils)
    pairs = make_pairs(case)
    with ops.precision(PREC[precision]):
        chain = ops.Conv1dPairChain(pairs, case.residual)
    assert chain.f16 == (precision == F16X3)
    assert chain.supported(case.x.to(DEV))
    gave_up = ops.pair_chain_status(DEV)[0]
    holds(case, chain, f"{case.name}, chain at {precision}")
    assert ops.pair_chain_status(DEV)[0] == gave_up, "a workgroup of the persistent run gave up"


# ---------------------------------------------------------------------------------------------- up-convolution, grouped deconvolution
@pytest.mark.parametrize("cin,cout,k,pad,opad,H,W", E.UPCONV_GEOMS)
def test_pointwise_upconv(cin, cout, k, pad, opad, H, W):
    """ops.PointwiseUpconv with relu_pre into a channel slice of a wider map."""
    case = N.UpconvCase(cin, cout, k, pad, opad, H, W)
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
    oh, ow = layer.out_hw(H, W)

    def launch(x):
        out = torch.full((x.shape[0], total, oh, ow), -7.0, device=DEV)
        layer(x, out=out)
        assert bool((out[:, :off] == -7).all()) and bool((out[:, off + cout:] == -7).all()), "wrote outside its channel slice"
        return out[:, off:off + cout]
    holds(case, launch)


@pytest.mark.parametrize("impl", ["staged", "gather"])
@pytest.mark.parametrize("epilogue", N.DECONV_EPILOGUES)
@pytest.mark.parametrize("outs,cin_g,H,W,B", E.DECONV_GEOMS)
def test_grouped_deconv(outs, cin_g, H, W, B, epilogue, impl, monkeypatch):
    """ops.GroupedDeconv, plain, with a sigmoid and with the soft-max over each group's channels, on both kernels."""
    case = N.DeconvCase(outs, cin_g, H, W, B, epilogue)
    cts = []
    for o, w, b in zip(outs, case.ws, case.biases):
        ct = nn.ConvTranspose2d(cin_g, o, 3, stride=2, padding=1, output_padding=1)
        with torch.no_grad():
            ct.weight.copy_(w); ct.bias.copy_(b)
        cts.append(ct)
    layer = ops.GroupedDeconv(cts, sigmoid_from=1 if epilogue == "sigmoid" else -1, softmax=epilogue == "softmax", device=DEV)
    if impl == "gather":
        monkeypatch.setenv("LAV_DECONV_IMPL", "gather")
    else:
        monkeypatch.delenv("LAV_DECONV_IMPL", raising=False)
    holds(case, layer, f"{case.name}, {impl} kernel")


# ---------------------------------------------------------------------------------------------- ERFNet's entry, the pooled branch
@pytest.mark.parametrize("where", N.ERFNET_PLANTS)
@pytest.mark.parametrize("affine", [None, (2.0 / 255.0, -1.0)], ids=["plain", "affine"])
@pytest.mark.parametrize("geom", N.ERFNET_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_erfnet_entry(geom, affine, where):
    """ops.erfnet_entry: both blocks' ReLUs and both 2x2 poolings, the plant at the map's corner, in a pixel that is its pooling
    window's maximum, and in one that is not."""
    from tests import test_gpu_erfnet_edge as T
    case = N.ErfnetCase(*geom, affine, where)
    fused, _ = T.stages(False, affine)
    holds(case, lambda x: ops.erfnet_entry(x, *fused.args))


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "no relu"])
def test_pool_affine(relu):
    """ops.pool_affine into channels [2, 5) of a 7-channel buffer: the other channels keep their bits."""
    case = N.PoolAffineCase(relu)
    scale, shift = case.scale.float().to(DEV), case.shift.float().to(DEV)

    def launch(x):
        out = torch.full((2, case.total, 3, 4), 7.0, device=DEV)
        ops.pool_affine(x, scale, shift, out, case.off, relu=relu)
        beside = torch.cat([out[:, :case.off], out[:, case.off + 3:]], dim=1)
        assert bool((beside == 7).all()), "the other channels of the buffer were touched"
        return out[:, case.off:case.off + 3]
    holds(case, launch)


def test_heads_at_peaks():
    """ops.heads_at_peaks: a NaN in the feature map under the peak rows around (2, 2) and under the corner row reaches those rows' head
    columns and no other row."""
    case = N.HeadsCase()
    layer = ops.HeadsAtPeaks(case.heads, device=DEV)
    rows = torch.from_numpy(case.rows).to(DEV)
    holds(case, lambda x: layer(x, rows)[..., 3:])


def test_attn_pool():
    """ops.attn_pool (rgb.Attention in eval mode): the planted image's row is non-finite, the other rows keep their bits."""
    case = N.AttnCase()
    dm = copy.deepcopy(case.module).to(DEV).eval()

    def launch(x):
        with torch.no_grad():
            return dm(x)
    holds(case, launch)
    nan_rows = torch.isnan(N.references(case)["nan"][0]).all(dim=1)
    assert nan_rows.tolist() == [False, True, False]


# ---------------------------------------------------------------------------------------------- the training kernels
@pytest.mark.parametrize("mode", N.BN_MODES + ("mask",))
@pytest.mark.parametrize("shape", N.BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_act_and_bn_mask_act(shape, mode):
    """hipnn.bn_act / hipnn.bn_mask_act in train mode: the planted channel is non-finite everywhere and so are its running mean and
    variance, as in torch; every other channel and statistic keeps its bits."""
    from tests import test_gpu_kernel_size_paths as T
    assert N.BN_SHAPES[1] == T.BN_VEC_S2
    case = N.BnCase(shape, mode)

    def launch(x):
        bn = nn.BatchNorm2d(shape[1], eps=N.BN_EPS, momentum=N.BN_MOMENTUM).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(case.gamma); bn.bias.copy_(case.beta)
        if mode == "mask":
            y = hipnn.bn_mask_act(bn, x, case.res.to(DEV), case.m.to(DEV))
            assert type(y.grad_fn).__name__.startswith("_BnMask")
        else:
            y = hipnn.bn_act(bn, x, relu_pre=mode == "relu_pre", relu_post=mode in ("relu_post", "residual"),
                             residual=None if case.res is None else case.res.to(DEV))
            assert type(y.grad_fn).__name__.startswith("_BnAct"), "the torch modules ran, not lav_bn_train_*"
        return y, bn.running_mean, bn.running_var
    holds(case, launch)
    nan_ch = [bool(v) for v in torch.isnan(N.references(case)["nan"][1])]
    assert nan_ch == [c == 1 for c in range(shape[1])]


@pytest.mark.parametrize("Cn,W,d", N.PAIR_TRAIN_GEOMS)
def test_pair_train_forward(Cn, W, d):
    """hipnn.pair_train's forward (lav_pair_train_forward): the ReLU between the two convolutions."""
    case = N.PairTrainCase(Cn, W, d)
    wa, ba, wb, bb = (t.to(DEV) for t in (case.wa, case.ba, case.wb, case.bb))
    holds(case, lambda x: hipnn._PairTrain.apply(x, wa, ba, wb, bb, d))


@pytest.mark.parametrize("up", [False, True], ids=["seg_cross_entropy", "seg_cross_entropy_up"])
def test_seg_cross_entropy_forward(up, monkeypatch):
    """hipnn.seg_cross_entropy / seg_cross_entropy_up at (3, 8, 7, 13): the loss is NaN exactly when float64 F.cross_entropy's is (a NaN
    logit), non-finite exactly when it is non-finite (+Inf / -Inf logits), finite on clean logits."""
    import torch.nn.functional as F
    monkeypatch.setenv("LAV_TRAIN_CONV", "hip")
    s = 2 if up else 1
    g = torch.Generator().manual_seed(5)
    logits = torch.randn((3, 8, 7, 13), generator=g) * 3
    labels = torch.randint(0, 8, (3, 7 * s, 13 * s), generator=g)
    plants = [(0, 3, 3, 6), (2, 7, 6, 12)]
    for plant in ("clean",) + N.PLANTS:
        x = logits.clone()
        if plant != "clean":
            for i, at in enumerate(plants):
                x[at] = N.NAN if plant == "nan" else (N.INF if i == 0 else -N.INF)
        ref = F.cross_entropy(F.interpolate(x.double(), scale_factor=s) if up else x.double(), labels)
        lg = x.to(DEV).requires_grad_(True)
        if up:
            n0 = ops.train_work.get("seg_xent_up_calls", 0)
            loss = hipnn.seg_cross_entropy_up(lg, labels.to(DEV), s)
            assert ops.train_work["seg_xent_up_calls"] == n0 + 1
        else:
            loss = hipnn.seg_cross_entropy(lg, labels.to(DEV))
            assert type(loss.grad_fn).__name__.startswith("_SegXent")
        loss = loss.detach().cpu()
        assert bool(torch.isfinite(ref)) == (plant == "clean") and (plant != "nan" or bool(torch.isnan(ref)))
        if plant != "inf":          # (for Inf a NaN may stand in, as everywhere)
            assert bool(torch.isnan(loss)) == bool(torch.isnan(ref)), (plant, float(loss), float(ref))
        assert bool(torch.isfinite(loss)) == bool(torch.isfinite(ref)), (plant, float(loss), float(ref))
