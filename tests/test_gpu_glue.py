"""The small fused kernels that replaced torch / library launches inside the frame graphs, each against
the torch ops it stands in for, through the C ABI."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lav_amd import _lib, ops
from lav_amd.planner_common import transform_points

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("shape", [(1, 64, 48, 48), (7, 64, 96, 96), (2, 3, 5, 7)])
def test_maxpool3x3s2_is_max_pool2d(shape):
    """nn.MaxPool2d(3, 2, 1) of the ResNet-18 stem (lav/models/resnet.py:165,237)."""
    torch.manual_seed(1)
    x = torch.randn(shape, device=DEV)
    assert torch.equal(ops.maxpool3x3s2(x), F.max_pool2d(x, 3, 2, 1))


def test_channel_affine_is_the_brake_normalisation():
    """normalize(rgb / 255) (team_code_v2/models/rgb.py:71-72) as one per-channel affine."""
    torch.manual_seed(2)
    x = torch.rand((1, 3, 288, 768), device=DEV) * 255
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    s, t = (1.0 / (255.0 * std.double())).float().to(DEV), (-mean.double() / std.double()).float().to(DEV)
    want = (x.double().cpu() / 255.0 - mean.double()[None, :, None, None]) / std.double()[None, :, None, None]
    got = ops.channel_affine(x, s, t).double().cpu()
    assert (got - want).abs().max().item() < 2e-6


@pytest.mark.parametrize("B,K,O,sig", [(1, 1024, 1, True), (5, 512, 6, True), (3, 100, 7, False)])
def test_linear_act_vs_torch(B, K, O, sig):
    """nn.Sequential(Linear, Sigmoid): the brake classifier (rgb.py:62,79) and cast_cmd_pred (uniplanner.py:50-53)."""
    torch.manual_seed(3)
    x, w, b = torch.randn(B, K), torch.randn(O, K) / K ** 0.5, torch.randn(O)
    want = F.linear(x.double(), w.double(), b.double())
    want = torch.sigmoid(want) if sig else want
    got = ops.linear_act(x.to(DEV), w.to(DEV), b.to(DEV), sigmoid=sig).double().cpu()
    assert (got - want).abs().max().item() < 2e-6


def test_copy_many_copies_every_pair_in_one_launch():
    torch.manual_seed(4)
    srcs = [torch.randn(n, device=DEV) for n in (4, 1024, 3 * 288 * 256, 36, 2, 7, 20, 400, 13, 64)]    # 10 pairs: two launches; 8 / 28 / 52 bytes: partial last word
    dsts = [torch.full_like(s, 9.0) for s in srcs]
    guard = [torch.full((s.numel() + 8,), 5.0, device=DEV) for s in srcs]                                # nothing past the end may be written
    dsts = [g[:s.numel()] for g, s in zip(guard, srcs)]
    odd_src, odd_dst = torch.randn(9, device=DEV)[1:], torch.zeros(8, device=DEV)                        # misaligned source: copy_ fallback
    ops.copy_many(list(zip(dsts, srcs)) + [(odd_dst, odd_src)])
    for d, s in zip(dsts + [odd_dst], srcs + [odd_src]):
        assert torch.equal(d, s)
    for g, s in zip(guard, srcs):
        assert bool((g[s.numel():] == 5.0).all())


def test_grouped_deconv_softmax_epilogue_is_softmax_of_the_transposed_convolution():
    """ERFNet's output layer ConvTranspose2d(16, 5, 2, stride 2) + softmax over the classes (erfnet.py:140-142,
    lav_agent_fast.py:258) in one launch."""
    torch.manual_seed(5)
    ct = torch.nn.ConvTranspose2d(16, 5, 2, stride=2)
    x = torch.randn(3, 16, 36, 32)
    want = torch.softmax(ct.double()(x.double()), dim=1)
    ct = ct.float()
    got = ops.GroupedDeconv([ct], softmax=True, device=DEV)(x.to(DEV)).double().cpu()
    assert (got - want).abs().max().item() < 2e-6
    assert (got.sum(1) - 1).abs().max().item() < 1e-6


@pytest.mark.parametrize("B,hw,with_pose", [(1, 9, False), (4, 9, True), (15, 1, True)])
def test_embed_cast_is_pool_cast_cmd_pred_and_transform(B, hw, with_pose):
    """lav_embed_cast against its parts: AdaptiveAvgPool2d + Flatten (uniplanner.py:36-40), the six cast GRUs through
    lav_gru_cast (itself pinned by the reference goldens, :288-308), Linear + Sigmoid (:50-53) and transform_points + translate
    (model_inference.py:164-165,240-251)."""
    torch.manual_seed(6)
    E, H, ncmd, T = 512, 64, 6, 10
    side = int(round(hw ** 0.5))
    feat = torch.randn(B, E, side, side, device=DEV)
    w = dict(w_ih=torch.randn(ncmd, 3 * H, E, device=DEV) / E ** 0.5, w_hh=torch.randn(ncmd, 3 * H, H, device=DEV) / H ** 0.5,
             b_ih=torch.randn(ncmd, 3 * H, device=DEV) * 0.1, b_hh=torch.randn(ncmd, 3 * H, device=DEV) * 0.1,
             mlp_w=torch.randn(ncmd, 2, H, device=DEV) / H ** 0.5, mlp_b=torch.randn(ncmd, 2, device=DEV) * 0.1)
    cmd_w, cmd_b = torch.randn(ncmd, E, device=DEV) / E ** 0.5, torch.randn(ncmd, device=DEV)
    oris = torch.randn(B, device=DEV) if with_pose else None
    locs = torch.randn(B, 2, device=DEV) * 10 if with_pose else None
    embd, cast, cmds = ops.embed_cast(feat, w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"], w["mlp_w"], w["mlp_b"], T,
                                      cmd_w=cmd_w, cmd_b=cmd_b, oris=oris, locs=locs)
    want_embd = feat.double().mean((2, 3))
    assert (embd.double() - want_embd).abs().max().item() < 1e-6
    want_cast = ops.gru_cast(want_embd.float(), w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"], w["mlp_w"], w["mlp_b"], T)
    if with_pose:
        want_cast = transform_points(want_cast, oris[:, None].expand(B, ncmd)) + locs[:, None, None]
    assert (cast - want_cast).abs().max().item() < 2e-5
    want_cmds = torch.sigmoid(F.linear(want_embd, cmd_w.double(), cmd_b.double()))
    assert (cmds.double() - want_cmds).abs().max().item() < 2e-6


@pytest.mark.parametrize("case", [("head", 1, 384, 256, 3, 1, 1, 40, False), ("s2", 2, 64, 128, 3, 2, 1, 40, False),
                                  ("up", 2, 128, 64, 3, 2, 1, 20, True), ("res", 7, 128, 128, 3, 1, 1, 12, False),
                                  ("stem", 2, 384, 64, 7, 2, 3, 96, False)])   # (tap-pair mode of the split kernel, K = 18 816)
def test_split_operand_convolution_is_as_accurate_as_fp32(case):
    """precision bf16x6 (three bf16 pieces per operand, the six leading products on the bf16 matrix cores, fp32 accumulation)
    against a float64 convolution: its error stays at the fp32 kernel's level (both ~1e-6 of sum |a||b|), so the 1e-4 / 3e-5
    parity bars of the frame are met with either; LAV_CONV_PRECISION / lav_conv.precision selects."""
    name, B, cin, cout, k, s, p, H, tr = case
    torch.manual_seed(7)
    w = torch.randn((cin, cout, k, k) if tr else (cout, cin, k, k)) / (cin * k * k) ** 0.5
    x = torch.randn(B, cin, H, H)
    if tr:
        want = F.conv_transpose2d(x.double(), w.double(), None, s, p, 1)
        mag = F.conv_transpose2d(x.double().abs(), w.double().abs(), None, s, p, 1)
    else:
        want = F.conv2d(x.double(), w.double(), None, s, p)
        mag = F.conv2d(x.double().abs(), w.double().abs(), None, s, p)
    kw = dict(stride=s, padding=(p, p), transposed=tr, output_padding=1 if tr else 0, device=DEV)
    errs = {}
    for prec, label in ((_lib.CONV_F32, "f32"), (_lib.CONV_BF16X6, "bf16x6")):
        y = ops.ConvLayer(w, precision=prec, **kw)(x.to(DEV)).double().cpu()
        errs[label] = ((y - want).abs() / mag).max().item()
    print(name, errs)
    assert errs["f32"] < 2e-6 and errs["bf16x6"] < 2e-6, errs


def test_split_operand_convolution_at_the_edges_of_the_fp32_range(monkeypatch):
    """VERDICT r3 #9 / ADVICE r3: what precision bf16x6 does where fp32 ends.
    (1) Large magnitudes: every finite activation up to FLT_MAX is split exactly (the first piece of |x| above the largest finite
        bf16 is that bound - round 3's round-up carried into Inf there), so a layer fed +-3e38 .. FLT_MAX through weights small
        enough to keep the sums finite agrees with the exact-fp32 kernel to the usual 2e-6 of sum |a||b|.
    (2) fp32 SUBNORMAL inputs are flushed to zero by the bf16 matrix pipe (documented in lav_amd.h): the result is the
        convolution of the flushed input - finite, and equal to the fp32 kernel's on an input whose subnormals were zeroed.
    (3) A non-finite activation makes the outputs it reaches NaN (documented), never a finite number that could pass for data;
        pixels it does not reach are untouched.
    pad_value travels the same path (out-of-image taps read it and it is split like an activation): checked with a large one."""
    import ctypes
    monkeypatch.setenv("LAV_CONV_SPLIT", "2")     # the split kernel wherever it can take the layer (by cost this small one would go direct)
    torch.manual_seed(11)
    cin, cout, H = 64, 64, 24
    w = torch.randn(cout, cin, 3, 3) * 1e-3 / (cin * 9) ** 0.5
    kw = dict(stride=1, padding=(1, 1), device=DEV)

    def run(prec, x, **extra):
        layer = ops.ConvLayer(w, precision=prec, **kw, **extra)
        if prec == _lib.CONV_BF16X6:
            d = _lib.Conv.from_buffer_copy(layer.desc); d.batch, d.h, d.w = 1, H, H
            info = (ctypes.c_int * 9)()
            assert _lib.load().lav_conv_tile_info(ctypes.byref(d), info) == 0 and info[0] == -1, "the layer must run on k_conv_split"
        return layer(x.to(DEV)).double().cpu()
    # (1) magnitudes up to FLT_MAX, signs mixed
    big = torch.empty(1, cin, H, H).uniform_(2.0e38, 3.4e38) * torch.where(torch.rand(1, cin, H, H) < 0.5, -1.0, 1.0)
    big[0, 0, 0, 0], big[0, 1, 3, 3] = torch.finfo(torch.float32).max, -torch.finfo(torch.float32).max
    want = F.conv2d(big.double(), w.double(), None, 1, 1)
    mag = F.conv2d(big.double().abs(), w.double().abs(), None, 1, 1)
    for prec in (_lib.CONV_F32, _lib.CONV_BF16X6):
        y = run(prec, big)
        assert torch.isfinite(y).all()
        assert ((y - want).abs() / mag).max().item() < 2e-6, prec
    # the same through a large pad value (what out-of-image taps read)
    y_pad = run(_lib.CONV_BF16X6, big, pad_value=-3.0e38)
    want_pad = F.conv2d(F.pad(big.double(), (1, 1, 1, 1), value=-3.0e38), w.double(), None, 1, 0)
    mag_pad = F.conv2d(F.pad(big.double().abs(), (1, 1, 1, 1), value=3.0e38), w.double().abs(), None, 1, 0)
    assert ((y_pad - want_pad).abs() / mag_pad).max().item() < 2e-6
    # (2) subnormal activations (and ordinary ones beside them)
    x = torch.randn(1, cin, H, H)
    sub = torch.rand(1, cin, H, H) < 0.3
    x[sub] = torch.empty(int(sub.sum())).uniform_(1e-45, 1.1e-38)
    flushed = torch.where(x.abs() < torch.finfo(torch.float32).tiny, torch.zeros_like(x), x)
    y = run(_lib.CONV_BF16X6, x)
    assert torch.isfinite(y).all()
    ref = F.conv2d(flushed.double(), w.double(), None, 1, 1)
    mag = F.conv2d(flushed.double().abs(), w.double().abs(), None, 1, 1) + 1e-30
    assert ((y - ref).abs() / mag).max().item() < 2e-6, "bf16x6 on subnormal inputs = the convolution of the flushed input"
    # (3) Inf / NaN activations: NaN wherever they reach, ordinary values elsewhere
    x = torch.randn(1, cin, H, H)
    x[0, 5, 10, 10], x[0, 7, 2, 20] = float("inf"), float("nan")
    y = run(_lib.CONV_BF16X6, x)
    reach = torch.zeros(H, H, dtype=torch.bool)
    reach[9:12, 9:12] = True; reach[1:4, 19:22] = True
    assert torch.isnan(y[0][:, reach]).all(), "a non-finite activation may not come out as a finite number"
    clean = x.clone(); clean[0, 5, 10, 10] = 0.0; clean[0, 7, 2, 20] = 0.0
    assert torch.equal(y[0][:, ~reach], run(_lib.CONV_BF16X6, clean)[0][:, ~reach])


@pytest.mark.parametrize("prec", [_lib.CONV_F32, _lib.CONV_BF16X6, _lib.CONV_F16X3])
@pytest.mark.parametrize("case", [(64, 128, 3, 2, False), (128, 64, 4, 2, True), (384, 256, 3, 1, False)])
def test_conv_layer_refresh_repacks_on_the_device_bit_for_bit(case, prec):
    """ConvLayer.refresh (lav_conv_repack + lav_bn_fold: the trainer's per-step log inference re-packs its student this way)
    after an in-place parameter update == a layer built anew from the updated parameters: packed weights, bias, BatchNorm affine.
    LAV_CONV_F16X3 (round 6, lav_conv_repack_scratch): the fp16 section too - its scale is the power of two of the UPDATED weights'
    largest magnitude, measured on the device (the update below changes it)."""
    cin, cout, k, s, tr = case
    torch.manual_seed(8)
    w = torch.nn.Parameter(torch.randn((cin, cout, k, k) if tr else (cout, cin, k, k), device=DEV) * 0.05)
    bias = torch.nn.Parameter(torch.randn(cout, device=DEV))
    bn = tuple(t.to(DEV) for t in (torch.randn(cout), torch.rand(cout) + 0.5, torch.rand(cout) + 0.5, torch.randn(cout)))
    kw = dict(stride=s, padding=(1, 1), transposed=tr, bias=bias, bn=bn, bn_eps=1e-3, relu_pre=True, precision=prec, device=DEV)
    layer = ops.ConvLayer(w, **kw)
    with torch.no_grad():
        w.add_(torch.randn_like(w) * 0.01); bias.mul_(1.1)
        w.view(-1)[5] = 3.7            # (a new largest weight: the fp16 section's scale doubles at least once)
        for t in bn:
            t.add_(0.01)
    layer.refresh()
    fresh = ops.ConvLayer(w, **kw)
    assert torch.equal(layer.w.view(torch.int32), fresh.w.view(torch.int32))
    assert torch.equal(layer.bias, fresh.bias) and torch.equal(layer.scale, fresh.scale) and torch.equal(layer.shift, fresh.shift)


def test_engines_follow_in_place_parameter_updates_across_train_eval_toggles():
    """The trainer's pattern (lav_amd/train/lav.py:mot_inference): eval-mode inference, train(), an optimiser step in place,
    eval() again - the cached engines are re-packed on the device and give what a model built from the new weights gives."""
    import copy
    import lav_amd
    from tests.util import CFG, state_dicts
    lm = lav_amd.LiDARModel(num_input=16, backbone="cnn", num_features=[64, 64], **CFG)
    lm.load_state_dict(state_dicts()[0])
    lm = lm.to(DEV).eval()
    x = torch.randn(1, 64, 320, 320, device=DEV).relu()
    with torch.no_grad():
        f0 = lm.backbone(x); h0 = lm.heads(f0)
        lm.train()
        for p in lm.parameters():
            p.add_(torch.randn_like(p) * 0.02)
        for m in lm.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.add_(0.05); m.running_var.mul_(1.2)
        lm.eval()
        f1 = lm.backbone(x); h1 = lm.heads(f1)
        ref = lav_amd.LiDARModel(num_input=16, backbone="cnn", num_features=[64, 64], **CFG)
        ref.load_state_dict(copy.deepcopy(lm.state_dict()))
        ref = ref.to(DEV).eval()
        f2 = ref.backbone(x); h2 = ref.heads(f2)
    assert not torch.equal(f0, f1)
    assert torch.equal(f1, f2)
    for a, b in zip(h1, h2):
        assert torch.equal(a, b)


def _erfnet(prec):
    from lav_amd.erfnet import ERFNet
    x = torch.rand(1, 3, 32, 256, device=DEV) * 255       # the three downsamplers give the pair kernels' widths 128, 64 and 32

    def run(m):
        with ops.precision(prec):
            return m(x, input_affine=(2.0 / 255.0, -1.0), softmax=True)
    return (lambda: ERFNet(5)), run


def _brake_trunk():
    from lav_amd.rgb import RGBBrakePredictionModel
    x = torch.rand(1, 3, 64, 64, device=DEV) * 255
    return (lambda: RGBBrakePredictionModel([4, 6, 7, 10, 18])), (lambda m: m.trunk(x))


def _pillar():
    from lav_amd.point_pillar import PointPillarNet
    pts = torch.rand(1, 300, 11, device=DEV)
    pts[..., 0] *= 16; pts[..., 1] = pts[..., 1] * 16 - 8                 # inside the 32x32 grid
    return (lambda: PointPillarNet(16, [64, 64], min_x=0, max_x=16, min_y=-8, max_y=8, pixels_per_meter=2)), (lambda m: m(pts, [300]))


@pytest.mark.parametrize("case", ["erfnet-f16x3", "erfnet-default", "brake-trunk", "pillar"])
def test_engines_of_the_other_modules_follow_in_place_updates_across_train_eval_toggles(case):
    """The same pattern on the modules whose caches are plain copies (ERFNet's packed pairs at both precisions, the folded PointNet,
    the brake net's input affine) or sit behind another module (its ResNet-18 trunk): eval output, train(), every parameter and running
    statistic changed in place, eval() - bit for bit what a model freshly built from the new state_dict gives."""
    import copy
    torch.manual_seed(21)
    make, run = {"erfnet-f16x3": lambda: _erfnet(_lib.CONV_F16X3), "erfnet-default": lambda: _erfnet(0),
                 "brake-trunk": _brake_trunk, "pillar": _pillar}[case]()
    m = make().to(DEV).eval()
    with torch.no_grad():
        y0 = run(m).clone()
        m.train()
        for p in m.parameters():
            p.add_(torch.randn_like(p) * 0.02)
        for b in m.modules():
            if isinstance(b, torch.nn.modules.batchnorm._BatchNorm):
                b.running_mean.add_(0.05); b.running_var.mul_(1.2)
        m.eval()
        y1 = run(m).clone()
        ref = make()
        ref.load_state_dict(copy.deepcopy(m.state_dict()))
        y2 = run(ref.to(DEV).eval())
    assert y0.shape == y1.shape and not torch.equal(y0, y1)
    assert torch.equal(y1, y2)


@pytest.mark.parametrize("B,cin,cout,H", [(57, 128, 64, 12), (2, 256, 128, 6), (16, 64, 32, 40)])
def test_transposed_convolution_with_empty_parity_classes(B, cin, cout, H):
    """ConvTranspose2d(k=1, stride=2, output_padding=1) - the adjoint of ResNet's 1x1 stride-2 down-sampling convolutions: three
    of the four output-parity classes have no tap at all (zeros).  The split-operand kernel's loaders would read past the packed
    weights there (found by tools/train_conv_probe.py as a memory fault): such layers must plan onto the fp32 kernels."""
    torch.manual_seed(9)
    w = torch.randn(cin, cout, 1, 1) / cin ** 0.5
    x = torch.randn(B, cin, H, H)
    want = F.conv_transpose2d(x.double(), w.double(), None, 2, 0, 1)
    layer = ops.ConvLayer(w, stride=2, padding=(0, 0), transposed=True, output_padding=1, device=DEV)
    d = _lib.Conv.from_buffer_copy(layer.desc); d.batch, d.h, d.w = B, H, H
    import ctypes
    info = (ctypes.c_int * 9)()
    assert _lib.load().lav_conv_tile_info(ctypes.byref(d), info) == 0 and info[0] != -1
    for _ in range(3):
        got = layer(x.to(DEV))
    torch.cuda.synchronize()
    assert (got.double().cpu() - want).abs().max().item() < 1e-5


def test_copy_many_stages_strided_and_uint8_tensors_like_copy_():
    """lav_stage_many: the camera tensors of a tick (channels-last views, float32 or uint8) into contiguous float32 buffers,
    together with an expanded / sliced 2-D tensor: exactly what Tensor.copy_ gives."""
    torch.manual_seed(10)
    hwc = torch.randint(0, 256, (3, 288, 256, 3), dtype=torch.uint8, device=DEV)
    a_src = hwc.permute(0, 3, 1, 2)                                                    # (3,3,288,256) uint8, channels last
    b_src = torch.rand(1, 192, 480, 3, device=DEV).permute(0, 3, 1, 2) * 255           # float32, channels last
    c_src = torch.randn(10, 7, device=DEV)[::2, 1:6]                                   # 2-D strided
    d_src = torch.randn(5, device=DEV)[1:]                                             # misaligned contiguous 1-D
    e_src = torch.randn(64, 4, device=DEV)                                             # contiguous: the 16-byte-word path
    srcs = [a_src, b_src, c_src, d_src, e_src]
    dsts = [torch.full(s.shape, -7.0, dtype=torch.float32, device=DEV) for s in srcs]
    ops.copy_many(list(zip(dsts, srcs)))
    for d, s in zip(dsts, srcs):
        want = torch.empty_like(d); want.copy_(s)
        assert torch.equal(d, want)
    # lav_stage_many_block: 176 bytes of host data ride in the same launch's kernel arguments (the frame's pose block); the host
    # buffer may change right after the call
    blk = torch.randint(0, 256, (176,), dtype=torch.uint8)
    want_blk = blk.clone()
    d_blk = torch.zeros(176, dtype=torch.uint8, device=DEV)
    for d in dsts:
        d.fill_(-7.0)
    ops.copy_many(list(zip(dsts, srcs)), block=(d_blk, blk))
    blk.zero_()
    assert torch.equal(d_blk.cpu(), want_blk)
    for d, s in zip(dsts, srcs):
        want = torch.empty_like(d); want.copy_(s)
        assert torch.equal(d, want)
    # a block that does not fit the arguments (or no staging launch to ride in) takes Tensor.copy_
    big = torch.randint(0, 256, (512,), dtype=torch.uint8)
    d_big = torch.zeros(512, dtype=torch.uint8, device=DEV)
    ops.copy_many(list(zip(dsts, srcs)), block=(d_big, big))
    assert torch.equal(d_big.cpu(), big)
