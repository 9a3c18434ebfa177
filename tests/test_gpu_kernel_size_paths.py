"""The training kernels that dispatch on size, on the far side of that dispatch, each at the smallest shape that gets there:
lav_bn_train_* on more than one slice per channel (slices that end inside a plane, a short last slice, the 64-slice clamp, the
scalar kernels and the masked variant across a slice boundary, one amax part per slice, data with |mean| >> sigma),
lav_seg_xent_forward / lav_seg_xent_up_forward on more pixels than one trip of their capped grid covers (and every class count
and the ends of the scale range), lav_attn_train_* / lav_attn_pool at the channel, head-width and token bounds they accept.
References are torch ops in float64 on the host over the same float32 inputs; every bar is that of the kernel's existing unit
test; every kernel result is bit-identical on a second launch."""
import copy

import pytest
import torch
import torch.nn.functional as F

from lav_amd import _lib, ops
from lav_amd.train import hipnn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# (B, C, H, W) -> slices per channel (geometry(), csrc/bn_train.hip); asserted by every case through lav_bn_train_amax_count
BN_VEC_S2 = (3, 3, 52, 56)       # N = 8736: the boundary falls 1456 floats into image 1
BN_VEC_S3 = (5, 8, 64, 64)       # N = 20480: 6828 per slice, the last one 4 short
BN_SCALAR_S2 = (3, 5, 53, 55)    # odd plane (scalar kernels), N = 8745: the boundary falls mid-row into image 1
BN_VEC_S64 = (2, 2, 512, 516)    # N = 528384: 65 slices wanted, clamped to 64
BN_SMALLEST = (2, 7, 1, 1)       # N = 2, the least the ABI accepts
BN_SLICES = {BN_VEC_S2: 2, BN_VEC_S3: 3, BN_SCALAR_S2: 2, BN_VEC_S64: 64, BN_SMALLEST: 1}
BN_NAMES = ["y", "running_mean", "running_var", "dx", "dgamma", "dbeta", "dres"]


def _assert_slices(shape, S):
    B, C, H, W = shape
    assert _lib.load().lav_bn_train_amax_count(B, C, H * W) == C * S


def _bn(C, device, dtype, momentum=0.01):
    bn = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=momentum).to(device=device, dtype=dtype).train()
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(0.5, 1.5, C)); bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
    return bn


def _bn_act_run(x, res, dy, mode, device, dtype, momentum=0.01):
    """test_bn_act_forward_backward_vs_torch's run: y, running statistics and every gradient of one bn_act step."""
    kw = dict(relu_pre=mode == "relu_pre", relu_post=mode in ("relu_post", "residual"))
    bn = _bn(x.shape[1], device, dtype, momentum)
    xx = x.to(device=device, dtype=dtype).requires_grad_(True)
    rr = None if res is None else res.to(device=device, dtype=dtype).requires_grad_(True)
    y = hipnn.bn_act(bn, xx, residual=rr, **kw)
    if xx.is_cuda:
        assert type(y.grad_fn).__name__.startswith("_BnAct"), "the torch modules ran, not lav_bn_train_*"
    y.backward(dy.to(device=device, dtype=dtype))
    out = [y.detach(), bn.running_mean, bn.running_var, xx.grad, bn.weight.grad, bn.bias.grad]
    if rr is not None:
        out.append(rr.grad)
    assert int(bn.num_batches_tracked) == 1
    return [t.detach().double().cpu() for t in out]


def _off_the_kink(dy, x, splits, res=None, m=None):
    """dy with zeros where the float64 pre-activation z of a trailing ReLU lies within the output's own bar (1e-4 of max(|z|, 1))
    of zero.  There the ReLU's derivative is not determined at float32 precision - a forward within its bar may land on either
    side, and one flipped element moves dx by gamma rstd dy, thousands of bars - so the upstream gradient carries no weight
    there.  The choice is made from the reference alone; y itself is compared at every element."""
    w = torch.cat([torch.linspace(0.5, 1.5, c) for c in splits]).double()
    b = torch.cat([torch.linspace(-0.3, 0.3, c) for c in splits]).double()
    z = F.batch_norm(x.double(), None, None, w, b, True, 0.0, 1e-3)
    if m is not None:
        z = m.double()[:, :, None, None] * z
    if res is not None:
        z = z + res.double()
    keep = z.abs() > 1e-4 * max(z.abs().max().item(), 1.0)
    assert keep.double().mean().item() > 0.99            # (a handful of elements, not a hollowed-out gradient)
    return dy * keep.to(dy.dtype)


def _bn_compare(names, got, ref, again):
    for n, a, b, c in zip(names, got, ref, again):
        assert torch.equal(a, c), f"{n}: two runs differ"
        scale = max(b.abs().max().item(), 1.0)
        err = (a - b).abs().max().item()
        assert err <= 1e-4 * scale, (n, err, scale)


@pytest.mark.parametrize("shape", list(BN_SLICES), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["plain", "relu_pre", "relu_post", "residual"])
def test_bn_act_past_one_slice_vs_torch(shape, mode):
    """hipnn.bn_act at shapes whose channels are cut into 2, 3 and 64 slices (and N = 2) against nn.BatchNorm2d + F.relu in float64:
    output, running statistics and all four gradients within 1e-4 of max(|ref|, 1); a second run bit-identical."""
    _assert_slices(shape, BN_SLICES[shape])
    torch.manual_seed(3)
    x = torch.randn(shape) * 1.5 + 0.3
    res = torch.randn(shape) if mode == "residual" else None
    dy = torch.randn(shape)
    if mode in ("relu_post", "residual"):
        dy = _off_the_kink(dy, x, [shape[1]], res)
    ref = _bn_act_run(x, res, dy, mode, "cpu", torch.float64)
    got = _bn_act_run(x, res, dy, mode, DEV, torch.float32)
    again = _bn_act_run(x, res, dy, mode, DEV, torch.float32)
    _bn_compare(BN_NAMES, got, ref, again)


def test_bn_act_one_value_per_channel_fails_loudly():
    """Batch statistics of a single value: lav_bn_train_forward refuses before any launch (no step is counted anywhere)."""
    assert _lib.load().lav_bn_train_amax_count(1, 7, 1) == 0
    bn = _bn(7, DEV, torch.float32)
    x = torch.randn((1, 7, 1, 1), device=DEV, requires_grad=True)
    n0 = ops.train_work["bn_train_fwd_bytes"]
    with pytest.raises(RuntimeError, match="more than one value per channel"):
        hipnn.bn_act(bn, x)
    assert ops.train_work["bn_train_fwd_bytes"] == n0 and int(bn.num_batches_tracked) == 0
    assert torch.equal(bn.running_mean.cpu(), torch.zeros(7)) and torch.equal(bn.running_var.cpu(), torch.ones(7))


@pytest.mark.parametrize("shape", [BN_VEC_S2, BN_SCALAR_S2], ids=["vector", "scalar"])
def test_bn_mask_act_past_one_slice_vs_torch(shape):
    """hipnn.bn_mask_act (lav_bn_train_*_mask) on two slices per channel - the mask's chmask[at / HW] lookup on both sides of a
    boundary inside image 1 - against relu(m * bn(z) + residual) in float64, a drawn mask with zeros in it."""
    _assert_slices(shape, 2)
    B, C, H, W = shape
    torch.manual_seed(11)
    z = torch.randn(shape) * 1.5 + 0.3
    res, dy = torch.randn(shape), torch.randn(shape)
    m = hipnn.dropout2d_mask(0.3, B, C, "cpu")
    assert bool((m == 0).any()) and bool((m > 0).any())
    dy = _off_the_kink(dy, z, [C], res, m)

    def run(device, dtype):
        bn = _bn(C, device, dtype)
        zz = z.to(device=device, dtype=dtype).requires_grad_(True)
        rr = res.to(device=device, dtype=dtype).requires_grad_(True)
        mm = m.to(device=device, dtype=dtype)
        if zz.is_cuda:
            y = hipnn.bn_mask_act(bn, zz, rr, mm)
            assert type(y.grad_fn).__name__.startswith("_BnMask")
        else:
            y = F.relu(mm[:, :, None, None] * bn(zz) + rr)
        y.backward(dy.to(device=device, dtype=dtype))
        assert int(bn.num_batches_tracked) == 1
        return [t.detach().double().cpu() for t in (y, bn.running_mean, bn.running_var, zz.grad, bn.weight.grad, bn.bias.grad, rr.grad)]

    ref = run("cpu", torch.float64)
    got, again = run(DEV, torch.float32), run(DEV, torch.float32)
    _bn_compare(["y", "running_mean", "running_var", "dz", "dgamma", "dbeta", "dres"], got, ref, again)


@pytest.mark.parametrize("mode", ["relu_pre", "relu_post"])
def test_bn_act_many_past_one_slice_vs_modules_one_by_one(mode):
    """hipnn.bn_act_many: modules of 3 and 5 channels over one 8-channel tensor in one launch pair on three slices, against the two
    modules run one by one in float64 (the host path of the same function); each module's running statistics are its channels'."""
    shape = BN_VEC_S3
    _assert_slices(shape, 3)
    torch.manual_seed(13)
    x = torch.randn(shape) * 1.5 + 0.3 + torch.arange(8.0)[None, :, None, None]      # (every channel its own mean)
    dy = torch.randn(shape)
    if mode == "relu_post":
        dy = _off_the_kink(dy, x, [3, 5])
    kw = dict(relu_pre=mode == "relu_pre", relu_post=mode == "relu_post")

    def run(device, dtype):
        bns = [_bn(3, device, dtype), _bn(5, device, dtype)]
        xx = x.to(device=device, dtype=dtype).requires_grad_(True)
        y = hipnn.bn_act_many(bns, xx, **kw)
        if xx.is_cuda:
            assert type(y.grad_fn).__name__.startswith("_BnAct"), "one launch pair for both modules"
        y.backward(dy.to(device=device, dtype=dtype))
        out = [y, xx.grad]
        for bn in bns:
            assert int(bn.num_batches_tracked) == 1
            out += [bn.running_mean, bn.running_var, bn.weight.grad, bn.bias.grad]
        return [t.detach().double().cpu() for t in out]

    ref = run("cpu", torch.float64)
    got, again = run(DEV, torch.float32), run(DEV, torch.float32)
    names = ["y", "dx"] + [f"{n}[{i}]" for i in (0, 1) for n in ("running_mean", "running_var", "dgamma", "dbeta")]
    assert [tuple(t.shape) for t in got[2:]] == [(3,)] * 4 + [(5,)] * 4
    _bn_compare(names, got, ref, again)


@pytest.mark.parametrize("shape", [BN_VEC_S3, BN_VEC_S64], ids=["S3", "S64"])
@pytest.mark.parametrize("mode", ["relu_pre", "residual"])
def test_bn_act_amax_parts_past_one_slice(shape, mode, monkeypatch):
    """Under f16x3 the BatchNorm launches leave one maximum per (channel, slice): C * S parts on y and on dx, whose largest is
    exactly max |y| resp. max |dx|."""
    monkeypatch.delenv("LAV_TRAIN_PRECISION", raising=False)
    monkeypatch.delenv("LAV_TRAIN_BN_AMAX", raising=False)
    S = BN_SLICES[shape]
    _assert_slices(shape, S)
    B, C, H, W = shape
    torch.manual_seed(7)
    x0 = (torch.randn(shape) * 2.0).to(DEV).requires_grad_(True)
    res = torch.randn(shape).to(DEV) if mode == "residual" else None
    bn = _bn(C, DEV, torch.float32)
    seen = []
    with hipnn.use_precision("f16x3"):
        x = x0 * 1.0            # (not a leaf: its hook sees the object the BatchNorm's backward returned, not an accumulated copy)
        x.register_hook(lambda g: seen.append((hipnn._trusted(g), g.detach().abs().max().item())) and None)
        y = hipnn.bn_act(bn, x, residual=res, relu_pre=mode == "relu_pre", relu_post=mode == "residual")
        am = hipnn._trusted(y)
        assert am is not None and am.count == C * S
        assert am.buf[:am.count].max().item() == y.detach().abs().max().item()
        y.backward(torch.randn(shape).to(DEV))
    assert len(seen) == 1
    tag, dx_max = seen[0]
    assert dx_max == x0.grad.abs().max().item() and dx_max > 0
    for t in (tag, hipnn._trusted(x0.grad)):      # (leaf gradients are accumulated into .grad by autograd: the object may be a copy)
        if t is not None:
            assert t.count == C * S
            assert t.buf[:t.count].max().item() == dx_max
    assert tag is not None, "autograd handed the hook another object than the BatchNorm's backward tagged"


@pytest.mark.parametrize("shape", [BN_VEC_S2, (4, 64, 40, 40)], ids=["S2", "4x64x40x40"])
@pytest.mark.parametrize("mode", ["plain", "relu_post"])
def test_bn_act_offset_data_keeps_its_variance(shape, mode):
    """x = 10 + 0.1 randn (|mean| = 100 sigma): sum x and sum x^2 are accumulated in float64, so the variance survives the
    cancellation.  The float32 saved mean costs at most 2^-24 |mean| rstd ~ 6e-6 in xhat, an order under the 1e-4 of
    max(|ref|, 1) every output is held to; a float32 sum of squares (relative error >= 6e-8 of 100 against a variance of 0.01:
    6e-4 of it) would miss the 1e-4 RELATIVE bar the saved and the running variance are held to here (momentum 1: the running
    statistics are the batch's)."""
    B, C, H, W = shape
    if shape == BN_VEC_S2:
        _assert_slices(shape, 2)
    torch.manual_seed(17)
    x = 10 + 0.1 * torch.randn(shape)
    dy = torch.randn(shape)
    if mode == "relu_post":
        dy = _off_the_kink(dy, x, [C])
    ref = _bn_act_run(x, None, dy, mode, "cpu", torch.float64, momentum=1.0)
    got = _bn_act_run(x, None, dy, mode, DEV, torch.float32, momentum=1.0)
    again = _bn_act_run(x, None, dy, mode, DEV, torch.float32, momentum=1.0)
    _bn_compare(BN_NAMES, got, ref, again)
    n = B * H * W
    var = x.double().var(dim=(0, 2, 3), unbiased=False)
    assert 0.005 < var.min().item() and var.max().item() < 0.02
    assert ((ref[2] - var * n / (n - 1)).abs() <= 1e-12).all()           # (the reference's running variance IS the batch's)
    assert ((got[2] - ref[2]).abs() <= 1e-4 * ref[2]).all(), ("running_var", ((got[2] - ref[2]).abs() / ref[2]).max().item())
    bn = _bn(C, DEV, torch.float32)
    _, mean, saved = hipnn._BnAct.apply(x.to(DEV), bn.weight, bn.bias, None, bn.eps, False, mode == "relu_post")
    assert ((saved.double().cpu() - var).abs() <= 1e-4 * var).all(), ("saved var", ((saved.double().cpu() - var).abs() / var).max().item())
    assert ((mean.double().cpu() - x.double().mean(dim=(0, 2, 3))).abs() <= 1e-4 * 10).all()


# ------------------------------------------------------------------------------------------------------------ segmentation losses
def _xent_cap():
    return _lib.load().lav_seg_xent_workspace_bytes() // 8


@pytest.mark.parametrize("B,Cn,H,W", [(2, 2, 600, 500), (1, 8, 513, 512)])
def test_seg_xent_past_the_workgroup_cap_vs_float64(B, Cn, H, W, monkeypatch):
    """lav_seg_xent_forward on more pixels than 256 x the capped grid: 600 000 (threads make two and three trips) and one pixel
    row past the cap with all 8 classes.  test_seg_xent_kernel_vs_float64's bars: loss at 1e-6 relative, dlogits at 1e-6 of the
    largest reference gradient; two runs bit-identical."""
    monkeypatch.setenv("LAV_TRAIN_CONV", "hip")
    assert B * H * W > 256 * _xent_cap()
    g = torch.Generator().manual_seed(B * Cn + H)
    logits = torch.randn((B, Cn, H, W), generator=g) * 4
    labels = torch.randint(0, Cn, (B, H, W), generator=g)
    assert len(labels.unique()) == Cn
    outs = []
    for _ in range(2):
        lg = logits.to(DEV).requires_grad_(True)
        loss = hipnn.seg_cross_entropy(lg, labels.to(DEV))
        assert type(loss.grad_fn).__name__.startswith("_SegXent")
        (loss * 3.0).backward()
        outs.append((loss.detach().cpu(), lg.grad.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    lr = logits.double().requires_grad_(True)
    ref = F.cross_entropy(lr, labels)
    (ref * 3.0).backward()
    assert abs(outs[0][0].item() - ref.item()) <= 1e-6 * abs(ref.item()), (outs[0][0].item(), ref.item())
    err = (outs[0][1].double() - lr.grad).abs().max().item()
    assert err <= 1e-6 * lr.grad.abs().max().item(), (err, lr.grad.abs().max().item())


@pytest.mark.parametrize("B,K,h,w,s,dtype,big", [
    (2, 3, 400, 330, 2, torch.uint8, True), (2, 3, 400, 330, 2, torch.int64, True),      # 264 000 cells: past the cap
    (2, 8, 5, 7, 1, torch.int64, False), (3, 1, 4, 4, 3, torch.uint8, False), (2, 2, 1, 2, 64, torch.uint8, False),
    (1, 5, 3, 2, 7, torch.int64, False)])
def test_seg_xent_up_past_the_cap_and_at_the_ends_vs_float64(B, K, h, w, s, dtype, big, monkeypatch):
    """lav_seg_xent_up_forward past the grid cap and at 1 and 8 classes, scales 1, 3, 7 and 64, against float64
    F.cross_entropy(F.interpolate(.)): test_seg_cross_entropy_up_matches_float64's 1e-5 relative on the loss and on dlogits (one
    class: loss and gradient are zero up to rounding, held to 1e-6 absolute); two runs bit-identical."""
    monkeypatch.delenv("LAV_TRAIN_CONV", raising=False)
    if big:
        assert B * h * w > 256 * _xent_cap()
    g = torch.Generator().manual_seed(K * 10 + s)
    logits = torch.randn(B, K, h, w, generator=g) * 3
    labels = torch.randint(0, K, (B, h * s, w * s), generator=g).to(dtype)
    l64 = logits.double().requires_grad_(True)
    ref = F.cross_entropy(F.interpolate(l64, scale_factor=s), labels.long())
    ref.backward()
    outs = []
    for _ in range(2):
        lg = logits.to(DEV).requires_grad_(True)
        n0 = ops.train_work.get("seg_xent_up_calls", 0)
        loss = hipnn.seg_cross_entropy_up(lg, labels.to(DEV), s)
        assert ops.train_work["seg_xent_up_calls"] == n0 + 1          # (the kernel ran, not the torch ops)
        (loss * 2).backward()
        outs.append((loss.detach().cpu(), lg.grad.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    loss, grad = outs[0][0].item(), outs[0][1].double() / 2
    err = (grad - l64.grad).abs().max().item()
    if K == 1:
        assert ref.item() == 0 and l64.grad.abs().max().item() == 0
        assert abs(loss) <= 1e-6 and err <= 1e-6, (loss, err)
    else:
        assert abs(loss - ref.item()) <= 1e-5 * abs(ref.item()), (loss, ref.item())
        assert err <= 1e-5 * l64.grad.abs().max().item() + 1e-30, (err, l64.grad.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------- attention
ATTN_SHAPES = [(2, 1024, 8, 2, 3),     # pooled-map loop: second pass; head width 128: output loop second pass; N = 6, not a multiple of 4
               (1, 16, 8, 64, 64),     # N = 4096, the LDS bound; head width 2
               (2, 64, 8, 1, 1),       # N = 1: soft-max of one token, p = 1, dd = 0
               (2, 768, 4, 3, 5)]      # head width 192: output loop three passes; odd N, rows not 16-byte aligned


def _attention(C, heads, seed):
    from lav_amd.rgb import Attention
    torch.manual_seed(seed)
    m = Attention(C, num_heads=heads)
    with torch.no_grad():                    # (a trained-looking scale: dots of a few units, not a one-hot soft-max)
        m.q.mul_(0.5)
        m.linear_kv.bias.normal_(0, 0.1)
    return m.train()


def _close(got, ref, name, rel=1e-4):
    ref = ref.double().cpu()
    err = (got.double().cpu() - ref).abs().max().item()
    assert err <= rel * ref.abs().max().item() + 1e-30, f"{name}: max error {err:.3g} vs max |ref| {ref.abs().max().item():.3g}"


def _attn_input(B, C, h, w):
    g = torch.Generator().manual_seed(h * w + C)
    return torch.relu(torch.randn(B, C, h, w, generator=g)) * 2, torch.randn(B, C, generator=g)


@pytest.mark.parametrize("B,C,heads,h,w", ATTN_SHAPES)
def test_attn_pool_train_at_the_bounds_vs_float64_autograd(B, C, heads, h, w, monkeypatch):
    """hipnn.attn_pool_train (lav_attn_train_*) at 1024 channels, head widths 2, 128 and 192, 1 and 4096 tokens against the module's
    float64 autograd; harness and bars of test_attn_pool_train_matches_float64_autograd."""
    monkeypatch.delenv("LAV_TRAIN_CONV", raising=False)
    m = _attention(C, heads, seed=B * 1000 + h)
    x, dout = _attn_input(B, C, h, w)
    ref = copy.deepcopy(m).double()
    x64 = x.double().requires_grad_(True)
    out64 = ref(x64)
    out64.backward(dout.double())

    def run():
        mm = copy.deepcopy(m).to(DEV)
        xx = x.to(DEV).requires_grad_(True)
        n0 = ops.train_work.get("attn_train_calls", 0)
        out = hipnn.attn_pool_train(mm, xx)
        assert ops.train_work["attn_train_calls"] == n0 + 1          # (the kernel ran, not the module's torch ops)
        out.backward(dout.to(DEV))
        torch.cuda.synchronize()
        return [t.detach().cpu().clone() for t in (out, xx.grad, mm.q.grad, mm.linear_kv.weight.grad, mm.linear_kv.bias.grad)]

    got = run()
    for t, r, name in zip(got, (out64, x64.grad, ref.q.grad, ref.linear_kv.weight.grad, ref.linear_kv.bias.grad),
                          ("out", "dx", "dq", "dW_kv", "db_kv")):
        if name == "db_kv":    # the key half is zero up to rounding (the soft-max is shift invariant): an absolute bar on it
            _close(t[C:], r[C:], "db_v")
            assert t[:C].abs().max().item() <= 1e-4 * r[C:].abs().max().item() + 1e-6, "db_k"
        else:
            _close(t, r, name)
    again = run()
    for a, b_ in zip(got, again):
        assert torch.equal(a, b_), "a repeat is not bit-identical"


@pytest.mark.parametrize("B,C,heads,h,w", ATTN_SHAPES + [(3, 512, 8, 6, 15)])
def test_attn_pool_eval_vs_float64_and_follows_its_parameters(B, C, heads, h, w):
    """Attention.eval() on the device (lav_attn_pool: k_attn_pool<false>, float4 loads of W_v, u and the bias folded on the host)
    against the same module's train-mode torch forward in float64, within 1e-4 of max |ref|; after an in-place change of q and
    then of linear_kv the folded u, bias, W_v and b_v follow (the class docstring's promise)."""
    m = _attention(C, heads, seed=B * 1000 + h)
    x, _ = _attn_input(B, C, h, w)
    dm = copy.deepcopy(m).to(DEV).eval()
    xd = x.to(DEV)

    def reference():
        with torch.no_grad():
            return copy.deepcopy(dm).cpu().double().train()(x.double())

    def device():
        with torch.no_grad():
            out = dm(xd)
            again = dm(xd)
        torch.cuda.synchronize()
        assert torch.equal(out, again), "a repeat is not bit-identical"
        return out.cpu()

    ref0 = reference()
    _close(device(), ref0, "out")
    with torch.no_grad():
        dm.q.mul_(-1.5)                          # u and the dots' bias change, W_v and b_v do not
    ref1 = reference()
    if h * w > 1:                                # (one token: p = 1 whatever the query)
        assert (ref1 - ref0).abs().max().item() > 1e-2 * ref0.abs().max().item()
    _close(device(), ref1, "out after q changed in place")
    with torch.no_grad():
        dm.linear_kv.weight.mul_(0.75)
        dm.linear_kv.bias.add_(0.25)
    ref2 = reference()
    assert (ref2 - ref1).abs().max().item() > 1e-2 * ref1.abs().max().item()
    _close(device(), ref2, "out after linear_kv changed in place")


@pytest.mark.parametrize("B,C,heads,h,w", [(1, 1040, 8, 2, 2), (1, 16, 8, 1, 4097)])
def test_attn_pool_train_rejects_what_the_kernels_cannot_hold(B, C, heads, h, w, monkeypatch):
    """More than 1024 channels or 4096 tokens: ValueError before anything is launched."""
    monkeypatch.delenv("LAV_TRAIN_CONV", raising=False)
    m = _attention(C, heads, seed=1).to(DEV)
    x = torch.zeros((B, C, h, w), device=DEV, requires_grad=True)
    n0 = ops.train_work.get("attn_train_calls", 0)
    with pytest.raises(ValueError, match="unsupported"):
        hipnn.attn_pool_train(m, x)
    assert ops.train_work.get("attn_train_calls", 0) == n0
