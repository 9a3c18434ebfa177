"""The segmenter's training path on the GPU: lav_pair_train_* (ERFNet's factorised pairs in train mode) and lav_seg_xent_forward
against float64, one non_bottleneck_1d on the training kernels against the torch module, and LAV(what="seg").train_seg against
the reference trainer's fixture (tests/golden/seg_train.npz)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lav_amd import _lib
from lav_amd.ops import _ptr, _stream, check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 128), (64, 64), (128, 32)]


@pytest.fixture(autouse=True)
def _seg_kernels(monkeypatch):
    """The segmenter's training kernels are opt-in (LAV_TRAIN_CONV=hip, hipnn._seg_kernels_on): on for every test here."""
    monkeypatch.setenv("LAV_TRAIN_CONV", "hip")


def _operand(shape, g, decades):
    """Normal values times 10^U(-decades/2, decades/2) per element."""
    v = torch.randn(shape, generator=g, dtype=torch.float64)
    return v * torch.pow(10.0, (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5) * decades)


def _pair_run(x, wa, ba, wb, bb, d, dz):
    lib = _lib.load()
    B, C, H, W = x.shape
    t, z, dt, dx = (torch.empty_like(x) for _ in range(4))
    dwa, dwb = torch.empty_like(wa), torch.empty_like(wb)
    dba, dbb = torch.empty_like(ba), torch.empty_like(bb)
    ws = torch.zeros(lib.lav_pair_train_workspace_bytes(B, C, H), dtype=torch.uint8, device=DEV)
    check(lib.lav_pair_train_forward(_ptr(x), _ptr(wa), _ptr(ba), _ptr(wb), _ptr(bb), B, C, H, W, d, _ptr(t), _ptr(z), _stream()), "fwd")
    check(lib.lav_pair_train_backward(_ptr(x), _ptr(t), _ptr(dz), _ptr(wa), _ptr(wb), B, C, H, W, d, _ptr(dt), _ptr(dx), _ptr(dwa), _ptr(dba),
                                      _ptr(dwb), _ptr(dbb), _ptr(ws), ws.numel(), _stream()), "bwd")
    torch.cuda.synchronize()
    return dict(t=t, z=z, dt=dt, dx=dx, dwa=dwa, dba=dba, dwb=dwb, dbb=dbb)


def _within(name, got, want, bound, rel=2e-6):
    err = (got.detach().cpu().double() - want).abs()
    lim = rel * bound + 1e-30
    worst = (err / lim).max().item()
    assert worst <= 1.0, f"{name}: error {worst:.3g} x the bar (2e-6 of sum |a||b|)"


@pytest.mark.parametrize("C,W", SHAPES)
@pytest.mark.parametrize("d", [1, 2, 4, 8, 16])
def test_pair_train_kernels_vs_float64(C, W, d):
    """Pair forward (t, z), dt, dx, dWa, dWb, dba, dbb at ERFNet's three stage shapes, every dilation, a ragged batch (3) and row
    count (7 / 5), operands spanning four decades: every element within 2e-6 of sum |a||b| of its float64 value (each stage from
    the kernel's own input to it); a second launch is bit-identical."""
    _check_pair(C, W, d, 3, 7 if d < 8 else 5)


@pytest.mark.parametrize("C,W,d", [(128, 32, 2), (16, 128, 1)])
def test_pair_train_kernels_many_rows_vs_float64(C, W, d):
    """B * H = 185 rows: more rows than the weight gradients' 128 partial slots, so every slot sums two rows and the last ones none."""
    _check_pair(C, W, d, 5, 37)


def _check_pair(C, W, d, B, H):
    g = torch.Generator().manual_seed(C + d)
    x64 = _operand((B, C, H, W), g, 4)
    wa64, wb64 = _operand((C, C, 3, 1), g, 4) / C, _operand((C, C, 1, 3), g, 4) / C
    ba64, bb64 = _operand((C,), g, 2), _operand((C,), g, 2)
    dz64 = _operand((B, C, H, W), g, 4)
    f = lambda a: a.float().to(DEV).contiguous()
    x, wa, ba, wb, bb, dz = map(f, (x64, wa64, ba64, wb64, bb64, dz64))
    out = _pair_run(x, wa, ba, wb, bb, d, dz)
    again = _pair_run(x, wa, ba, wb, bb, d, dz)
    for k in out:
        assert torch.equal(out[k], again[k]), f"{k}: two launches differ"
    xd, wad, bad, wbd, bbd, dzd = (a.cpu().double() for a in (x, wa, ba, wb, bb, dz))
    conv_a = lambda v, w: F.conv2d(v, w, None, 1, (d, 0), (d, 1))
    conv_b = lambda v, w: F.conv2d(v, w, None, 1, (0, d), (1, d))
    pre = conv_a(xd, wad) + bad[None, :, None, None]
    _within("t", out["t"], pre.clamp_min(0), conv_a(xd.abs(), wad.abs()) + bad.abs()[None, :, None, None])
    t = out["t"].cpu().double()
    _within("z", out["z"], conv_b(t, wbd) + bbd[None, :, None, None], conv_b(t.abs(), wbd.abs()) + bbd.abs()[None, :, None, None])
    convT_b = lambda v, w: F.conv_transpose2d(v, w, None, 1, (0, d), 0, 1, (1, d))
    convT_a = lambda v, w: F.conv_transpose2d(v, w, None, 1, (d, 0), 0, 1, (d, 1))
    mask = (t > 0).double()
    _within("dt", out["dt"], mask * convT_b(dzd, wbd), mask * convT_b(dzd.abs(), wbd.abs()))
    dt = out["dt"].cpu().double()
    _within("dx", out["dx"], convT_a(dt, wad), convT_a(dt.abs(), wad.abs()))
    wg_b = lambda a, s: torch.nn.grad.conv2d_weight(s, (C, C, 1, 3), a, 1, (0, d), (1, d))
    wg_a = lambda a, s: torch.nn.grad.conv2d_weight(s, (C, C, 3, 1), a, 1, (d, 0), (d, 1))
    _within("dwb", out["dwb"], wg_b(dzd, t), wg_b(dzd.abs(), t.abs()))
    _within("dwa", out["dwa"], wg_a(dt, xd), wg_a(dt.abs(), xd.abs()))
    _within("dbb", out["dbb"], dzd.sum((0, 2, 3)), dzd.abs().sum((0, 2, 3)))
    _within("dba", out["dba"], dt.sum((0, 2, 3)), dt.abs().sum((0, 2, 3)))


class _InjectedDropout(torch.nn.Module):
    def __init__(self, p, mask):
        super().__init__()
        self.p, self.mask = p, mask

    def forward(self, y):
        return y * self.mask[:, :, None, None]


@pytest.mark.parametrize("C,W,d,p", [(16, 128, 1, 0.0), (64, 64, 1, 0.03), (128, 32, 4, 0.3), (128, 32, 16, 0.3)])
def test_nb1d_block_train_vs_torch(C, W, d, p):
    """One non_bottleneck_1d in train mode on the training kernels (hipnn.nb1d_train: pairs on lav_pair_train_*, bn2 -> Dropout2d ->
    + x -> ReLU on lav_bn_train_*_mask) vs the torch module (forward_torch) with the same injected Dropout2d mask (p > 0: a drawn
    {0, 1/(1-p)} mask with zeros in it; p = 0: the fused residual path): output, input gradient, every parameter gradient and the
    running statistics within 1e-4 of the largest reference value (test_training_convolution_function_vs_torch's bar)."""
    from lav_amd.erfnet import non_bottleneck_1d
    from lav_amd.train import hipnn
    torch.manual_seed(C + d)
    blk = non_bottleneck_1d(C, p, d).to(DEV).train()
    ref = non_bottleneck_1d(C, p, d).to(DEV).train()
    ref.load_state_dict(blk.state_dict())
    x = torch.randn((3, C, 9, W), device=DEV)
    dy = torch.randn((3, C, 9, W), device=DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    mask = None
    if p > 0:
        mask = hipnn.dropout2d_mask(max(p, 0.25), 3, C, DEV)
        assert bool((mask == 0).any()) and bool((mask > 0).any())
        ref.dropout = _InjectedDropout(p, mask)
    assert hipnn._pair_train_ok(blk, xa)
    ya = hipnn.nb1d_train(blk, xa, mask=mask)
    if p > 0:
        assert type(ya.grad_fn).__name__.startswith("_BnMask"), "bn2 -> dropout -> + x -> ReLU must be the masked BatchNorm launch"
    ya.backward(dy)
    yb = ref.forward_torch(xb)
    yb.backward(dy)
    close = lambda a, b, what: ((a - b).abs().max().item() <= 1e-4 * b.abs().max().item() + 1e-7) or pytest.fail(what)
    close(ya.detach(), yb.detach(), "output")
    close(xa.grad, xb.grad, "input gradient")
    grads = {n: (pa.grad, pb.grad) for (n, pa), (_, pb) in zip(blk.named_parameters(), ref.named_parameters())}
    for n, (ga, gb) in grads.items():
        if n in ("conv1x3_1.bias", "conv1x3_2.bias"):
            # a bias right in front of a train-mode BatchNorm has gradient exactly 0 (the batch mean removes it): both sides hold
            # rounding noise of sum(dz) only, held to the scale of the same layer's weight gradient
            scale = grads[n.replace("bias", "weight")][1].abs().max().item()
            assert ga.abs().max().item() <= 1e-4 * scale and gb.abs().max().item() <= 1e-4 * scale, n
            continue
        close(ga, gb, n)
    for (n, ba), (_, bb) in zip(blk.named_buffers(), ref.named_buffers()):
        close(ba.double(), bb.double(), n)


@pytest.mark.parametrize("B,Cn,H,W", [(2, 5, 48, 256), (3, 8, 7, 13), (1, 1, 5, 5), (4, 3, 31, 17)])
def test_seg_xent_kernel_vs_float64(B, Cn, H, W):
    """lav_seg_xent_forward (through hipnn.seg_cross_entropy): loss and dlogits (scaled by the incoming gradient) vs
    F.cross_entropy in float64 at 1e-6 relative; two runs bit-identical."""
    from lav_amd.train import hipnn
    g = torch.Generator().manual_seed(B * Cn + H)
    logits = (torch.randn((B, Cn, H, W), generator=g) * 4).to(DEV)
    labels = torch.randint(0, Cn, (B, H, W), generator=g).to(DEV)
    outs = []
    for _ in range(2):
        lg = logits.clone().requires_grad_(True)
        loss = hipnn.seg_cross_entropy(lg, labels)
        assert type(loss.grad_fn).__name__.startswith("_SegXent")
        (loss * 3.0).backward()
        outs.append((loss.detach().clone(), lg.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    lr = logits.cpu().double().requires_grad_(True)
    ref = F.cross_entropy(lr, labels.cpu())
    (ref * 3.0).backward()
    np.testing.assert_allclose(outs[0][0].item(), ref.item(), rtol=1e-6)
    got = outs[0][1].cpu().double()
    assert (got - lr.grad).abs().max().item() <= 1e-6 * lr.grad.abs().max().item()


def test_seg_training_kernels_are_opt_in(monkeypatch):
    """Without LAV_TRAIN_CONV=hip the segmenter trains on torch (the kernels measured slower)."""
    from lav_amd.erfnet import non_bottleneck_1d
    from lav_amd.train import hipnn
    blk = non_bottleneck_1d(64, 0.0, 1).to(DEV).train()
    x = torch.randn((2, 64, 4, 64), device=DEV, requires_grad=True)
    assert hipnn._pair_train_ok(blk, x)
    monkeypatch.delenv("LAV_TRAIN_CONV")
    assert not hipnn._pair_train_ok(blk, x)
    lg = torch.randn((2, 5, 3, 3), device=DEV, requires_grad=True)
    assert type(hipnn.seg_cross_entropy(lg, torch.zeros((2, 3, 3), dtype=torch.int64, device=DEV)).grad_fn).__name__ != "_SegXentBackward"


def test_seg_xent_rejects_labels_out_of_range():
    from lav_amd.train import hipnn
    lg = torch.randn((2, 5, 3, 3), device=DEV, requires_grad=True)
    bad = torch.zeros((2, 3, 3), dtype=torch.int64, device=DEV)
    bad[1, 2, 2] = 5
    with pytest.raises(ValueError, match="labels"):
        hipnn.seg_cross_entropy(lg, bad)


def _seg_steps(seed=0):
    from lav_amd.train import TrainConfig
    from lav_amd.train.lav import LAV
    from lav_amd.train.synthetic import synthetic_seg_batch
    torch.manual_seed(seed)
    lav = LAV(TrainConfig(), DEV, what="seg")
    for m in lav.seg_model.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    losses = []
    for step in range(3):
        rgb, sem = synthetic_seg_batch(2, seed=300 + step, hw=(48, 256), num_classes=5)
        losses.append(lav.train_seg(rgb, sem)["loss"])
    return lav, losses


def test_train_seg_on_gpu_matches_reference_trainer(golden, monkeypatch):
    """LAV(what="seg").train_seg on the GPU (LAV_TRAIN_CONV=hip: pairs, BatchNorms and loss on the training kernels) vs the reference LAV.train_seg run
    on CPU (seeded weights, Dropout2d off, batch 2 of 48 x 256): step 0 at rtol 1e-3, later steps at 3e-2."""
    from lav_amd.train import hipnn
    g = golden["seg_train"]
    calls = {"pair": 0}
    real = hipnn.pair_train

    def counted(*a):
        calls["pair"] += 1
        return real(*a)
    monkeypatch.setattr(hipnn, "pair_train", counted)
    _, losses = _seg_steps()
    assert calls["pair"] == 3 * 2 * 17, "every pair of the 17 blocks must run on lav_pair_train_forward"
    for step in range(3):
        np.testing.assert_allclose(losses[step], g["losses"][step], rtol=1e-3 if step == 0 else 3e-2, err_msg=f"step {step}")


def test_train_seg_on_gpu_is_reproducible():
    """Two runs of three steps give bit-identical parameters (torch's own layers in deterministic mode: the downsamplers, upsamplers
    and the output layer are MIOpen's; liblav_amd's kernels reduce in a fixed order anyway)."""
    from lav_amd.train.run import set_deterministic
    prev = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark, torch.are_deterministic_algorithms_enabled(),
            getattr(getattr(torch.backends, "miopen", None), "immediate", None))
    set_deterministic(True)
    try:
        a, la = _seg_steps()
        b, lb = _seg_steps()
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = prev[0], prev[1]
        torch.use_deterministic_algorithms(prev[2])
        if prev[3] is not None:
            torch.backends.miopen.immediate = prev[3]
    assert la == lb
    for (n, pa), (_, pb) in zip(a.seg_model.state_dict().items(), b.seg_model.state_dict().items()):
        assert torch.equal(pa, pb), n


def test_train_seg_cli_on_gpu(tmp_path):
    """python train_seg.py --synthetic --num-epoch 1 --batch-size 8 (on the training kernels) writes seg_1.th, which loads into
    RGBSegmentationModel with strict keys."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "train_seg.py"), "--synthetic", "--num-epoch", "1", "--batch-size", "8",
                        "--save-dir", str(tmp_path)], cwd=str(tmp_path), capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, LAV_TRAIN_CONV="hip"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    import lav_amd
    m = lav_amd.RGBSegmentationModel([4, 6, 7, 10])
    m.load_state_dict(torch.load(tmp_path / "seg_1.th", map_location="cpu"), strict=True)
