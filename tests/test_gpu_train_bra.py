"""The brake net's training path on the GPU: lav_attn_train_* (the attention pooling in train mode) against float64 autograd of
lav_amd.rgb.Attention, lav_seg_xent_up_forward against float64 F.cross_entropy(F.interpolate(.)), BrakeTrainer.train_bra against
the reference trainer's fixture (tests/golden/bra_train.npz), reproducibility, and the train_bra_v2.py command line feeding the
agent."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from lav_amd import ops
from lav_amd.train import hipnn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")


def _attention(C, seed):
    from lav_amd.rgb import Attention
    torch.manual_seed(seed)
    m = Attention(C, num_heads=8)
    with torch.no_grad():                    # (a trained-looking scale: dots of a few units, not a one-hot soft-max)
        m.q.mul_(0.5)
        m.linear_kv.bias.normal_(0, 0.1)
    return m.train()


def _close(got, ref, name, rel=1e-4):
    ref = ref.double().cpu()
    err = (got.double().cpu() - ref).abs().max().item()
    assert err <= rel * ref.abs().max().item() + 1e-30, f"{name}: max error {err:.3g} vs max |ref| {ref.abs().max().item():.3g}"


@pytest.mark.parametrize("B,C,h,w", [(3, 512, 9, 24), (3, 512, 6, 15), (2, 512, 7, 13), (1, 256, 40, 40)])
def test_attn_pool_train_matches_float64_autograd(B, C, h, w, monkeypatch):
    monkeypatch.delenv("LAV_TRAIN_CONV", raising=False)
    m = _attention(C, seed=B * 1000 + h)
    g = torch.Generator().manual_seed(h * w)
    x = torch.relu(torch.randn(B, C, h, w, generator=g)) * 2
    dout = torch.randn(B, C, generator=g)
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


@pytest.mark.parametrize("K", [4, 5])
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_seg_cross_entropy_up_matches_float64(K, s, dtype, monkeypatch):
    monkeypatch.delenv("LAV_TRAIN_CONV", raising=False)
    g = torch.Generator().manual_seed(K * 10 + s)
    B, h, w = 3, 7, 13
    logits = torch.randn(B, K, h, w, generator=g) * 3
    labels = torch.randint(0, K, (B, h * s, w * s), generator=g).to(dtype)
    l64 = logits.double().requires_grad_(True)
    ref = F.cross_entropy(F.interpolate(l64, scale_factor=s), labels.long())
    ref.backward()
    lg = logits.to(DEV).requires_grad_(True)
    n0 = ops.train_work.get("seg_xent_up_calls", 0)
    loss = hipnn.seg_cross_entropy_up(lg, labels.to(DEV), s)
    assert ops.train_work["seg_xent_up_calls"] == n0 + 1
    (loss * 2).backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    _close(lg.grad / 2, l64.grad, "dlogits", rel=1e-5)


def test_seg_cross_entropy_up_rejects_bad_labels_and_shapes():
    lg = torch.zeros(2, 4, 5, 6, device=DEV, requires_grad=True)
    bad = torch.zeros(2, 20, 24, dtype=torch.int64, device=DEV)
    bad[1, 3, 3] = 4
    with pytest.raises(ValueError, match="labels span"):
        hipnn.seg_cross_entropy_up(lg, bad, 4)
    with pytest.raises(ValueError, match="labels span"):
        hipnn.seg_cross_entropy_up(lg, torch.full((2, 20, 24), 9, dtype=torch.uint8, device=DEV), 4)
    with pytest.raises(ValueError, match="not 4 x the logits"):
        hipnn.seg_cross_entropy_up(lg, torch.zeros(2, 20, 25, dtype=torch.uint8, device=DEV), 4)
    with pytest.raises(ValueError, match="not 2 x the logits"):
        hipnn.seg_cross_entropy_up(lg, torch.zeros(2, 20, 24, dtype=torch.uint8, device=DEV), 2)


def _fixture_run(monkeypatch, mode):
    """BrakeTrainer for the fixture's three steps on the GPU; mode: a LAV_TRAIN_CONV value, or None for the defaults."""
    from lav_amd.train import BrakeTrainer, TrainConfig, synthetic_bra_batch
    if mode is None:
        monkeypatch.delenv("LAV_TRAIN_CONV", raising=False)
    else:
        monkeypatch.setenv("LAV_TRAIN_CONV", mode)
    monkeypatch.delenv("LAV_TRAIN_BRA", raising=False)
    tr = BrakeTrainer(TrainConfig(), DEV)
    losses, preds, calls = [], [], []
    for step in range(3):
        a0, x0 = ops.train_work.get("attn_train_calls", 0), ops.train_work.get("seg_xent_up_calls", 0)
        info = tr.train_bra(*synthetic_bra_batch(2, seed=400 + step, hw=(64, 192), tel_hw=(64, 96), num_classes=4))
        calls.append((ops.train_work.get("attn_train_calls", 0) - a0, ops.train_work.get("seg_xent_up_calls", 0) - x0))
        losses.append(info["loss"])
        preds.append(info["pred_bra"])
    return tr, np.array(losses), np.array(preds), calls


@pytest.mark.parametrize("mode", ["hip", None])
def test_train_bra_on_gpu_matches_reference_trainer(mode, monkeypatch):
    g = dict(np.load(os.path.join(GOLD, "bra_train.npz")))
    tr, losses, preds, calls = _fixture_run(monkeypatch, mode)
    if mode == "hip":
        assert calls == [(2, 2)] * 3, calls          # both attention poolings and both seg losses on the kernels, every step
    else:
        want = (2 if hipnn.brake_piece_on("attn") else 0, 2 if hipnn.brake_piece_on("xent") else 0)
        assert calls == [want] * 3, calls
    np.testing.assert_allclose(losses[0], g["losses"][0], rtol=1e-3)
    np.testing.assert_allclose(losses[1:], g["losses"][1:], rtol=3e-2)
    np.testing.assert_allclose(np.log(preds[0]), np.log(g["pred_bra"][0]), rtol=1e-3)
    sd = tr.state_dict("bra")
    names = [str(n) for n in g["names"]]
    assert names == list(sd)
    abs_sums = np.array([sd[k].double().abs().sum().item() for k in names])
    np.testing.assert_allclose(abs_sums, g["abs_sums"], rtol=3e-2, atol=1e-3)


def test_train_bra_all_torch_step_uses_no_brake_kernels(monkeypatch):
    _, losses, _, calls = _fixture_run(monkeypatch, "torch")
    assert calls == [(0, 0)] * 3
    g = dict(np.load(os.path.join(GOLD, "bra_train.npz")))
    np.testing.assert_allclose(losses[0], g["losses"][0], rtol=1e-3)


def test_train_bra_deterministic_runs_are_bit_identical(monkeypatch):
    from lav_amd.train.run import set_deterministic
    set_deterministic(True)
    try:
        a, la, _, _ = _fixture_run(monkeypatch, None)
        b, lb, _, _ = _fixture_run(monkeypatch, None)
    finally:
        set_deterministic(False)
    assert np.array_equal(la, lb)
    for (k, p), q in zip(a.bra_model.named_parameters(), b.bra_model.parameters()):
        assert torch.equal(p, q), k


def test_train_bra_cli_on_gpu_feeds_the_agent(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(REPO, "train_bra_v2.py"), "--synthetic", "--num-epoch", "1", "--batch-size", "8",
                        "--steps-per-epoch", "2", "--save-dir", str(tmp_path / "ck"), "--config-path", ""],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert '"what": "bra"' in r.stdout and '"steps": 2' in r.stdout
    path = tmp_path / "ck" / "bra_1.th"
    sd = torch.load(path, map_location="cpu")
    assert sd["seg_head.upconv.9.weight"].shape[0] == 4 and all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    from lav_amd.lav_agent import LAVAgent
    cfg = tmp_path / "agent.yaml"
    cfg.write_text(yaml.safe_dump(dict(synthetic_weights=True, points_per_tick=8192, precapture=False, hip_graphs=False,
                                       bra_model_dir=str(path))))
    agent = LAVAgent(str(cfg))
    assert agent.bra_model.seg_head.upconv[9].out_channels == 4
    assert torch.equal(agent.bra_model.attn1.q.detach().cpu(), sd["attn1.q"])
