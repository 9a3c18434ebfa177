"""lav_augment_u8 (csrc/augment.hip) on the GPU against the NumPy restatement lav_amd.data.augment.augment_numpy: every op alone at
both ends of its range, full chains of all seven ops in fixed and drawn orders over tile seams and image edges, batch independence,
determinism, and the trainers' --augment.

The rule of every comparison: bit-identical where noise is inactive.  Where noise is active - two float32 evaluations of Box-Muller
(the device's logf / cosf, NumPy's) can land on opposite sides of a .5 boundary - no pixel-channel may differ by more than one grey
level and at most 1e-4 of them may differ at all.  That cap is a condition, not a measurement: float32 against float64, and float32
against a 4-ulp perturbation, differ on 3e-6 to 9e-6 of the pixel-channels over scales 0.5 to 12.75 (1.8 M samples, NumPy); the cap
leaves an order of magnitude over that.  Every comparison prints its share.  (In a chain a flipped noise value can be spread by a
later blur or warp and scaled by multiply / contrast: the same cap is kept there and the measured share is printed.)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lav_amd import ops
from lav_amd.data import augment as A

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2021
SIZES = [(288, 256), (288, 768), (192, 480), (37, 53), (1, 1)]      # train_seg's, train_bra's wide and telephoto, odd, degenerate
NOISE_SHARE = 1e-4


def images(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def run_gpu(img, params, seed=SEED):
    return ops.augment_u8(torch.from_numpy(img).cuda(), params, seed).cpu().numpy()


def compare(got, ref, noise, what):
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    share = float(np.mean(diff != 0))
    print(f"{what}: {diff.size} pixel-channels, differing share {share:.3g}, max |difference| {int(diff.max()) if diff.size else 0}")
    if not noise:
        assert np.array_equal(got, ref), f"{what}: {int((diff != 0).sum())} of {diff.size} pixel-channels differ (max {int(diff.max())})"
    else:
        assert diff.max() <= 1, f"{what}: a pixel-channel differs by {int(diff.max())} grey levels"
        assert share <= NOISE_SHARE, f"{what}: {share:.3g} of the pixel-channels differ (cap {NOISE_SHARE})"


SINGLE = [
    ("blur", dict(blur_sigma=1e-3)), ("blur", dict(blur_sigma=0.5)),
    ("noise", dict(noise_scale=0.0)), ("noise", dict(noise_scale=12.75)),
    ("noise", dict(noise_scale=0.5, per_channel=["noise"])), ("noise", dict(noise_scale=12.75, per_channel=["noise"])),
    ("dropout", dict(dropout_p=0.01)), ("dropout", dict(dropout_p=0.1)),
    ("dropout", dict(dropout_p=0.01, per_channel=["dropout"])), ("dropout", dict(dropout_p=0.1, per_channel=["dropout"])),
    ("multiply", dict(multiply=1 / 1.2)), ("multiply", dict(multiply=1.2)), ("multiply", dict(multiply=(1 / 1.2, 1.0, 1.2))),
    ("contrast", dict(contrast=1 / 1.2)), ("contrast", dict(contrast=1.2)), ("contrast", dict(contrast=(1.2, 1.0, 1 / 1.2))),
    ("grayscale", dict(gray_alpha=0.0)), ("grayscale", dict(gray_alpha=0.5)),
    ("elastic", dict(elastic_alpha=0.5)), ("elastic", dict(elastic_alpha=3.5)),
]


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_each_op_alone_matches_the_restatement(hw):
    img = images((2, *hw, 3), seed=hw[0] * 1000 + hw[1])
    for op, kw in SINGLE:
        p = A.make_params(2, active=[op], sample0=5, **kw)
        compare(run_gpu(img, p), A.augment_numpy(img, p, SEED), op == "noise", f"{op} {kw} {hw}")


def test_identity_cases_on_the_gpu():
    img = images((3, 45, 70, 3), seed=9)
    assert np.array_equal(run_gpu(img, A.make_params(3)), img)
    assert np.array_equal(run_gpu(img, A.make_params(3, active=["elastic"], elastic_alpha=0.0)), img)
    t = torch.from_numpy(img).cuda()
    assert A.Augmenter(0.0, SEED)(t) is t
    with pytest.raises(RuntimeError, match="overlap"):
        from lav_amd import _lib
        _lib.check(_lib.load().lav_augment_u8(t.data_ptr(), t.data_ptr(), 3, 45, 70, t.data_ptr(), SEED, 0), "lav_augment_u8")


def chain_orders():
    """blur -> ... -> elastic, elastic -> ... -> blur, blur and elastic adjacent in both orders (at the start, in the middle, at the
    end), and 64 drawn orders."""
    B, N, D, M, C, G, E = range(7)
    fixed = [[B, N, D, M, C, G, E], [E, N, D, M, C, G, B], [B, E, N, D, M, C, G], [E, B, N, D, M, C, G], [N, D, B, E, M, C, G],
             [N, D, E, B, M, C, G], [N, D, M, C, G, B, E], [N, D, M, C, G, E, B]]
    rng = np.random.default_rng(7)
    return fixed + [rng.permutation(7).tolist() for _ in range(64)]


def chain_params(orders, rng, noise=True):
    """One record per order, all seven ops active (noise optional), scalars drawn over the specified ranges, ends included."""
    recs = []
    for k, order in enumerate(orders):
        u = lambda name: [A.RANGES[name][0], A.RANGES[name][1], rng.uniform(*A.RANGES[name])][k % 3 if k % 5 else 2]
        active = [o for o in range(7) if noise or o != A.NOISE]
        recs.append(A.make_params(1, order=order, active=active, sample0=1000 + k, stream_tag=k % 2,
                                  per_channel=[o for o in (A.NOISE, A.DROPOUT) if rng.random() < 0.5],
                                  blur_sigma=max(u("blur_sigma"), 0.05), noise_scale=u("noise_scale"), dropout_p=u("dropout_p"),
                                  multiply=[u("multiply") for _ in range(3)], contrast=[u("contrast") for _ in range(3)],
                                  gray_alpha=u("gray_alpha"), elastic_alpha=u("elastic_alpha")))
    return np.concatenate(recs)


@pytest.mark.parametrize("noise", [False, True], ids=["without_noise", "with_noise"])
@pytest.mark.parametrize("hw", [(75, 150), (97, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_full_chains_in_fixed_and_drawn_orders(hw, noise):
    """Batches of 32, all seven ops (six without noise: exact).  75 x 150 and 97 x 131 are no multiples of the 64 x 32 tile: three
    columns and three or four rows of tiles, so every seam, a partial last tile and all four image edges are compared."""
    orders = chain_orders()
    assert len(orders) == 72
    params = chain_params(orders, np.random.default_rng(11), noise)
    for lo in range(0, len(orders), 32):        # 8 fixed + 64 drawn orders: two batches of 32 and one of 8
        p = params[lo:lo + 32]
        img = images((len(p), *hw, 3), seed=lo + hw[1])
        compare(run_gpu(img, p), A.augment_numpy(img, p, SEED), noise, f"chains {lo}..{lo + len(p) - 1} {hw} noise={noise}")


def test_an_images_result_does_not_depend_on_its_batch():
    orders = chain_orders()[:32]
    params = chain_params(orders, np.random.default_rng(13))
    img = images((32, 75, 150, 3), seed=21)
    batch = run_gpu(img, params)
    for k in (0, 1, 17, 31):
        assert np.array_equal(run_gpu(img[k:k + 1], params[k:k + 1])[0], batch[k]), k
    assert np.array_equal(run_gpu(img[::-1].copy(), params[::-1].copy())[::-1], batch)


def test_drawn_batch_matches_the_restatement_and_is_deterministic():
    """Augmenter on cuda: the same seed gives the same bytes, another seed other bytes; and the CPU path computes the same images."""
    img = images((32, 96, 160, 3), seed=5)
    t = torch.from_numpy(img).cuda()
    a, b, c = A.Augmenter(0.5, SEED)(t), A.Augmenter(0.5, SEED)(t), A.Augmenter(0.5, SEED + 1)(t)
    assert a.dtype == torch.uint8 and a.shape == t.shape and a.is_cuda
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, t)
    cpu = A.Augmenter(0.5, SEED)(torch.from_numpy(img))
    params = A.Augmenter(0.5, SEED).draw(32)
    compare(a.cpu().numpy(), cpu.numpy(), bool((params["active"] >> A.NOISE & 1).any()), "Augmenter cuda against cpu")
    quiet = ~(params["active"] >> A.NOISE & 1).astype(bool)
    assert quiet.any() and np.array_equal(a.cpu().numpy()[quiet], cpu.numpy()[quiet])
    second = A.Augmenter(0.5, SEED)
    second.draw(32)
    assert not torch.equal(second(t), a)         # the next 32 sample ids


def _run(script, tmp_path, *args):
    r = subprocess.run([sys.executable, os.path.join(REPO, script), "--synthetic", "--num-epoch", "2", "--steps-per-epoch", "2",
                        "--num-per-log", "1", "--save-dir", str(tmp_path / "ck"), "--config-path", "", "--augment", "0.5", *args],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_train_seg_cli_with_augment(tmp_path):
    import re
    import lav_amd
    out = _run("train_seg.py", tmp_path, "--batch-size", "8")
    losses = [float(v) for v in re.findall(r"'loss': ([-\w.+]+)", out)]
    assert len(losses) == 4 and np.isfinite(losses).all(), out
    assert '"what": "seg"' in out and '"steps": 4' in out
    for e in (1, 2):
        sd = torch.load(tmp_path / "ck" / f"seg_{e}.th", map_location="cpu")
        lav_amd.RGBSegmentationModel([4, 6, 7, 10]).load_state_dict(sd, strict=True)
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())


def test_train_bra_cli_with_augment(tmp_path):
    import re
    from lav_amd.rgb import RGBBrakePredictionModel
    out = _run("train_bra_v2.py", tmp_path, "--batch-size", "8")
    losses = [float(v) for v in re.findall(r"'loss': ([-\w.+]+)", out)]
    assert len(losses) == 4 and np.isfinite(losses).all(), out
    assert '"what": "bra"' in out and '"steps": 4' in out
    for e in (1, 2):
        sd = torch.load(tmp_path / "ck" / f"bra_{e}.th", map_location="cpu")
        RGBBrakePredictionModel([4, 10, 18]).load_state_dict(sd, strict=True)
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
