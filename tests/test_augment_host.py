"""Image augmentation on the host (lav_amd/data/augment.py): Philox4x32-10 against Random123's known answers, the per-sample
draws (batch independence, ranks, stream tags, rates, ranges), the identity cases, and every op of the NumPy restatement
against an independent formulation (scipy's correlate1d, float64 tables, the float grayscale formula, sampling statistics);
train_seg.py --augment on the CPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from lav_amd.data import augment as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2021


def images(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- Philox
@pytest.mark.parametrize("counter, key, expect", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox4x32_known_answers(counter, key, expect):
    out = A.philox4x32(*[np.array([c, c]) for c in counter], key)
    assert " ".join(f"{int(o[0]):08x}" for o in out) == expect
    assert all(o[0] == o[1] and o.dtype == np.uint32 for o in out)
    # the 64-bit seed form: key word 0 is its low half
    out64 = A.philox4x32(*[np.array([c]) for c in counter], key[0] | key[1] << 32)
    assert " ".join(f"{int(o[0]):08x}" for o in out64) == expect


def test_uniforms_are_exact_24_bit_fractions():
    w = np.array([0, 255, 256, 0xffffffff], np.uint32)
    assert A._uniform(w).tolist() == [0.0, 0.0, 2.0 ** -24, 1 - 2.0 ** -24]
    assert A._uniform_open(w).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]


# ---------------------------------------------------------------------------------------------------------------- draws
def test_a_samples_draw_does_not_depend_on_its_batch():
    alone = [A.Augmenter(0.5, SEED).draw(0)] + [A.draw_sample(0.5, SEED, n) for n in range(40)]
    one = A.Augmenter(0.5, SEED).draw(40)
    a = A.Augmenter(0.5, SEED)
    pieces = np.concatenate([a.draw(k) for k in (1, 7, 0, 13, 19)])
    assert one.tobytes() == np.concatenate(alone).tobytes() == pieces.tobytes()
    assert one["sample"].tolist() == list(range(40))


def test_draws_differ_across_ranks_stream_tags_and_seeds():
    base = A.Augmenter(0.5, SEED, rank=0, world=2).draw(16)
    rank1 = A.Augmenter(0.5, SEED, rank=1, world=2).draw(16)
    assert base["sample"].tolist() == list(range(0, 32, 2)) and rank1["sample"].tolist() == list(range(1, 32, 2))
    both = A.Augmenter(0.5, SEED).draw(32)      # the two ranks together draw the single process's samples
    assert both[0::2].tobytes() == base.tobytes() and both[1::2].tobytes() == rank1.tobytes()
    tag1 = A.Augmenter(0.5, SEED, rank=0, world=2, stream_tag=1).draw(16)
    other = A.Augmenter(0.5, SEED + 1, rank=0, world=2).draw(16)
    for p in (rank1, tag1, other):
        assert not np.array_equal(p["order"], base["order"]) and not np.array_equal(p["elastic_alpha"], base["elastic_alpha"])
    assert (tag1["tag"] == 1 << 16).all() and (base["tag"] == 0).all()


def test_draw_rates_and_ranges():
    n, prob = 2000, 0.5
    p = A.Augmenter(prob, SEED).draw(n)
    assert (np.sort(p["order"], axis=1) == np.arange(7)).all()
    sd = np.sqrt(prob * (1 - prob) / n)
    for op in range(7):
        share = np.mean(p["active"] >> op & 1)
        assert abs(share - prob) <= 5 * sd, (A.OP_NAMES[op], share)
        first = np.mean(p["order"][:, 0] == op)           # the order is a uniform permutation
        assert abs(first - 1 / 7) <= 5 * np.sqrt(6 / 49 / n), (A.OP_NAMES[op], first)
    for op in (A.NOISE, A.DROPOUT, A.MULTIPLY, A.CONTRAST):
        assert abs(np.mean(p["per_channel"] >> op & 1) - 0.5) <= 5 * np.sqrt(0.25 / n)
    for name, (lo, hi) in A.RANGES.items():
        v = p[name]
        assert (v >= np.float32(lo)).all() and (v <= np.float32(hi)).all(), name
        assert v.max() - v.min() > 0.8 * (hi - lo), name
    for name, op in (("multiply", A.MULTIPLY), ("contrast", A.CONTRAST)):
        pc = (p["per_channel"] >> op & 1).astype(bool)
        assert (p[name][~pc] == p[name][~pc][:, :1]).all() and (p[name][pc][:, 0] != p[name][pc][:, 1]).all()
    assert np.allclose(p["blur_w"].sum(1), 1, atol=1e-6) and (p["field_w"] == A.gaussian_taps(0.25)).all()
    # a blur below sigma 1e-3 is never active
    assert not (p["active"][p["blur_sigma"] < 1e-3] & 1).any()
    assert not A.Augmenter(0.0, SEED).draw(200)["active"].any()


# ---------------------------------------------------------------------------------------------------------------- identity
def test_prob_zero_and_inactive_records_return_the_input_bytes():
    img = images((3, 20, 31, 3))
    t = torch.from_numpy(img)
    assert torch.equal(A.Augmenter(0.0, SEED)(t), t)
    assert np.array_equal(A.augment_numpy(img, A.make_params(3), SEED), img)


def test_elastic_with_alpha_zero_is_the_identity():
    """The cubic weights at fraction 0 are exactly [0, 1, 0, 0]."""
    assert [float(w) for w in A._cubic(np.float32(0))] == [0.0, 1.0, 0.0, 0.0]
    img = images((2, 37, 53, 3))
    assert np.array_equal(A.augment_numpy(img, A.make_params(2, active=["elastic"], elastic_alpha=0.0), SEED), img)
    moved = A.augment_numpy(img, A.make_params(2, active=["elastic"], elastic_alpha=3.5), SEED)
    assert np.mean(moved != img) > 0.5


def test_cubic_weights_are_keys_kernel_at_minus_three_quarters():
    """W(s) = (a+2)|s|^3 - (a+3)|s|^2 + 1 for |s| <= 1, a|s|^3 - 5a|s|^2 + 8a|s| - 4a for 1 < |s| < 2 (Keys 1981), a = -0.75, in float64."""
    t = np.linspace(0, 1, 257, dtype=np.float32)[:-1]
    w = np.stack(A._cubic(t)).astype(np.float64)
    a, t = -0.75, t.astype(np.float64)
    near = lambda s: (a + 2) * s ** 3 - (a + 3) * s ** 2 + 1
    far = lambda s: a * s ** 3 - 5 * a * s ** 2 + 8 * a * s - 4 * a
    assert np.allclose(w, np.stack([far(t + 1), near(t), near(1 - t), far(2 - t)]), atol=1e-6)
    assert np.allclose(w.sum(0), 1, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- the ops
@pytest.mark.parametrize("sigma", [0.2, 0.35, 0.5])
def test_blur_against_scipy(sigma):
    from scipy.ndimage import correlate1d
    img = images((1, 41, 58, 3), seed=3)
    got = A.augment_numpy(img, A.make_params(1, active=["blur"], blur_sigma=sigma), SEED)[0]
    k = np.exp(-np.arange(-2, 3) ** 2 / (2 * sigma ** 2))
    k /= k.sum()
    ref = correlate1d(correlate1d(img[0].astype(np.float64), k, axis=1, mode="mirror"), k, axis=0, mode="mirror")
    assert np.abs(got.astype(np.float64) - ref).max() <= 1.0 - 0.49     # |rounded - exact| <= 0.5 (+ float32's error)
    assert np.abs(got.astype(int) - np.clip(np.rint(ref), 0, 255).astype(int)).max() <= 1
    assert sigma < 0.3 or np.mean(got != img[0]) > 0.3     # (at sigma 0.2 the outer taps weigh 4e-6)


@pytest.mark.parametrize("alpha", [0.0, 0.3, 0.5])
def test_grayscale_against_the_float_formula(alpha):
    img = images((1, 33, 47, 3), seed=4)
    got = A.augment_numpy(img, A.make_params(1, active=["grayscale"], gray_alpha=alpha), SEED)[0].astype(np.float64)
    v = img[0].astype(np.float64)
    g = (0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2])[..., None]
    assert np.abs(got - (v + alpha * (g - v))).max() <= 1.0
    if alpha == 0.0:
        assert np.array_equal(got, v)


@pytest.mark.parametrize("op, value", [("multiply", 1 / 1.2), ("multiply", 1.2), ("multiply", (0.9, 1.0, 1.15)),
                                       ("contrast", 1 / 1.2), ("contrast", 1.2), ("contrast", (0.85, 1.0, 1.1))])
def test_multiply_and_contrast_against_a_float64_table(op, value):
    img = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :, None], (1, 2, 256, 3)).copy()
    p = A.make_params(1, active=[op], **{op: value})
    got = A.augment_numpy(img, p, SEED)[0, 0]
    for c in range(3):
        m = float(p[op][0, c])        # the float32 parameter the op sees
        v = np.arange(256, dtype=np.float64)
        exact = v * m if op == "multiply" else 128 + m * (v - 128)
        assert np.array_equal(got[:, c], np.clip(np.rint(exact), 0, 255).astype(np.uint8)), (op, c)


@pytest.mark.parametrize("p_drop", [0.01, 0.1])
def test_dropout_share_and_channel_masks(p_drop):
    img = np.full((1, 200, 300, 3), 200, np.uint8)
    n = 200 * 300
    same = A.augment_numpy(img, A.make_params(1, active=["dropout"], dropout_p=p_drop), SEED)[0]
    per = A.augment_numpy(img, A.make_params(1, active=["dropout"], dropout_p=p_drop, per_channel=["dropout"]), SEED)[0]
    assert set(np.unique(same)) <= {0, 200} and set(np.unique(per)) <= {0, 200}
    assert (same[..., 0] == same[..., 1]).all() and (same[..., 0] == same[..., 2]).all()
    assert abs(np.mean(same[..., 0] == 0) - p_drop) <= 5 * np.sqrt(p_drop * (1 - p_drop) / n)
    assert abs(np.mean(per == 0) - p_drop) <= 5 * np.sqrt(p_drop * (1 - p_drop) / (3 * n))
    for a, b in ((0, 1), (0, 2), (1, 2)):     # independent masks: they coincide on p^2 of the pixels, not on p
        assert abs(np.mean((per[..., a] == 0) & (per[..., b] == 0)) - p_drop ** 2) <= 5 * np.sqrt(p_drop ** 2 / n)
    assert np.array_equal(per[..., 0], same[..., 0])       # channel 0 uses the same word in both modes


@pytest.mark.parametrize("scale", [2.0, 12.75])
def test_noise_moments_and_channels(scale):
    img = np.full((1, 200, 300, 3), 128, np.uint8)
    n = 200 * 300
    same = A.augment_numpy(img, A.make_params(1, active=["noise"], noise_scale=scale), SEED)[0].astype(np.float64) - 128
    per = A.augment_numpy(img, A.make_params(1, active=["noise"], noise_scale=scale, per_channel=["noise"]), SEED)[0].astype(np.float64) - 128
    assert (same[..., 0] == same[..., 1]).all() and (same[..., 0] == same[..., 2]).all()
    var = scale ** 2 + 1 / 12                         # rounding to integers adds a uniform's variance
    for d, count in ((same[..., 0], n), (per[..., 0], n), (per[..., 1], n), (per[..., 2], n)):
        assert abs(d.mean()) <= 5 * np.sqrt(var / count)
        assert abs(d.var() - var) <= 5 * var * np.sqrt(2 / count)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert abs(np.corrcoef(per[..., a].ravel(), per[..., b].ravel())[0, 1]) <= 5 / np.sqrt(n)
    assert np.array_equal(per[..., 0], same[..., 0])


def test_random_words_depend_on_sample_tag_and_seed():
    img = np.full((1, 40, 40, 3), 128, np.uint8)
    kw = dict(active=["noise", "dropout", "elastic"], per_channel=["noise"])
    base = A.augment_numpy(img, A.make_params(1, **kw), SEED)
    assert np.array_equal(base, A.augment_numpy(img, A.make_params(1, **kw), SEED))
    for other in (A.augment_numpy(img, A.make_params(1, sample0=1, **kw), SEED), A.augment_numpy(img, A.make_params(1, stream_tag=1, **kw), SEED),
                  A.augment_numpy(img, A.make_params(1, **kw), SEED + 1)):
        assert np.mean(other != base) > 0.5


def test_full_chain_differs_by_order_and_bad_tables_are_refused():
    img = images((1, 30, 30, 3), seed=5)
    fwd = A.augment_numpy(img, A.make_params(1, active=range(7), multiply=1.2, contrast=0.85), SEED)
    rev = A.augment_numpy(img, A.make_params(1, order=range(6, -1, -1), active=range(7), multiply=1.2, contrast=0.85), SEED)
    assert not np.array_equal(fwd, rev)
    with pytest.raises(ValueError, match="permutation"):
        A.make_params(1, order=[0, 0, 1, 2, 3, 4, 5])
    bad = A.make_params(1)
    bad["order"][0, 1] = 0
    with pytest.raises(ValueError, match="permutation"):
        A.augment_numpy(img, bad, SEED)
    with pytest.raises(ValueError, match="records"):
        A.augment_numpy(img, A.make_params(2), SEED)


def test_ops_augment_u8_refuses_cpu_tensors():
    from lav_amd import ops
    with pytest.raises(RuntimeError, match="HBM"):
        ops.augment_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), A.make_params(1), SEED)


# ---------------------------------------------------------------------------------------------------------------- trainer
def _train_seg_cpu(tmp_path, name, *extra):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(REPO, "train_seg.py"), "--synthetic", "--device", "cpu", "--num-epoch", "1",
                        "--batch-size", "2", "--steps-per-epoch", "2", "--num-per-log", "1", "--save-dir", str(out), "--config-path", "", *extra],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = re.findall(r"^\d+ \{'loss': [^}]*\}$", r.stdout, flags=re.M)
    assert len(losses) == 2, r.stdout
    return out, losses


def test_train_seg_cpu_with_augment(tmp_path):
    import lav_amd
    out, aug = _train_seg_cpu(tmp_path, "aug", "--augment", "0.5")
    assert all(np.isfinite(float(re.search(r"'loss': ([-\w.+]+)", l).group(1))) for l in aug)
    lav_amd.RGBSegmentationModel([4, 6, 7, 10]).load_state_dict(torch.load(out / "seg_1.th", map_location="cpu"), strict=True)
    _, plain = _train_seg_cpu(tmp_path, "plain")
    _, zero = _train_seg_cpu(tmp_path, "zero", "--augment", "0")
    assert plain == zero
    assert plain != aug          # the augmented run trains on other pixels
