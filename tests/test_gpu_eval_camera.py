"""lav_eval_seg and lav_eval_scores on the MI355X against their specifications (lav_amd.train.evaluate_camera.eval_seg_numpy /
eval_scores_numpy), every word compared exactly, the two evaluators with the accumulator in HBM and on the host, and the two command
lines end to end.  The specifications themselves are checked in tests/test_eval_camera_host.py."""
import json

import numpy as np
import pytest
import torch

from lav_amd import ops, synth
from lav_amd.train import evaluate_camera as C
from tests import eval_camera_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def seg_kernel(case, section=None):
    section = torch.zeros(68, dtype=torch.int64, device=DEV) if section is None else section
    return ops.eval_seg(section, dev(case["logits"]), dev(case["labels"]), case["scale"])


def seg_spec(case, section=None):
    section = np.zeros(68, np.int64) if section is None else section
    return C.eval_seg_numpy(section, case["logits"], case["labels"], case["scale"])


@pytest.mark.parametrize("name", list(U.SHAPES))
def test_seg_kernel_equals_specification(name):
    case = U.shape_case(name)
    n, k, h, w, scale = U.SHAPES[name]
    want = seg_spec(case)
    f = C.fields(want, "seg")
    if n * h * w >= 4 * k:             # the case does what it is there for: every class predicted, every label present, the planted pixels
        assert (f["conf"][:k, :k].sum(axis=0) > 0).all() and (f["conf"][:k, :k].sum(axis=1) > 0).all()
        assert int(f["nonfinite"]) == 5 * scale * scale and int(f["ignored"]) > 0
    assert int(f["pixels"]) == n * h * w * scale * scale == int(f["ignored"]) + int(f["nonfinite"]) + int(f["conf"].sum())
    np.testing.assert_array_equal(seg_kernel(case).cpu().numpy(), want)


@pytest.mark.parametrize("name", ["scale4_9x13", "eight_classes_16x12", "odd_37x53"])
def test_seg_kernel_on_tensors_that_start_off_every_boundary(name):
    """Labels that start on an odd byte (the byte loads, at every scale) and logits that start 4 bytes past a 16-byte boundary:
    views into larger buffers, contiguous and of the right shape, so they are accepted as they are."""
    case = U.shape_case(name)
    logits, labels = case["logits"], case["labels"]
    lbuf, fbuf = torch.zeros(labels.size + 1, dtype=torch.uint8, device=DEV), torch.zeros(logits.size + 1, device=DEV)
    lview, fview = lbuf[1:].view(labels.shape), fbuf[1:].view(logits.shape)
    lview.copy_(dev(labels))
    fview.copy_(dev(logits))
    assert lview.data_ptr() % 2 == 1 and fview.data_ptr() % 16 == 4 and lview.is_contiguous() and fview.is_contiguous()
    got = ops.eval_seg(torch.zeros(68, dtype=torch.int64, device=DEV), fview, lview, case["scale"])
    np.testing.assert_array_equal(got.cpu().numpy(), seg_spec(case))


def test_sections_are_added_to_and_nothing_else_is_touched():
    """Random 40-bit values everywhere, two launches into the middle: start + 2 * spec there, the guard words on both sides unchanged."""
    case = U.shape_case("odd_37x53")
    start = np.random.default_rng(0).integers(0, 1 << 40, 16 + 68 + 16).astype(np.int64)
    acc = dev(start.copy())
    seg_kernel(case, acc[16:84])
    seg_kernel(case, acc[16:84])
    want = start.copy()
    want[16:84] += 2 * seg_spec(case)
    np.testing.assert_array_equal(acc.cpu().numpy(), want)
    sc = U.scores_case(3, 52)
    start = np.random.default_rng(1).integers(0, 1 << 40, 16 + 6 + 2 * 256 + 16).astype(np.int64)
    acc = dev(start.copy())
    for _ in range(2):
        ops.eval_scores(acc[16:-16], dev(sc["scores"]), dev(sc["flags"]), sc["threshold"], 256)
    want = start.copy()
    want[16:-16] += 2 * C.eval_scores_numpy(np.zeros(6 + 512, np.int64), sc["scores"], sc["flags"], sc["threshold"], 256)
    np.testing.assert_array_equal(acc.cpu().numpy(), want)


def test_three_sections_of_one_accumulator():
    wide, tele, sc = U.shape_case("wide_head"), U.seg_case(77, 1, 4, 48, 120, 4), U.scores_case(9, 1)
    acc, want = torch.zeros(len(C.BRA), dtype=torch.int64, device=DEV), C.BRA.zeros()
    seg_kernel(wide, C.BRA.view(acc, "wide"))
    seg_kernel(tele, C.BRA.view(acc, "tele"))
    ops.eval_scores(C.BRA.view(acc, "scores"), dev(sc["scores"]), dev(sc["flags"]), 0.1, 256)
    seg_spec(wide, C.BRA.view(want, "wide"))
    seg_spec(tele, C.BRA.view(want, "tele"))
    C.eval_scores_numpy(C.BRA.view(want, "scores"), sc["scores"], sc["flags"], 0.1, 256)
    np.testing.assert_array_equal(acc.cpu().numpy(), want)
    assert C.BRA.named(want)["tele"]["pixels"] == 192 * 480 and C.BRA.named(want)["scores"]["samples"] == 1


@pytest.mark.parametrize("n", [1, 52, 1000])
@pytest.mark.parametrize("nbins", [1, 31, 256, 1024])
def test_scores_kernel_equals_specification(n, nbins):
    sc = U.scores_case(100 + n, n)
    want = C.eval_scores_numpy(np.zeros(6 + 2 * nbins, np.int64), sc["scores"], sc["flags"], sc["threshold"], nbins)
    if n >= 52:
        assert C.fields(want, C.SCORES)["nonfinite"] == 6 and C.fields(want, C.SCORES)["samples"] == n
    got = ops.eval_scores(torch.zeros(6 + 2 * nbins, dtype=torch.int64, device=DEV), dev(sc["scores"]), dev(sc["flags"]), sc["threshold"], nbins)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_bad_arguments_raise_before_any_launch():
    case = U.shape_case("scale4_9x13")
    acc = torch.zeros(len(C.BRA), dtype=torch.int64, device=DEV)
    sec, logits, labels = C.BRA.view(acc, "wide"), dev(case["logits"]), dev(case["labels"])
    with pytest.raises(ValueError, match="labels"):
        ops.eval_seg(sec, logits, labels[:, :-1], 4)
    with pytest.raises(ValueError, match="labels"):
        ops.eval_seg(sec, logits, labels, 2)
    with pytest.raises(ValueError, match="scale 3"):
        ops.eval_seg(sec, logits, labels, 3)
    with pytest.raises(ValueError, match="9 classes"):
        ops.eval_seg(sec, torch.zeros((1, 9, 9, 13), device=DEV), labels, 4)
    with pytest.raises(ValueError, match="HBM"):
        ops.eval_seg(sec, logits.cpu(), labels, 4)
    with pytest.raises(ValueError, match="float32"):
        ops.eval_seg(sec, logits.double(), labels, 4)
    with pytest.raises(ValueError, match="contiguous"):
        ops.eval_seg(sec, logits.transpose(2, 3).contiguous().transpose(2, 3), labels, 4)
    with pytest.raises(ValueError, match="68 words"):
        ops.eval_seg(acc[:67], logits, labels, 4)
    with pytest.raises(ValueError, match="HBM"):
        ops.eval_seg(torch.zeros(68, dtype=torch.int64), logits, labels, 4)
    scores, flags = torch.zeros(4, device=DEV), torch.zeros(4, dtype=torch.uint8, device=DEV)
    ssec = C.BRA.view(acc, "scores")
    with pytest.raises(ValueError, match="bins"):
        ops.eval_scores(ssec, scores, flags, 0.1, 1025)
    with pytest.raises(ValueError, match="words"):
        ops.eval_scores(ssec, scores, flags, 0.1, 100)
    with pytest.raises(ValueError, match="flags"):
        ops.eval_scores(ssec, scores, flags[:3], 0.1, 256)
    with pytest.raises(ValueError, match="HBM"):
        ops.eval_scores(ssec, scores.cpu(), flags, 0.1, 256)
    with pytest.raises(ValueError, match="float32"):
        ops.eval_scores(ssec, scores.double(), flags, 0.1, 256)
    with pytest.raises(ValueError, match="number"):
        ops.eval_scores(ssec, scores, flags, float("nan"), 256)
    assert int(acc.abs().sum()) == 0


def seeded(model, prefix):
    model.load_state_dict(synth.seeded_state_dict(model, prefix=prefix))
    return model.to(DEV).eval()


def test_seg_evaluator_adds_the_same_counters_on_the_device_and_on_the_host():
    from lav_amd.rgb import RGBSegmentationModel
    from lav_amd.train.synthetic import synthetic_seg_batch
    model = seeded(RGBSegmentationModel([4, 6, 7, 10]), "seg.")
    batches = [synthetic_seg_batch(4, seed=5), synthetic_seg_batch(2, seed=6)]       # calls of 3, 1 and 2 images
    on_gpu, on_host = C.SegEvaluator(model), C.SegEvaluator(model, device="cpu")
    assert on_gpu.run(batches) == on_host.run(batches) == 6
    assert on_gpu.acc.is_cuda and not on_host.acc.is_cuda
    got = on_gpu.counters()
    np.testing.assert_array_equal(got, on_host.counters())
    f = C.SEG.fields(got, "seg")
    assert int(f["images"]) == 6 and int(f["pixels"]) == 6 * 288 * 256 == int(f["ignored"]) + int(f["nonfinite"]) + int(f["conf"].sum())
    assert int(f["ignored"]) == 0 and on_gpu.precision() == on_host.precision()
    assert on_gpu.run(batches, max_images=8) == 8          # (two more, then it stops)


def test_brake_evaluator_adds_the_same_counters_on_the_device_and_on_the_host():
    from lav_amd.rgb import RGBBrakePredictionModel
    from lav_amd.train.synthetic import synthetic_bra_batch
    model = seeded(RGBBrakePredictionModel([4, 10, 18]), "bra.")
    batch = synthetic_bra_batch(2, seed=5)
    on_gpu, on_host = C.BrakeEvaluator(model), C.BrakeEvaluator(model, device="cpu")
    assert on_gpu.run([batch]) == on_host.run([batch]) == 2
    got = on_gpu.counters()
    np.testing.assert_array_equal(got, on_host.counters())
    named = C.BRA.named(got)
    for name, pixels in (("wide", 288 * 768), ("tele", 192 * 480)):
        s = named[name]
        assert s["images"] == 2 and s["pixels"] == 2 * pixels == s["ignored"] + s["nonfinite"] + int(np.sum(s["conf"]))
    assert named["scores"]["samples"] == 2 == named["scores"]["nonfinite"] + int(np.sum(named["scores"]["at"]))


@pytest.mark.parametrize("what,frames,pixels", [("seg", 6, 6 * 288 * 256), ("bra", 2, 2 * (288 * 768 + 192 * 480))])
def test_command_line_synthetic_at_every_offered_precision(what, frames, pixels, capsys):
    """--precision all: one line per arithmetic that ops.precision really switches in this net, each naming the one that was in force;
    the counters of each account for every label pixel fed.  How the predictions differ between them is what the tool is there to
    measure: nothing is asserted about it."""
    offered = list(C._WHAT[what]["precisions"])
    lines = C.main(what, ["--synthetic", "--frames", str(frames), "--precision", "all"])
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["precision"] for l in printed] == offered and len(lines) == len(offered)
    for l in printed:
        sections = [l["counters"]["seg"]] if what == "seg" else [l["counters"]["wide"], l["counters"]["tele"]]
        assert sum(s["images"] for s in sections) == frames * len(sections)
        assert sum(s["pixels"] for s in sections) == pixels == sum(s["ignored"] + s["nonfinite"] + int(np.sum(s["conf"])) for s in sections)
        assert l["what"] == ("eval_seg" if what == "seg" else "eval_bra_v2") and f"{frames} synthetic" in l["data"]
        if what == "seg":
            assert l["summary"]["images"] == frames and l["summary"]["pixels"] == pixels
        else:
            assert l["counters"]["scores"]["samples"] == frames and l["summary"]["brake"]["samples"] == frames
