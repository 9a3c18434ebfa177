"""The specifications of the camera evaluation (lav_amd.train.evaluate_camera.eval_seg_numpy / eval_scores_numpy) against counters
derived by hand and against torch's own nearest up-sampling, the summaries on known fractions, the accumulator's layout and the command
lines' refusal of a missing checkpoint.  No GPU: the kernels are compared with these specifications in tests/test_gpu_eval_camera.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lav_amd.train import evaluate_camera as C
from tests import eval_camera_util as U


def seg_fields(section):
    return C.fields(section, "seg")


def score_fields(section):
    return C.fields(section, C.SCORES)


def seg_words(**named):
    s = np.zeros(C.SEG_WORDS, np.int64)
    f = seg_fields(s)
    for k, v in named.items():
        f[k][...] = np.asarray(v)
    return s


def logits_for(pred, k, margin=1.0):
    """(1, k, h, w) float32 whose first maximum is pred[y, x]."""
    pred = np.asarray(pred)
    x = np.zeros((1, k) + pred.shape, np.float32)
    for c in range(k):
        x[0, c][pred == c] = margin
    return x


def conf_of(rows):
    c = np.zeros((8, 8), np.int64)
    r = np.asarray(rows)
    c[:r.shape[0], :r.shape[1]] = r
    return c


BLOCKS = {(0, 0): [0, 0, 0, 1], (0, 1): [0, 1, 1, 2], (0, 2): [2, 2, 2, 2], (1, 0): [1, 2, 2, 0], (1, 1): [1, 1, 1, 1], (1, 2): [0, 0, 1, 2]}
NINE = [[4, 1, 2], [2, 6, 1], [2, 1, 5]]      # conf[label][prediction] of BLOCKS under predictions [[0, 1, 2], [0, 1, 2]]


def nine_cells():
    labels = np.zeros((1, 4, 6), np.uint8)
    for (y, x), four in BLOCKS.items():
        labels[0, 2 * y:2 * y + 2, 2 * x:2 * x + 2] = np.asarray(four).reshape(2, 2)
    return logits_for([[0, 1, 2], [0, 1, 2]], 3), labels


def test_nine_cells_by_hand():
    """A 2 x 3 map of three classes at scale 2: column x predicts class x, the 2 x 2 label blocks are BLOCKS; counted by hand."""
    logits, labels = nine_cells()
    got = C.eval_seg_numpy(np.zeros(68, np.int64), logits, labels, 2)
    np.testing.assert_array_equal(got, seg_words(images=1, pixels=24, conf=conf_of(NINE)))
    C.eval_seg_numpy(got, logits, labels, 2)                       # added to, not overwritten
    np.testing.assert_array_equal(got, 2 * seg_words(images=1, pixels=24, conf=conf_of(NINE)))


def test_a_tie_goes_to_the_lower_index():
    logits = np.full((1, 4, 1, 3), -1.0, np.float32)
    logits[0, [1, 3], 0, 0] = 2.0          # channels 1 and 3 tie: 1
    logits[0, :, 0, 1] = 0.5               # all four tie: 0
    logits[0, [2, 3], 0, 2] = 7.0          # 2 and 3: 2
    labels = np.array([[[3, 3, 3]]], np.uint8)
    got = seg_fields(C.eval_seg_numpy(np.zeros(68, np.int64), logits, labels, 1))
    want = np.zeros((8, 8), np.int64)
    want[3, [1, 0, 2]] = 1
    np.testing.assert_array_equal(got["conf"], want)


@pytest.mark.parametrize("channel,value", [(0, np.nan), (1, np.nan), (2, np.nan), (1, np.inf), (0, -np.inf)])
def test_a_pixel_that_is_not_finite_counts_in_nonfinite_only(channel, value):
    logits, labels = nine_cells()
    logits[0, channel, 1, 1] = value       # the pixel of block (1, 1): four label pixels of class 1, predicted 1
    labels[0, 2, 2] = 200                  # an out-of-range label under it: still nonfinite, not ignored
    conf = conf_of(NINE)
    conf[1, 1] -= 4
    got = C.eval_seg_numpy(np.zeros(68, np.int64), logits, labels, 2)
    np.testing.assert_array_equal(got, seg_words(images=1, pixels=24, nonfinite=4, conf=conf))


def test_labels_out_of_range_are_ignored():
    logits, labels = nine_cells()
    labels[0, 0, 0], labels[0, 3, 5] = 3, 255      # a label equal to k (was 0 under prediction 0) and 255 (was 2 under prediction 2)
    conf = conf_of(NINE)
    conf[0, 0] -= 1
    conf[2, 2] -= 1
    got = C.eval_seg_numpy(np.zeros(68, np.int64), logits, labels, 2)
    np.testing.assert_array_equal(got, seg_words(images=1, pixels=24, ignored=2, conf=conf))


@pytest.mark.parametrize("scale", [4, 2])
def test_scale_is_torchs_nearest_upsampling_then_argmax(scale):
    case = U.seg_case(5 + scale, 2, 4, 9, 13, scale, plant=False)
    logits, labels = case["logits"], case["labels"]
    assert labels.shape == (2, 9 * scale, 13 * scale)
    pred = F.interpolate(torch.from_numpy(logits), scale_factor=scale).argmax(1).numpy()
    want = np.zeros((8, 8), np.int64)
    np.add.at(want, (labels.astype(np.int64), pred), 1)
    got = seg_fields(C.eval_seg_numpy(np.zeros(68, np.int64), logits, labels, scale))
    np.testing.assert_array_equal(got["conf"], want)
    assert (want[:4, :4] > 0).all() and int(got["pixels"]) == labels.size == want.sum() and int(got["ignored"]) == int(got["nonfinite"]) == 0


def test_the_planted_cases_plant_what_they_say():
    case = U.shape_case("odd_37x53")
    f = seg_fields(C.eval_seg_numpy(np.zeros(68, np.int64), case["logits"], case["labels"], case["scale"]))
    kinds = [k for k, _ in case["planted"]]
    assert kinds.count("nan") == 3 and "inf" in kinds and "-inf" in kinds and "tie" in kinds
    assert int(f["nonfinite"]) == 5 and 1 <= int(f["ignored"]) <= 4 and (f["conf"][:5, :5] > 0).all()
    assert int(f["pixels"]) == int(f["ignored"]) + int(f["nonfinite"]) + int(f["conf"].sum()) == 2 * 37 * 53


# ------------------------------------------------------------------------------------------------------------ scores
SCORES = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), -0.25, np.nan, np.inf], np.float32)
FLAGS = np.array([1, 7, 0, 0, 255, 0, 1, 0], np.uint8)


@pytest.mark.parametrize("nbins,hist", [
    (1, {(0, 0): 3, (1, 0): 3}),
    (100, {(1, 50): 2, (0, 0): 2, (0, 99): 1, (1, 99): 1}),
    (1024, {(1, 512): 2, (0, 0): 2, (0, 1023): 1, (1, 1023): 1})])
def test_scores_by_hand(nbins, hist):
    """Threshold 0.5: 0.5 itself is not above it, the next float32 is; 1.0 and the float32 below it fall in the last bin, 0.0 and -0.25
    in bin 0; the NaN and the Inf count in samples and nonfinite only."""
    got = score_fields(C.eval_scores_numpy(np.zeros(6 + 2 * nbins, np.int64), SCORES, FLAGS, 0.5, nbins))
    want = np.zeros((2, nbins), np.int64)
    for at, count in hist.items():
        want[at] = count
    assert int(got["samples"]) == 8 and int(got["nonfinite"]) == 2
    np.testing.assert_array_equal(got["at"], [[2, 1], [1, 2]])       # [flag][above]: negatives 0.0, -0.25 | 1.0; positives 0.5 | next, ~1
    np.testing.assert_array_equal(got["hist"], want)


def test_the_threshold_is_compared_in_float64():
    """float32(0.1) = 0.100000001490116... is above the double 0.1 - the agent's `pred_bra > 0.1` on a Python float -, and not above
    itself."""
    s = np.array([0.1], np.float32)
    assert score_fields(C.eval_scores_numpy(np.zeros(14, np.int64), s, [1], 0.1, 4))["at"].tolist() == [[0, 0], [0, 1]]
    assert score_fields(C.eval_scores_numpy(np.zeros(14, np.int64), s, [1], float(s[0]), 4))["at"].tolist() == [[0, 0], [1, 0]]


def test_far_scores_take_the_end_bins():
    got = score_fields(C.eval_scores_numpy(np.zeros(6 + 2 * 256, np.int64), np.array([3e38, -3e38], np.float32), [0, 0], 0.1, 256))
    assert got["hist"][0, 255] == 1 and got["hist"][0, 0] == 1 and int(got["nonfinite"]) == 0


def test_a_score_section_of_31_bins_is_as_long_as_a_map_section():
    """6 + 2 * 31 = 68 words: a section's kind is said where it is used, never guessed from its length."""
    section = C.eval_scores_numpy(np.zeros(68, np.int64), SCORES, FLAGS, 0.5, 31)
    got = score_fields(section)
    want = np.zeros((2, 31), np.int64)
    want[0, 0], want[0, 30], want[1, 15], want[1, 30] = 2, 1, 2, 1        # 0.5 * 31 = 15.5 and the next float32: bin 15
    assert int(got["samples"]) == 8 and int(got["nonfinite"]) == 2 and got["at"].tolist() == [[2, 1], [1, 2]]
    np.testing.assert_array_equal(got["hist"], want)
    s = C.summarise_scores(section)
    assert (s["tn"], s["fp"], s["fn"], s["tp"]) == (2, 1, 1, 2) and (s["positives"], s["negatives"]) == (3, 3) and s["nonfinite"] == 2
    lay = C.CameraLayout((), nbins=31)
    named = lay.named(section)
    assert len(lay) == 68 and set(named) == {"scores"} and set(named["scores"]) == {"samples", "nonfinite", "at", "hist"}
    assert named["scores"]["hist"] == want.tolist()
    np.testing.assert_array_equal(lay.unnamed(named), section)
    both = C.CameraLayout(("m",), nbins=31)                              # two sections of 68 words, one of each kind
    acc = both.zeros()
    C.eval_seg_numpy(both.view(acc, "m"), *nine_cells(), 2)
    C.eval_scores_numpy(both.view(acc, "scores"), SCORES, FLAGS, 0.5, 31)
    assert both.named(acc)["m"]["conf"][1][1] == 6 and both.named(acc)["scores"]["hist"] == want.tolist()
    assert C.summarise_seg(both.view(acc, "m"), 3)["labelled"] == [7, 9, 8]
    with pytest.raises(ValueError):
        C.fields(np.zeros(67, np.int64), C.SCORES)
    with pytest.raises(ValueError):
        C.fields(np.zeros(70, np.int64), "seg")


# ------------------------------------------------------------------------------------------------------------ summaries
def test_summarise_seg_on_known_fractions():
    s = C.summarise_seg(seg_words(images=1, pixels=27, ignored=2, nonfinite=1, conf=conf_of(NINE)), 3)
    assert s["iou"] == [4 / 11, 6 / 11, 5 / 11] and s["mean_iou"] == pytest.approx(5 / 11, rel=1e-15)
    assert s["accuracy"] == 15 / 24 and s["precision"] == [4 / 8, 6 / 8, 5 / 8] and s["recall"] == [4 / 7, 6 / 9, 5 / 8]
    assert s["labelled"] == [7, 9, 8] and (s["images"], s["pixels"], s["ignored"], s["nonfinite"]) == (1, 27, 2, 1)
    # a fourth class that is neither labelled nor predicted: None, and the mean is over the three that have an IoU
    s = C.summarise_seg(seg_words(conf=conf_of(NINE)), 4)
    assert s["iou"][3] is None and s["precision"][3] is None and s["recall"][3] is None and s["mean_iou"] == pytest.approx(5 / 11, rel=1e-15)
    empty = C.summarise_seg(seg_words(), 5)
    assert empty["mean_iou"] is None and empty["accuracy"] is None and empty["iou"] == [None] * 5


def test_summarise_scores_on_known_fractions():
    s = np.zeros(6 + 2 * 4, np.int64)
    f = score_fields(s)
    f["samples"][...], f["nonfinite"][...] = 11, 1
    f["at"][...] = [[5, 1], [2, 2]]
    f["hist"][...] = [[5, 0, 1, 0], [0, 2, 0, 2]]
    got = C.summarise_scores(s)
    assert (got["tn"], got["fp"], got["fn"], got["tp"]) == (5, 1, 2, 2) and (got["positives"], got["negatives"]) == (4, 6)
    assert got["precision"] == 2 / 3 and got["recall"] == 1 / 2 and got["f1"] == 4 / 7 and got["accuracy"] == 7 / 10
    # points from the top bin down: (1/2, 1), (1/2, 2/3), (1, 4/5), (1, 2/5); envelope 1, 4/5, 4/5, 2/5: 1/2 * 1 + 1/2 * 4/5
    assert got["ap"] == pytest.approx(0.9, rel=1e-15) and got["nonfinite"] == 1 and got["samples"] == 11
    none = C.summarise_scores(np.zeros(14, np.int64))
    assert none["precision"] is None and none["recall"] is None and none["f1"] is None and none["ap"] is None and none["accuracy"] is None


# ------------------------------------------------------------------------------------------------------------ layout
def test_layout():
    assert len(C.SEG) == 68 and len(C.BRA) == 68 + 68 + 6 + 2 * 256 and C.BRA.nbins == 256 and C.SEG.nbins is None
    lay = C.CameraLayout(("a", "b"), nbins=10)
    acc = lay.zeros()
    assert acc.dtype == np.int64 and len(acc) == len(lay) == 136 + 26
    assert [len(lay.view(acc, n)) for n in ("a", "b", "scores")] == [68, 68, 6 + 2 * 10]
    lay.view(acc, "b")[4] += 5                       # a view: conf[0][0] of section b
    lay.fields(acc, "scores")["hist"][1, 9] += 3
    assert acc[68 + 4] == 5 and acc[-1] == 3 and acc.sum() == 8
    t = torch.zeros(len(lay), dtype=torch.int64)
    lay.view(t, "a")[3] += 2
    assert int(t[3]) == 2 and lay.view(t, "scores").shape == (26,)
    acc[:] = np.random.default_rng(0).integers(0, 1 << 40, len(acc))
    named = lay.named(acc)
    assert set(named) == {"a", "b", "scores"} and named["b"]["conf"][0][0] == acc[68 + 4] and len(named["scores"]["hist"][1]) == 10
    np.testing.assert_array_equal(lay.unnamed(named), acc)
    with pytest.raises(ValueError):
        C.CameraLayout(("a",), nbins=1025)
    with pytest.raises(ValueError):
        C.eval_seg_numpy(np.zeros(67, np.int64), np.zeros((1, 3, 2, 2), np.float32), np.zeros((1, 2, 2), np.uint8), 1)
    with pytest.raises(ValueError):
        C.eval_seg_numpy(np.zeros(68, np.int64), np.zeros((1, 3, 2, 2), np.float32), np.zeros((1, 4, 5), np.uint8), 2)


# ------------------------------------------------------------------------------------------------------------ command lines
@pytest.mark.parametrize("what,key", [("seg", "seg_model_dir"), ("bra", "bra_model_dir")])
def test_a_missing_checkpoint_is_an_error(what, key, tmp_path):
    """Named on the command line or by the config: a file that is not there ends the run with a sentence, before anything else
    (a GPU included) is asked for."""
    with pytest.raises(SystemExit) as e:
        C.main(what, ["--synthetic", f"--{what}", str(tmp_path / "absent.th")])
    assert e.value.code not in (0, None) and key in str(e.value.code) and "absent.th" in str(e.value.code)
    cfg = tmp_path / "config.yaml"
    cfg.write_text(f"{key}: weights/none_{what}.th\ndata_dir: {tmp_path}\n")
    with pytest.raises(SystemExit) as e:
        C.main(what, ["--config-path", str(cfg)])
    assert e.value.code not in (0, None) and key in str(e.value.code) and f"none_{what}.th" in str(e.value.code)
    cfg.write_text(f"data_dir: {tmp_path}\n")
    with pytest.raises(SystemExit) as e:
        C.main(what, ["--config-path", str(cfg)])
    assert key in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        C.main(what, [])
    assert "--config-path" in str(e.value.code)
