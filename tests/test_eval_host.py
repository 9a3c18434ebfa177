"""CPU checks of the open-loop evaluation (lav_amd.train.evaluate): the specification against counters derived by hand, the summary,
order independence, the ground-truth pixel convention against the loader's own heat maps, the accumulator's length through the C ABI
and the per-sample seeding.  The kernel is held to this specification in tests/test_gpu_eval.py."""
import itertools

import numpy as np
import pytest
import torch

from lav_amd.train import evaluate as E
from tests import eval_util as U

Q = 1 << 20


def run(f, acc=None, nbins=256):
    acc = E.Layout(nbins).zeros() if acc is None else acc
    return E.eval_frame_numpy(acc, *U.positional(f), nbins=nbins, **f["kw"])


def expect(**fields):
    """An accumulator with the named slices set (flat index within the slice -> value), everything else 0."""
    acc = E.ACC.zeros()
    for name, items in fields.items():
        view = E.ACC.view(acc, name).reshape(-1)
        for i, v in (items.items() if isinstance(items, dict) else {0: items}.items()):
            view[i] = v
    return acc


def hist_at(c, kind, b):
    return (c * 2 + kind) * 256 + b


def test_every_scene_runs_and_counts_one_frame():
    for name, make in U.SCENES.items():
        acc = run(make())
        assert E.ACC.view(acc, "frames").item() == 1 and (acc >= 0).all(), name
    acc = run(U.scene_empty())
    assert np.array_equal(acc, expect(frames=1, plan={6: 1})), "empty: one frame, the plan of command 2 on its target, nothing else"
    acc = run(U.scene_nonfinite())
    v = lambda n: E.ACC.view(acc, n).reshape(-1)[0]
    assert v("plan_nonfinite") == 1 and E.ACC.view(acc, "plan").sum() == 0
    assert (v("oth_matched"), v("oth_unmatched"), v("oth_nonfinite")) == (2, 0, 1)
    for make in (U.SCENES["others7"], U.scene_full):       # the scenes the kernel is compared on hold forecasts of both kinds
        acc = run(make())
        assert v("oth_matched") >= 1 and v("oth_unmatched") >= 1 and v("oth_matched") + v("oth_unmatched") == 7
    acc = run(U.scene_full())
    assert (E.ACC.view(acc, "hist").sum(axis=(1, 2)) == U.D).all(), "full: all 20 rows of both classes are used"


def test_compete_greedy_order_decides():
    """Actors 0 (20, 10) and 1 (40, 10), class 1.  Row 0 (0.9, at (22, 10)) is 2 px from actor 0 and takes it.  Row 1 (0.8, at (21, 10))
    is nearer to actor 0 (1 px) but that one is taken; the nearest free actor is 19 px away, beyond the 8 px radius: a false positive.
    Row 2 (0.7, at (40, 12)) is 2 px from actor 1: a true positive.  All three scores exceed 0.2.  Bins: int(float32(0.9) * 256) =
    int(230.39...) = 230, int(204.80...) = 204, int(179.19...) = 179.  The plan is on its target: command 2 gets (1, 0, 0)."""
    want = expect(frames=1, n_gt={1: 2}, det={2: 2, 3: 1}, plan={6: 1},
                  hist={hist_at(1, 0, 230): 1, hist_at(1, 1, 204): 1, hist_at(1, 0, 179): 1})
    assert np.array_equal(run(U.scene_compete()), want)


def test_tie_goes_to_the_lowest_index():
    """Row 0 of class 1 at (22, 10) is 2 px from actor 1 (20, 10) and from actor 3 (24, 10): it takes actor 1.  Its forecast is actor 1's
    future moved 1 m in x in every mode: q_t = 2^20 for each of the 20 waypoints, so S_m = 20 * 2^20 for every mode (best and top alike),
    the final q is 2^20.  Had it taken actor 3 (another track) these sums would differ.  Pedestrians 0 and 2 are in the map, no row is
    theirs: n_gt = (2, 2).  Score 0.5 -> bin 128."""
    want = expect(frames=1, n_gt={0: 2, 1: 2}, det={2: 1}, plan={6: 1}, hist={hist_at(1, 0, 128): 1},
                  oth_matched=1, oth_min=20 * Q, oth_top=20 * Q, oth_top_final=Q)
    assert np.array_equal(run(U.scene_tie()), want)


def test_outside_actors_are_ignored():
    """Of the class-1 centres x = -0.5 (out), 52.75 (in), 0 (in), 53 = W (out), y = -0.25 (out), 36.75 (in), 37 = H (out), three count.
    Row 0 (0.9) sits on the actor at x = 0, row 1 (0.6, at (52, 10)) is 0.75 px from the one at 52.75: two true positives.  Row 2 (0.5,
    at (45, 10)) is exactly 8 px from the ignored actor at x = W - which would match, the radius being inclusive - and far from the one
    free actor at (10, 36.75): a false positive.  Bins 230, int(float32(0.6) * 256) = int(153.60...) = 153, 128."""
    want = expect(frames=1, n_gt={1: 3}, det={2: 2, 3: 1}, plan={6: 1},
                  hist={hist_at(1, 0, 230): 1, hist_at(1, 0, 153): 1, hist_at(1, 1, 128): 1})
    assert np.array_equal(run(U.scene_outside()), want)


def test_edges_of_every_comparison():
    """min_score 0.125, det_score 0.25.  Class 0, three actors in the map.  Row 0: score 1.0 on actor 0 - true positive, bin
    min(255, int(256.0)) = 255, above det_score.  Row 1: 0.5 with no actor near - false positive, bin 128, above det_score.  Row 2: 0.25 on
    actor 1 - used (0.25 > 0.125), true positive, bin 64, NOT above det_score (strict).  Row 3: 0.125 on actor 2 - not used (strict).
    Row 4: NaN - skipped.  So det[0] = (1, 1).
    Segmentation, mask = columns < 30: channel 0 predicts exactly the threshold everywhere (not above it: no positive) and has 3 x 4
    labels in the mask: (0, 0, 12).  Channel 1 predicts 0.75 everywhere, rows < 10 are labelled: tp = 10 * 30, fp = 27 * 30, fn = 0.
    Channel 2 predicts and is labelled only where the mask is 0: (0, 0, 0).
    The plan is 0.5 m off at each of 20 waypoints: command 5 gets (1, 20 * 2^19, 2^19)."""
    want = expect(frames=1, n_gt={0: 3}, det={0: 1, 1: 1}, seg={2: 12, 3: 300, 4: 810}, plan={15: 1, 16: 20 * (Q // 2), 17: Q // 2},
                  hist={hist_at(0, 0, 255): 1, hist_at(0, 1, 128): 1, hist_at(0, 0, 64): 1})
    assert np.array_equal(run(U.scene_edges()), want)


def test_perfect_predictions_and_an_exact_shift():
    s = E.summarise(run(U.perfect()))
    assert s["seg"]["iou"] == [1.0, 1.0, 1.0] and s["seg"]["mean_iou"] == 1.0
    for d in s["det"]:
        assert (d["n_gt"], d["tp"], d["fp"], d["fn"]) == (4, 4, 0, 0) and d["precision"] == d["recall"] == d["ap"] == 1.0
    assert s["plan"]["ade"] == s["plan"]["fde"] == 0.0 and s["plan"]["per_cmd"][1]["frames"] == 1
    assert s["others"] == dict(matched=4, unmatched=0, nonfinite=0, min_ade=0.0, top_ade=0.0, top_fde=0.0)
    # moved by exactly 1 m in x: every q is 2^20, the averages are 1.0 to the last bit
    s = E.summarise(run(U.perfect(shift=1.0)))
    assert s["plan"]["ade"] == s["plan"]["fde"] == 1.0
    assert s["others"]["min_ade"] == s["others"]["top_ade"] == s["others"]["top_fde"] == 1.0
    assert s["det"][0]["ap"] == 1.0, "the rows did not move"


def test_summary_of_nothing_and_average_precision_by_hand():
    s = E.summarise(E.ACC.zeros())
    assert s["frames"] == 0 and s["seg"]["iou"] == [None] * 3 and s["seg"]["mean_iou"] is None
    assert all(d["precision"] is None and d["recall"] is None and d["ap"] is None for d in s["det"])
    assert s["plan"]["ade"] is None and s["plan"]["fde"] is None and all(c["ade"] is None for c in s["plan"]["per_cmd"])
    assert s["others"]["min_ade"] is None and s["others"]["top_fde"] is None
    import json
    json.dumps(s)
    # four bins, four actors.  True positives: 2 in bin 3, 1 in bin 1; false positives: 1 in bin 2, 1 in bin 0.  From the top:
    # (recall, precision) = (0.5, 1), (0.5, 2/3), (0.75, 0.75), (0.75, 0.6); the envelope from the low end: 0.6, 0.75, 0.75, 1.
    # AP = 0.5 * 1 + 0 * 0.75 + 0.25 * 0.75 + 0 * 0.6 = 0.6875
    assert E.average_precision([0, 1, 0, 2], [1, 0, 1, 0], 4) == 0.6875
    lay = E.Layout(4)
    acc = lay.zeros()
    lay.view(acc, "hist")[1] = [[0, 1, 0, 2], [1, 0, 1, 0]]
    lay.view(acc, "n_gt")[1] = 4
    assert E.summarise(acc)["det"][1]["ap"] == 0.6875 and E.summarise(acc)["det"][0]["ap"] is None


def test_accumulation_does_not_depend_on_the_order():
    frames = [U.scene_full(), U.scene_others(7), U.scene_edges()]
    accs = []
    for order in itertools.permutations(range(3)):
        acc = E.ACC.zeros()
        for i in order:
            run(frames[i], acc)
        accs.append(acc)
    assert E.ACC.view(accs[0], "frames").item() == 3
    for a in accs[1:]:
        assert np.array_equal(a, accs[0])


def test_ground_truth_pixels_are_where_the_loader_draws_them(tmp_path):
    """detections_to_heatmap draws a unit-radius Gaussian exp(-dx^2 - dy^2) at float32(loc) * ppm + centre; the evaluator's pixel is the
    same product in float64, so the pixel nearest to it is at most 0.5 px off per axis: the heat there is at least exp(-0.5).  An actor
    whose centre is a pixel or more outside the map leaves less than that on the border pixel nearest to it (exp(-1)), unless another
    actor of its class is near."""
    from lav_amd.train.lav import LAV, TrainConfig  # noqa: F401  (bev_center's formula is restated below)
    from tests.util import dataset_fixture_config
    frames = E.held_out_frames(dataset_fixture_config(str(tmp_path), routes=2, frames=26), seed=0)
    cfg = TrainConfig()
    Hm, Wm = 320, 320
    centre = (Wm / 2 + (cfg.min_y + cfg.max_y) / 2 * cfg.pixels_per_meter, Hm / 2 + (cfg.min_x + cfg.max_x) / 2 * cfg.pixels_per_meter)
    assert centre == (160.0, 280.0)
    bound = np.exp(-0.5)
    inside = outside = 0
    for idx in range(len(frames)):
        item = frames[idx]
        heat, locs, typs, n = item[2].numpy(), item[10], item[12], item[13]
        px = locs[:n, 0, 0].astype(np.float64) * cfg.pixels_per_meter + centre[0]
        py = locs[:n, 0, 1].astype(np.float64) * cfg.pixels_per_meter + centre[1]
        for g in range(n):
            c = int(typs[g])
            assert c in (0, 1)
            if 0.0 <= px[g] < Wm and 0.0 <= py[g] < Hm:
                x, y = int(np.rint(px[g])), int(np.rint(py[g]))
                if x < Wm and y < Hm:
                    inside += 1
                    assert heat[c, y, x] >= bound, (idx, g, px[g], py[g], heat[c, y, x])
                continue
            x, y = int(np.clip(np.rint(px[g]), 0, Wm - 1)), int(np.clip(np.rint(py[g]), 0, Hm - 1))
            away = max(-px[g], px[g] - (Wm - 1), -py[g], py[g] - (Hm - 1))
            near = [k for k in range(n) if k != g and typs[k] == c and abs(px[k] - x) < 3 and abs(py[k] - y) < 3]
            if away >= 1.0 and not near:
                outside += 1
                assert heat[c, y, x] < bound, (idx, g, px[g], py[g], heat[c, y, x])
    assert inside >= 10, (inside, outside)


def test_layout_has_the_length_the_library_says():
    from lav_amd import _lib
    lib = _lib.load()
    assert len(E.ACC) == lib.lav_eval_acc_words(256) == 41 + 4 * 256
    assert len(E.Layout(1)) == lib.lav_eval_acc_words(1) and len(E.Layout(1024)) == lib.lav_eval_acc_words(1024)
    assert lib.lav_eval_acc_words(0) == 0 and lib.lav_eval_acc_words(1025) == 0
    assert E.Layout.of(E.ACC.zeros()).nbins == 256


def test_samples_do_not_depend_on_the_worker_that_loads_them(tmp_path):
    from tests.util import dataset_fixture_config
    cfg = dataset_fixture_config(str(tmp_path), routes=1, frames=24)
    passes = []
    for workers in (0, 2):
        frames = E.held_out_frames(cfg, seed=7)
        assert frames.dataset.angle_jitter == 0 and frames.dataset.stack_loc_jitter == 0 and frames.dataset.stack_ori_jitter == 0
        loader = torch.utils.data.DataLoader(frames, batch_size=2, shuffle=False, drop_last=False, num_workers=workers)
        passes.append([t for batch in loader for t in batch])
    assert len(passes[0]) == len(passes[1]) == 2 * 14 and sum(len(t) for t in passes[0][::14]) == 4
    for a, b in zip(*passes):
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))


def test_forecast_rows_name_the_rows_the_others_branch_decodes():
    """forecast_rows against det_decode_fast's own ego-frame positions: forecast k is made at locs[k], which must be row
    other_row[k]'s pixel - through score, size and range filters and the ego-box skip (rows as in test_capi_host's decode test)."""
    import types
    from lav_amd.model_inference import InferModel
    from lav_amd.uniplanner import UniPlanner
    up = types.SimpleNamespace(pixels_per_meter=4, offsets=lambda: (0.0, 0.75))
    up.others_from_detections = lambda det, H, W: UniPlanner.others_from_detections(up, det, H, W)
    im = types.SimpleNamespace(pixels_per_meter=4, uniplanner=up, _bev_hw=(320, 320))
    rng = np.random.default_rng(1)
    total = 0
    for trial in range(30):
        rows = np.zeros((2, 20, 7), np.float32)
        rows[..., 0] = np.sort(rng.uniform(-0.2, 1.0, (2, 20)), axis=1)[:, ::-1]
        pix = rng.permutation(120 * 169)[:40].reshape(2, 20)                      # peaks of one class never share a pixel
        rows[..., 1], rows[..., 2] = 100 + pix % 120, 150 + pix // 120
        rows[..., 3:5] = rng.uniform(0, 3, (2, 20, 2)); rows[..., 5:7] = rng.normal(size=(2, 20, 2))
        rows[1, 0, 1:3] = (160, 280); rows[1, 1, 1:3] = (161, 282); rows[1, 2, 1:3] = (163, 281)    # the ego's own box
        dets, locs, _ = InferModel.det_decode_fast(im, rows)
        other_row = E.forecast_rows(im, rows, dets[1])
        assert other_row.dtype == np.int32 and len(other_row) == len(locs) and (np.diff(other_row) > 0).all()
        np.testing.assert_array_equal((rows[1, other_row, 1:3].astype(np.float64) - (160.0, 280.0)) / 4, locs)
        total += len(locs)
    assert total > 100


def test_data_dir_override_changes_nothing_by_default(tmp_path):
    from lav_amd.data.datasets import TemporalLiDARPaintedDataset
    from tests.util import dataset_fixture_config
    cfg = dataset_fixture_config(str(tmp_path), routes=1, frames=23)
    a = TemporalLiDARPaintedDataset(cfg)
    b = TemporalLiDARPaintedDataset(cfg, overrides=dict(data_dir=a.data_dir))
    assert len(a) == len(b) == 3 and a.dir_map == b.dir_map
    with pytest.raises(Exception):
        E.held_out_frames(cfg, data_dir=str(tmp_path / "nowhere"))[0]
