"""lav_eval_det on the MI355X against its specification (lav_amd.train.evaluate_det.eval_det_numpy), every word of the accumulator compared
exactly; its centre arm against lav_eval_frame on the same device tensors; DetEvaluator with both head paths against the specification
on the rows the device produced; the command line.  The specification itself is checked in tests/test_eval_det_host.py."""
import json

import numpy as np
import pytest
import torch

from lav_amd import ops
from lav_amd.train import evaluate as F
from lav_amd.train import evaluate_det as E
from tests import eval_det_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def on_device(f):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if isinstance(a, np.ndarray) else a for a in U.positional(f)]


def nbins_of(f):
    return f["kw"].get("nbins", 256)


def kernel(f, acc=None):
    acc = torch.zeros(len(E.DetLayout(nbins_of(f))), dtype=torch.int64, device=DEV) if acc is None else acc
    return ops.eval_det(acc, *on_device(f), **f["kw"])


def spec(f, acc=None):
    acc = E.DetLayout(nbins_of(f)).zeros() if acc is None else acc
    return E.eval_det_numpy(acc, *U.positional(f), **f["kw"])


def same(f):
    got, want = kernel(f).cpu().numpy(), spec(f)
    lay = E.DetLayout(nbins_of(f))
    assert lay.named(got) == lay.named(want)
    np.testing.assert_array_equal(got, want)
    return want


@pytest.mark.parametrize("name", sorted(U.HAND))
def test_kernel_equals_specification_on_the_hand_cases(name):
    pred, gt, iou = U.HAND[name]
    for cls in (0, 1):
        want = same(U.pair_scene(pred, gt, cls=cls))
        lay = E.DetLayout()
        assert lay.view(want, "pairs").sum() == 1
        if iou in (0.0, 0.5, 1.0):
            assert lay.view(want, "sum_iou").sum() == int(iou * U.Q)


@pytest.mark.parametrize("D", [1, 15, 32])
@pytest.mark.parametrize("G", [0, 1, 20, 64])
def test_kernel_equals_specification_on_random_scenes(D, G):
    """Every row count with every actor count; n = 0 and n = G; sparse and heavily overlapping; 1, 256 and 1024 score bins."""
    if G == 0:
        f = U.random_scene(D, D=D, G=1, n=0, used=D)
        f["locs"], f["typs"] = f["locs"][:0], f["typs"][:0]
        same(f)
        return
    for k, nbins in enumerate((1, 256, 1024)):
        f = U.random_scene(31 * D + G + k, D=D, G=G, n=G if k else G // 2, used=D if k == 1 else None, heavy=k == 1, nbins=nbins)
        want = same(f)
        assert E.DetLayout(nbins).view(want, "hist").sum() > 0


def test_heavy_overlap_of_30_boxes_in_12_by_12_pixels():
    seen = 0
    for seed in range(4):
        f = U.random_scene(900 + seed, D=32, G=30, used=30, heavy=True)
        want = same(f)
        lay = E.DetLayout()
        seen += int(lay.view(want, "det")[1:, :, :, 0].sum())
    assert seen > 20          # the IoU arms matched something


def test_padding_rows_nan_scores_and_invalid_boxes_on_both_sides():
    for seed in range(4):
        f = U.random_scene(500 + seed, D=15, G=20, used=9, heavy=seed % 2 == 0, bad=True)
        want = same(f)
        lay = E.DetLayout()
        assert lay.view(want, "pred_invalid").sum() > 0 and lay.view(want, "gt_invalid").sum() > 0
    f = U.random_scene(3, bad=True)
    f["rows"][:, :, 1:3] = np.nan          # rows without a position: false positives everywhere
    f["locs"][2, 0] = np.nan
    f["locs"][3, 0] = np.inf
    same(f)
    # other thresholds: fewer of each, and dyadic ones
    same(dict(U.random_scene(8, heavy=True), kw=dict(ppm=U.PPM, centre=U.CENTRE, radius_px=3.0, iou_thresholds=(0.5,), range_edges_m=(2.0,),
                                                     heading_edges_deg=(30, 90), min_score=0.0, det_score=0.5, nbins=16)))
    same(dict(U.random_scene(9), kw=dict(ppm=U.PPM, centre=U.CENTRE, radius_px=0.0, iou_thresholds=(), range_edges_m=(), heading_edges_deg=())))


@pytest.mark.parametrize("nbins", [1, 256, 1024])
def test_two_launches_into_one_accumulator_and_two_sections(nbins):
    lay = E.det_layout(E.HEADS, nbins)
    start = np.random.default_rng(nbins).integers(0, 1 << 40, len(lay)).astype(np.int64)
    acc, want = torch.from_numpy(start.copy()).to(DEV), start.copy()
    for section, seeds in (("peaks", (1, 2)), ("dense", (3, 4))):
        for seed in seeds:
            f = U.random_scene(seed, heavy=seed % 2 == 0, bad=seed == 4, nbins=nbins)
            kernel(f, lay.view(acc, section))
            spec(f, lay.view(want, section))
    np.testing.assert_array_equal(acc.cpu().numpy(), want)
    for section in E.HEADS:
        assert lay.fields(want - start, section)["frames"].item() == 2


def test_centre_arm_equals_lav_eval_frame_on_the_same_tensors():
    for seed in range(6):
        f = U.random_scene(700 + seed, D=20, G=16, used=14, heavy=seed % 2 == 1, bad=seed == 5)
        rows, locs, typs, n, size_map, ori_map = on_device(f)
        mine = ops.eval_det(torch.zeros(len(E.DetLayout()), dtype=torch.int64, device=DEV), rows, locs, typs, n, size_map, ori_map, **f["kw"]).cpu().numpy()
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
        full = ops.eval_frame(torch.zeros(len(F.ACC), dtype=torch.int64, device=DEV), z(3, U.H, U.W), z(3, U.H, U.W, dtype=torch.uint8),
                              z(U.H, U.W, dtype=torch.uint8), rows, locs, typs, n, z(U.T, 2), z(U.T + 1, 2), 0, None, None, None, ppm=U.PPM,
                              centre=U.CENTRE, radius_px=U.RADIUS).cpu().numpy()
        lay = E.DetLayout()
        np.testing.assert_array_equal(lay.view(mine, "n_gt").sum(axis=1), F.ACC.view(full, "n_gt"))
        np.testing.assert_array_equal(lay.view(mine, "det")[0].sum(axis=1), F.ACC.view(full, "det"))
        np.testing.assert_array_equal(lay.view(mine, "hist")[0], F.ACC.view(full, "hist"))


def test_the_library_and_the_layout_agree_on_the_length():
    for nbins in (1, 7, 256, 1024):
        assert ops.eval_det_words(nbins) == len(E.DetLayout(nbins))


def test_bad_arguments_raise_before_any_launch():
    f = U.random_scene(5)
    acc = torch.zeros(len(E.DetLayout()), dtype=torch.int64, device=DEV)

    def call(acc=acc, **changed):
        g = dict(zip(U.ARGS, on_device(f)))
        kw = dict(f["kw"])
        for k in list(changed):
            if k not in U.ARGS:
                kw[k] = changed.pop(k)
        g.update(changed)
        return ops.eval_det(acc, *[g[k] for k in U.ARGS], **kw)

    z = lambda *shape, dtype=torch.float32, device=DEV: torch.zeros(shape, dtype=dtype, device=device)
    bad = [dict(rows=z(2, 33, 7)), dict(rows=z(2, 0, 7)), dict(rows=z(2, 15, 6)), dict(rows=z(1, 15, 7)), dict(rows=z(2, 15, 7, dtype=torch.float64)),
           dict(rows=torch.from_numpy(f["rows"])), dict(locs=z(65, 3, 2), typs=z(65, dtype=torch.int32)), dict(locs=z(20, 3, 3)), dict(typs=z(20, dtype=torch.int64)),
           dict(typs=z(19, dtype=torch.int32)), dict(n=21), dict(n=-1), dict(size_map=z(2, U.H, U.W + 1)), dict(ori_map=z(1, U.H, U.W)),
           dict(size_map=z(2, U.H, U.W, device="cpu")), dict(nbins=0), dict(nbins=1025), dict(nbins=32), dict(iou_thresholds=(0.1, 0.2, 0.3, 0.4)),
           dict(iou_thresholds=(1.5,)), dict(range_edges_m=(1, 2, 3, 4)), dict(range_edges_m=(3, 2)), dict(heading_edges_deg=tuple(range(1, 9))),
           dict(ppm=0.0), dict(radius_px=-1.0), dict(min_score=-0.5), dict(det_score=float("nan")), dict(acc=acc[:-1]), dict(acc=acc.cpu()),
           dict(acc=acc.to(torch.int32))]
    for changed in bad:
        with pytest.raises(ValueError):
            call(**changed)
    assert int(acc.abs().sum()) == 0
    call()
    assert int(acc[0]) == 1


def test_evaluator_with_both_head_paths_equals_the_specification_on_the_devices_rows():
    """DetEvaluator over 2 synthetic frames of 20 000 points, --heads both: the accumulator in HBM equals the specification run on the rows
    the device produced, in both sections."""
    from lav_amd.train.synthetic import synthetic_lidar_batch
    from tests.util import build_models
    lidar_model, _ = build_models(DEV)
    batch = synthetic_lidar_batch(2, seed=5, max_points=20000)
    ev = E.DetEvaluator(lidar_model, heads="both")
    want = ev.layout.zeros()
    for i in range(ev.upload(batch)):
        out = ev.forward(i)
        assert sorted(out) == ["dense", "peaks"] and all(r.is_cuda and tuple(r.shape) == (2, 15, 7) for r in out.values())
        ev.metrics(i, out)
        ev.frames += 1
        b = ev._batch
        for h, rows in out.items():
            E.eval_det_numpy(ev.layout.view(want, h), rows.cpu().numpy(), b["locs"][i].cpu().numpy(), b["typs"][i].cpu().numpy(), b["n"][i],
                             b["size"][i].cpu().numpy(), b["ori"][i].cpu().numpy(), **ev.kw)
    assert ev.acc.is_cuda and len(ev.acc) == 2 * len(E.DetLayout())
    got = ev.counters()
    np.testing.assert_array_equal(got, want)
    for h in E.HEADS:
        fields = ev.layout.fields(got, h)
        assert fields["frames"].item() == 2 and fields["hist"][0].sum() > 0
    # run() over the same batch counts the same
    again = E.DetEvaluator(lidar_model, heads="both")
    assert again.run([batch]) == 2
    np.testing.assert_array_equal(again.counters(), want)
    s = ev.summaries(got)
    assert s["peaks"]["frames"] == s["dense"]["frames"] == 2 and "NaN" not in json.dumps(s)


def test_command_line_synthetic(capsys):
    lines = E.main(["--synthetic", "--frames", "2", "--precision", "f16x3", "--max-points", "20000", "--heads", "both", "--iou", "0.5", "0.7"])
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == len(printed) == 1
    line = printed[0]
    assert line["what"] == "eval_det" and line["precision"] == "f16x3" and line["heads"] == "both" and line["measured"] == ["peaks", "dense"]
    assert "NOT applied" in line["note"] and "UNPINNED" in line["note"] and "smoke" in line["note"]
    assert line["iou_thresholds"] == [0.5, 0.7]
    lay = E.det_layout(E.HEADS)
    acc = lay.unnamed(line["counters"])
    for h in E.HEADS:
        assert line["summary"][h]["frames"] == 2 and line["summary"][h]["arms"] == ["centre", "iou0.5", "iou0.7"]
        assert line["summary"][h] == json.loads(json.dumps(E.summarise(acc[lay.sections[h]], iou_thresholds=(0.5, 0.7))))
    import eval_det_v2                                   # the tool at the top level is the same main
    one = eval_det_v2.main(["--synthetic", "--frames", "1", "--max-points", "20000"])
    assert one[0]["heads"] == "peaks" and one[0]["measured"] == ["peaks"] and list(one[0]["counters"]) == ["peaks"]
