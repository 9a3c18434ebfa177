"""lav_eval_frame on the MI355X against its specification (lav_amd.train.evaluate.eval_frame_numpy), every word of the accumulator
compared exactly, and the evaluator's command line end to end.  The specification itself is checked in tests/test_eval_host.py."""
import json

import numpy as np
import pytest
import torch

from lav_amd import ops
from lav_amd.train import evaluate as E
from tests import eval_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def on_device(f):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if isinstance(a, np.ndarray) else a for a in U.positional(f)]


def kernel(f, acc=None, nbins=256):
    acc = torch.zeros(len(E.Layout(nbins)), dtype=torch.int64, device=DEV) if acc is None else acc
    return ops.eval_frame(acc, *on_device(f), nbins=nbins, **f["kw"])


def spec(f, acc=None, nbins=256):
    acc = E.Layout(nbins).zeros() if acc is None else acc
    return E.eval_frame_numpy(acc, *U.positional(f), nbins=nbins, **f["kw"])


@pytest.mark.parametrize("name", sorted(U.SCENES))
def test_kernel_equals_specification_on_every_scene(name):
    f = U.SCENES[name]()
    np.testing.assert_array_equal(kernel(f).cpu().numpy(), spec(f))


@pytest.mark.parametrize("h,w,centre", [(320, 320, (160.0, 280.0)), (1, 1, (0.0, 0.0)), (8, 4, (2.0, 4.0))])
def test_kernel_equals_specification_at_other_sizes(h, w, centre):
    """320 x 320 (the frame's: every plane 16-byte aligned, 100 workgroups), and maps smaller than one workgroup's share."""
    f = U.random_frame(31 + h, h=h, w=w, centre=centre, N=7)
    np.testing.assert_array_equal(kernel(f).cpu().numpy(), spec(f))
    if h == 320:     # other bin counts, the histogram's limits
        for nbins in (1, 100, 1024):
            np.testing.assert_array_equal(kernel(f, nbins=nbins).cpu().numpy(), spec(f, nbins=nbins))


def test_three_frames_into_one_buffer():
    frames = [U.scene_full(), U.scene_others(7), U.scene_edges()]
    acc, want = None, None
    for f in frames:
        acc, want = kernel(f, acc), spec(f, want)
    np.testing.assert_array_equal(acc.cpu().numpy(), want)
    assert E.ACC.view(want, "frames").item() == 3


def test_the_accumulator_is_added_to():
    f = U.scene_full()
    start = np.random.default_rng(0).integers(0, 1 << 40, len(E.ACC)).astype(np.int64)
    acc = torch.from_numpy(start.copy()).to(DEV)
    kernel(f, acc)
    kernel(f, acc)
    np.testing.assert_array_equal(acc.cpu().numpy(), start + 2 * spec(f))


def test_peaks_of_the_loaders_heat_maps_are_true_positives():
    """Five hand-placed objects at least 12 px apart, drawn by the loader's detections_to_heatmap, found by lav_extract_peaks, matched
    here: every peak is the pixel nearest to a centre (score >= exp(-0.5) > 0.2, at most 0.71 px away), the zero plateau's peaks score
    0 < min_score.  5 true positives, nothing else."""
    import types
    from lav_amd.data.datasets import LiDARDataset
    ds = types.SimpleNamespace(x_edges=np.zeros(320), y_edges=np.zeros(320), pixels_per_meter=4, min_x=-10, max_x=70, min_y=-40, max_y=40)
    # (no centre exactly between two pixels: both would be maxima of the same height, and lav_extract_peaks keeps both)
    pixels = np.array([(100.3, 100.0), (130.0, 100.45), (100.0, 130.25), (200.4, 200.4), (250.0, 60.75)])
    typs = np.array([1, 1, 0, 0, 1])
    raw = -(pixels - np.array([160.0, 280.0])) / 4.0                    # the recorded frame; the loaders return its negative
    heat, size, ori = LiDARDataset.detections_to_heatmap(ds, raw, np.zeros(5), np.full((5, 2), 2.0), typs)
    rows = ops.extract_peaks(heat.to(DEV), size.to(DEV), ori.to(DEV), max_det=20)
    host = rows.cpu().numpy()
    assert ((host[..., 0] >= np.exp(-0.5)).sum(axis=1) == (2, 3)).all() and (host[..., 0] > 0.1).sum() == 5
    f = U.blank(320, 320, G=5, centre=(160.0, 280.0))
    f["locs"][:] = np.repeat((-raw).astype(np.float32)[:, None], U.T + 1, axis=1)
    f["typs"][:], f["n"] = typs, 5
    args = on_device(f)
    args[3] = rows
    acc = ops.eval_frame(torch.zeros(len(E.ACC), dtype=torch.int64, device=DEV), *args, **f["kw"]).cpu().numpy()
    np.testing.assert_array_equal(acc, E.eval_frame_numpy(E.ACC.zeros(), *[host if i == 3 else a for i, a in enumerate(U.positional(f))], **f["kw"]))
    det = E.summarise(acc)["det"]
    assert [(d["tp"], d["fp"], d["fn"]) for d in det] == [(2, 0, 0), (3, 0, 0)]


def test_bad_arguments_raise_before_any_launch():
    f = U.scene_others(7)
    acc = torch.zeros(len(E.ACC), dtype=torch.int64, device=DEV)

    def call(**changed):
        g = dict(zip(U.ARGS, on_device(f)))
        g.update(changed)
        return ops.eval_frame(acc, *[g[k] for k in U.ARGS], **f["kw"])

    with pytest.raises(ValueError, match="rows per class"):
        call(rows=torch.zeros((2, 33, 7), device=DEV))
    with pytest.raises(ValueError, match="bev"):
        call(bev=torch.zeros((4, U.H, U.W), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="HBM"):
        call(locs=torch.from_numpy(f["locs"]))
    with pytest.raises(ValueError, match="forecasts"):
        call(other_row=torch.zeros(8, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.eval_frame(acc[:-1], *on_device(f), **f["kw"])
    assert int(acc.sum()) == 0
    # no forecasts: the CPU zeros UniPlanner.infer_all returns then are taken for what they are
    call(other_cast=torch.zeros((0, 6, U.T, 2)), other_cmds=torch.zeros((0, 6)), other_row=torch.zeros(0, dtype=torch.int32))
    assert int(acc[0]) == 1


def test_evaluator_adds_the_same_counters_on_the_device_and_on_the_host():
    """Evaluator over (lidar_model, uniplanner): the accumulator in HBM (the kernel) and on the host (the specification, on copies of
    the frame's tensors) end equal over a two-frame synthetic batch."""
    from lav_amd.train.synthetic import synthetic_lidar_batch
    from tests.util import build_models
    lm, up = build_models(DEV)
    batch = synthetic_lidar_batch(2, seed=5, max_points=20000)
    on_gpu, on_host = E.Evaluator((lm, up)), E.Evaluator((lm, up), device="cpu")
    assert on_gpu.run([batch]) == on_host.run([batch]) == 2
    assert on_gpu.acc.is_cuda and not on_host.acc.is_cuda
    np.testing.assert_array_equal(on_gpu.counters(), on_host.counters())
    assert E.summarise(on_gpu.counters())["frames"] == 2 and on_gpu.run([batch], max_frames=3) == 3


@pytest.fixture(scope="module")
def seeded_checkpoints(tmp_path_factory):
    from lav_amd.train import LAV, TrainConfig
    root = tmp_path_factory.mktemp("eval_ck")
    seeded = LAV(TrainConfig(), torch.device("cpu"), what="lidar")
    for k, sd in dict(bev=seeded.bev_planner.state_dict(), lidar=seeded.state_dict("lidar"), uniplanner=seeded.state_dict("uniplanner")).items():
        torch.save(sd, root / f"{k}_seed.th")
    return root


def test_command_line_on_recorded_routes(tmp_path, seeded_checkpoints, monkeypatch, capsys):
    """eval_full_v2 over a 3-frame synthetic route with saved seeded checkpoints: the JSON's counters are the specification's on what
    the kernel was handed (captured on the way in), a second run prints the same counters, a missing checkpoint is an error."""
    from tests.util import dataset_fixture_config
    cfg = dataset_fixture_config(str(tmp_path), routes=1, frames=23)
    ck = seeded_checkpoints
    base = ["--config-path", cfg, "--num-workers", "0", "--precision", "f16x3", "--bev", str(ck / "bev_seed.th"), "--uniplanner", str(ck / "uniplanner_seed.th")]
    with pytest.raises(SystemExit) as e:
        E.main(base)
    assert e.value.code not in (0, None) and "lidar_model_dir" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        E.main(base + ["--lidar", str(tmp_path / "absent.th")])
    assert e.value.code not in (0, None) and "lidar_model_dir" in str(e.value.code)

    seen, real = [], ops.eval_frame

    def spy(acc, *args, **kw):
        seen.append(([a.detach().cpu().numpy().copy() if torch.is_tensor(a) else a for a in args], dict(kw)))
        return real(acc, *args, **kw)

    monkeypatch.setattr(ops, "eval_frame", spy)
    capsys.readouterr()
    out_file = tmp_path / "eval.json"
    lines = E.main(base + ["--lidar", str(ck / "lidar_seed.th"), "--out", str(out_file)])
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == len(printed) == 1 and printed[0] == json.loads(json.dumps(lines[0])) == json.loads(out_file.read_text())
    assert len(seen) == 3 and printed[0]["summary"]["frames"] == 3 and printed[0]["precision"] == "f16x3"
    want = E.ACC.zeros()
    for args, kw in seen:
        assert args[0].shape == (3, 320, 320) and args[1].dtype == np.uint8 and args[3].shape == (2, 20, 7)
        E.eval_frame_numpy(want, *args, **kw)
    assert printed[0]["counters"] == E.ACC.named(want)
    assert printed[0]["counters"]["frames"] == 3 and sum(printed[0]["counters"]["n_gt"]) > 0
    again = E.main(base + ["--lidar", str(ck / "lidar_seed.th")])
    assert again[0]["counters"] == printed[0]["counters"]


def test_command_line_synthetic_at_every_precision(capsys):
    """--precision all: three summaries of the same frames.  What does not depend on the arithmetic - frames, ground-truth counts, the
    labelled pixels per channel - is identical; how the predictions differ is what the tool is there to measure, nothing is asserted."""
    lines = E.main(["--synthetic", "--frames", "2", "--precision", "all", "--max-points", "20000"])
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["precision"] for l in printed] == ["f16x3", "bf16x6", "f32"] and len(lines) == 3
    for l in printed:
        assert l["summary"]["frames"] == 2
        assert [d["n_gt"] for d in l["summary"]["det"]] == [d["n_gt"] for d in printed[0]["summary"]["det"]]
        assert l["summary"]["seg"]["labelled"] == printed[0]["summary"]["seg"]["labelled"]
    assert sum(printed[0]["summary"]["seg"]["labelled"]) > 0
