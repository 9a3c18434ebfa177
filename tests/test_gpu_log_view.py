"""lav_log_view (csrc/log_view.hip, ops.log_view) on the GPU against the specification lav_amd.train.log_view.log_view_numpy: every
comparison is exact.  The mixed frame (tests/log_view_util.py: 75 x 131, neither a multiple of the kernel's 32 x 8 tile, five panels of
the five kinds) with each scene, each trainer's frame once at its real geometry, and train_seg --log-dir end to end."""
import os
import sys

import numpy as np
import pytest
import torch

from lav_amd import ops
from lav_amd.train import log_view as V
from tests.log_view_util import FRAME_HW, LIST, SCENES, decode_png, mixed_panels, mixed_scene, mixed_sources, seeded_view

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def both(panels, prims, text, sources, size=None):
    want = V.log_view_numpy(panels, prims, text, sources, size=size)
    got = ops.log_view(panels, prims, text, [dev(s) for s in sources], size=size).cpu().numpy()
    return got, want


@pytest.mark.parametrize("scene", SCENES)
def test_mixed_frame_equals_specification(scene):
    prims, text = mixed_scene(scene)
    if scene == "overflow":
        assert len(prims) > LIST + 37
    if scene == "empty":
        assert len(prims) == 0 and len(text) == 0
    got, want = both(mixed_panels(), prims, text, mixed_sources(), size=FRAME_HW)
    np.testing.assert_array_equal(got, want)


def test_constant_planes_and_label_widths():
    got, want = both(mixed_panels(), *mixed_scene("empty"), mixed_sources(constant_planes=True), size=FRAME_HW)
    np.testing.assert_array_equal(got, want)
    assert not want[38:, :53].any()
    for dtype in (np.uint8, np.int32):          # (int64 is the mixed frame's)
        src = mixed_sources()
        src[3] = np.clip(src[3], 0, 6).astype(dtype)
        got, want = both(mixed_panels(), *mixed_scene("straddle"), src, size=FRAME_HW)
        np.testing.assert_array_equal(got, want)


def test_frame_without_panels_and_wrong_arguments():
    p = V._Prims()
    p.dot(0, (3, 3), 2, (1, 2, 3))
    none = V.panel_table([])
    out = ops.log_view(none, V._Prims().table(), V.text_table([(1, 8, "ab")]), [], size=(9, 40), out=torch.empty((9, 40, 3), dtype=torch.uint8, device="cuda"))
    np.testing.assert_array_equal(out.cpu().numpy(), V.log_view_numpy(none, V._Prims().table(), V.text_table([(1, 8, "ab")]), [], size=(9, 40)))
    src = mixed_sources()
    for bad in (dict(sources=src), dict(sources=[dev(s) for s in src[:3]]), dict(prims=p.table()[["kind", "p0"]]),
                dict(sources=[dev(src[0]), dev(src[1]).double(), dev(src[2]), dev(src[3])])):
        args = dict(panels=mixed_panels(), prims=p.table(), text=V.text_table([]), sources=[dev(s) for s in src])
        args.update(bad)
        with pytest.raises(ValueError):
            ops.log_view(args["panels"], args["prims"], args["text"], args["sources"], size=FRAME_HW)


@pytest.mark.parametrize("what,ndet", [("bev", 0), ("lidar", 0), ("lidar", 7), ("seg", 0), ("bra", 0)])
def test_trainer_frames_at_their_real_geometry(what, ndet):
    view = seeded_view(what, ndet)
    frame = V.build_frame(what, view)
    on_device = frame._replace(sources=[dev(s) for s in frame.sources])
    got = V.render(on_device)
    assert got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(), V.render(frame))


def test_train_seg_log_dir_end_to_end(tmp_path, monkeypatch):
    """Two steps of train_seg.py --log-dir on the device write two PNG files; the second decodes to the frame the specification
    renders from that step's own tensors (the view the trainer returned, copied to the host as the frame is built)."""
    from lav_amd.train import run
    seen = []
    build = V.build_frame

    def capture(what, view, cfg=None):
        frame = build(what, view, cfg)
        assert all(s.is_cuda for s in frame.sources)
        seen.append(frame._replace(sources=[s.detach().cpu().numpy().copy() for s in frame.sources]))
        return frame

    monkeypatch.setattr(run.log_view, "build_frame", capture)
    d = tmp_path / "viz"
    monkeypatch.setattr(sys, "argv", ["train_seg.py", "--synthetic", "--batch-size", "2", "--num-epoch", "1", "--steps-per-epoch", "2", "--num-per-log", "1",
                                      "--log-dir", str(d), "--save-dir", str(tmp_path / "ck"), "--config-path", str(tmp_path / "none.yaml")])
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    run.main("seg")
    assert sorted(os.listdir(d)) == ["seg_0000000.png", "seg_0000001.png"] and len(seen) == 2
    for name, frame in zip(sorted(os.listdir(d)), seen):
        img = decode_png(open(d / name, "rb").read())
        assert img.shape == (288, 768, 3)
        np.testing.assert_array_equal(img, V.render(frame))
    assert (V.render(seen[0]) != V.render(seen[1])).any()


def test_train_lidar_keys_without_and_with_the_view():
    from lav_amd.train import LAV, TrainConfig, synthetic_lidar_batch
    torch.manual_seed(0)
    lav = LAV(TrainConfig(log_every=1), torch.device("cuda"), what="lidar")
    batch = synthetic_lidar_batch(1, seed=41, max_points=6000, num_objs=2, device="cuda")
    today = {"loss", "hm_loss", "box_loss", "ori_loss", "seg_loss", "plan_loss", "ego_cast_loss", "other_cast_loss", "cmd_loss", "ego_plan_locs", "num_det"}
    assert set(lav.train_lidar(*batch)) == today
    lav.log_view = True
    info = lav.train_lidar(*batch)
    assert set(info) == today | {"view"}
    view = info["view"]
    assert set(view) == {"det", "gt_det", "pred_bev", "bev", "other_next_locs", "other_cast_locs", "other_cast_cmds", "ego_plan_locs", "ego_next_locs", "nxp", "cmd"}
    assert view["bev"].is_cuda and view["pred_bev"].is_cuda and tuple(view["pred_bev"].shape) == (3, 320, 320)
    assert len(view["gt_det"]) == 2 and sum(len(d) for d in view["gt_det"]) > 0 and view["other_cast_locs"].shape[1:] == (6, 20, 2)
    frame = V.build_frame("lidar", view)
    host = frame._replace(sources=[s.cpu().numpy() for s in frame.sources])
    np.testing.assert_array_equal(V.render(frame).cpu().numpy(), V.render(host))
