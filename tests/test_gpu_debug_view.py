"""lav_debug_view (csrc/debug_view.hip, ops.debug_view) on the GPU against the specification lav_amd.agent.debug_view: every
comparison is exact.  Small geometries (tests/debug_view_util.py says why they need no enlarging for the kernel's 32 x 16 tiles) with
every scene - no vehicles, 15 vehicles, all dots on one spot (the tile's culled list overflows and the global list is walked),
records straddling and outside the panel, overlapping kinds -, the agent's own geometry, repeatability and the zeroed workspace,
refused arguments, and the agent with the view on (graphs and eager) and off."""
import os

import numpy as np
import pytest
import torch
import yaml

from lav_amd import ops, synth
from lav_amd.agent import RoadOption
from lav_amd.agent import debug_view as V
from tests.debug_view_util import AGENT_GRID, CMD_THRESH, FRAMES, GEOMETRIES, SCENES, cloud, controls, images, pred_bev, scene

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def render(rgb, tel, pts, bev, prims, text, grid):
    return ops.debug_view(dev(rgb), dev(tel), dev(pts), dev(bev), prims, text, grid=grid).cpu().numpy()


def records(kind, grid, ego, seed=3):
    plan, locs, cmds, det, tgt = scene(kind, grid, ego, seed)
    cmd, spd, steer, throt, brake, bra = controls(seed)
    return V.primitives(plan, locs, cmds, det, tgt, ppm=grid[4], cmd_thresh=CMD_THRESH, ego=ego), V.text_rows(cmd, spd, steer, throt, brake, bra)


@pytest.fixture(scope="module")
def inputs():
    """Per geometry: images, cloud and BEV, made once and left unchanged."""
    return {name: (*images(rs, ts), cloud(grid), pred_bev(grid)) for name, (grid, rs, ts, _) in GEOMETRIES.items()}


@pytest.mark.parametrize("kind", SCENES)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_kernel_equals_specification_on_small_geometries(inputs, name, kind):
    grid, _, _, ego = GEOMETRIES[name]
    rgb, tel, pts, bev = inputs[name]
    prims, text = records(kind, grid, ego)
    got = render(rgb, tel, pts, bev, prims, text, grid)
    assert got.shape == (*FRAMES[name][:2], 3)
    np.testing.assert_array_equal(got, V.compose_numpy(rgb, tel, pts, bev, prims, text, grid=grid))
    if kind == "pile":       # more records on one tile's footprint than its list of 512 holds
        spot = prims["p0"][100]
        assert (np.abs(prims["p0"] - spot).max(axis=1) <= 8).sum() > 1024


def test_kernel_equals_specification_at_the_agent_geometry():
    rgb, tel = images((288, 768, 3), (192, 480, 3), seed=5)
    pts = cloud(AGENT_GRID, n=196608 - 1500, seed=6)
    pts = np.concatenate([pts, np.full((196608 - len(pts), 11), np.nan, np.float32)])          # the graphed pipeline's absent rows
    assert pts.shape == (196608, 11)
    bev = pred_bev(AGENT_GRID, seed=7)
    prims, text = records("full", AGENT_GRID, (160, 280), seed=8)
    got = render(rgb, tel, pts, bev, prims, text, AGENT_GRID)
    assert got.shape == (160, 1146, 3)
    np.testing.assert_array_equal(got, V.compose_numpy(rgb, tel, pts, bev, prims, text, grid=AGENT_GRID))


def test_same_call_twice_and_the_workspace_is_zeroed(inputs):
    grid, _, _, ego = GEOMETRIES["odd"]
    rgb, tel, pts, bev = inputs["odd"]
    prims, text = records("overlap", grid, ego)
    a, b = render(rgb, tel, pts, bev, prims, text, grid), render(rgb, tel, pts, bev, prims, text, grid)
    assert a.tobytes() == b.tobytes()
    none, text = prims[:0], np.zeros_like(text)                      # (no text: at this size the lines would cross the LiDAR panel)
    lay = V.layout(rgb.shape, tel.shape, grid, bev.shape)
    for empty in (np.zeros((0, 11), np.float32), np.full((64, 11), np.nan, np.float32)):
        got = render(rgb, tel, empty, bev, none, text, grid)
        np.testing.assert_array_equal(got, V.compose_numpy(rgb, tel, empty, bev, none, text, grid=grid))
        # the LiDAR panel is empty: black wherever a frame pixel reads only that panel and no text lies
        inner = got[lay["frame_h"] // 2:, (lay["x_lidar"] + 3) // 2 + 1:lay["x_bev"] // 2 - 1]
        assert inner.size > 0 and not inner.any()
    assert render(rgb, tel, pts, bev, none, text, grid)[lay["frame_h"] // 2:, (lay["x_lidar"] + 3) // 2 + 1:lay["x_bev"] // 2 - 1].any()


def test_ops_debug_view_refuses_wrong_arguments(inputs):
    grid, _, _, ego = GEOMETRIES["even"]
    rgb, tel, pts, bev = (dev(a) for a in inputs["even"])
    prims, text = records("empty", grid, ego)
    ok = dict(rgb=rgb, tel_rgb=tel, lidar=pts, pred_bev=bev, prims=prims, text=text)
    bad = [dict(rgb=rgb.float()), dict(rgb=rgb.permute(2, 0, 1)), dict(rgb=rgb[..., 0]), dict(rgb=rgb.cpu()), dict(tel_rgb=tel.to(torch.int8)),
           dict(tel_rgb=tel[..., :2]), dict(lidar=pts.double()), dict(lidar=pts[:, 0]), dict(lidar=pts[:, :1]), dict(pred_bev=bev.half()),
           dict(pred_bev=bev[:2]), dict(pred_bev=bev[:, :-1]), dict(pred_bev=bev[0]), dict(prims=prims.view(np.uint8)), dict(prims=np.zeros(4, np.int32)),
           dict(text=text[:3]), dict(text=text.astype(np.int32)), dict(text=text[:, :10])]
    for change in bad:
        with pytest.raises(ValueError):
            ops.debug_view(**{**ok, **change}, grid=grid)
    for g in ((-2, 10, -6, 6), (-2, -2, -6, 6, 4), (-2, 10, -6, 6, 0.3)):
        with pytest.raises(ValueError):
            ops.debug_view(**ok, grid=g)
    with pytest.raises(ValueError):
        ops.debug_view(**ok, grid=grid, out=torch.empty((24, 164, 4), dtype=torch.uint8, device="cuda"))
    wild = prims.copy()
    wild["p0"][0] = (1 << 21, 0)
    with pytest.raises(ValueError):
        ops.debug_view(**{**ok, "prims": wild}, grid=grid)
    out = torch.empty((24, 164, 3), dtype=torch.uint8, device="cuda")
    assert ops.debug_view(**ok, grid=grid, out=out) is out


# ---------------------------------------------------------------------------------------------- the agent
def _agent(tmp_path, tag, **over):
    from lav_amd.lav_agent import LAVAgent
    cfg = dict(dict(synthetic_weights=True, points_per_tick=8192, precapture=False), **over)
    p = tmp_path / f"cfg_{tag}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    agent = LAVAgent(str(p))
    sc = synth.agent_scenario()
    agent.set_global_plan([({"lat": la, "lon": lo, "z": 0.0}, RoadOption(int(c))) for la, lo, c in zip(sc["lat"], sc["lon"], sc["cmds"])])
    return agent, sc


@pytest.mark.parametrize("hip_graphs", [True, False])
def test_agent_records_the_specified_frames_and_drives_the_same(tmp_path, hip_graphs):
    out_dir = tmp_path / "views"
    a, sc = _agent(tmp_path, "on", hip_graphs=hip_graphs, debug_view=True, debug_view_flush=4, debug_view_dir=str(out_dir))
    b, _ = _agent(tmp_path, "off", hip_graphs=hip_graphs)
    seen = []
    real = a.visualize
    a.visualize = lambda *args: (seen.append(args), real(*args))[1]
    grid = (a.min_x, a.max_x, a.min_y, a.max_y, a.pixels_per_meter)
    ticks = 7                                      # tick 0 only stashes its sweep: six frames, one file of four and two left for destroy()
    for i in range(ticks):
        data = synth.agent_inputs(i, sc)
        ca, cb = a.run_step(data, i * 0.05), b.run_step(synth.agent_inputs(i, sc), i * 0.05)
        assert (ca.steer, ca.throttle, ca.brake) == (cb.steer, cb.throttle, cb.brake), i
        assert len(b.vizs) == 0
        if i == 0:
            assert len(a.vizs) == 0 and not seen
            continue
        assert len(seen) == i and len(a.vizs) == (i % 4) and len(a.vizs.written) == i // 4
        if len(a.vizs):
            frame = a.vizs.frames()[-1].copy()
        else:
            saved = np.load(a.vizs.written[-1])
            assert saved.shape == (4, 160, 1146, 3) and saved.dtype == np.uint8 and os.path.basename(a.vizs.written[-1]) == f"view_{i - 2:06d}.npy"
            frame = saved[-1]
        # the specification from the pipeline's outputs and the tick's inputs
        _, _, _, pred_bra, _, pred_loc, cast_locs, cast_cmds, det, tgt, cmd, spd, steer, throt, brake = seen[-1]
        o = a.last_outputs
        assert (steer, throt, brake) == (ca.steer, ca.throttle, ca.brake) and pred_bra == float(o["pred_bra"]) and det is o["det"]
        np.testing.assert_array_equal(cast_locs, o["other_cast_locs"].cpu().numpy())
        np.testing.assert_array_equal(pred_loc, o["ego_cast_locs" if cmd in (4, 5) else "ego_plan_locs"].cpu().numpy())
        np.testing.assert_array_equal(np.float32(tgt), a.pipeline.b_nxp.cpu().numpy() if hip_graphs else np.float32(tgt))
        rgb = np.concatenate([data[f"RGB_{k}"][1][..., :3][..., ::-1] for k in range(3)], axis=1)
        tel = data["TEL_RGB"][1][..., :3][..., ::-1][:-a.crop_tel_bottom]
        want = V.debug_view_numpy(rgb, tel, o["lidar_points"].cpu().numpy(), pred_bra, torch.sigmoid(o["pred_bev"][0]).cpu().numpy(), pred_loc,
                                  cast_locs, cast_cmds, det, tgt, cmd, spd, steer, throt, brake, grid=grid, cmd_thresh=a.cmd_thresh)
        np.testing.assert_array_equal(frame, want)
    assert sorted(os.listdir(out_dir)) == ["view_000002.npy"]
    a.destroy(); b.destroy()
    assert sorted(os.listdir(out_dir)) == ["view_000002.npy", "view_000006.npy"] and np.load(out_dir / "view_000006.npy").shape == (2, 160, 1146, 3)
    assert len(a.vizs) == 0


def test_agent_with_the_default_config_records_nothing(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    a, sc = _agent(tmp_path, "default")
    assert a.debug_view is False and (a.debug_view_dir, a.debug_view_every, a.debug_view_flush) == ("debug_view", 1, 600)
    for i in range(3):
        a.run_step(synth.agent_inputs(i, sc), i * 0.05)
        assert len(a.vizs) == 0
    assert a.flush_data() is None and a._view_frame is None
    a.destroy()
    assert sorted(os.listdir(tmp_path)) == ["cfg_default.yaml"]
