"""CPU checks of the offline point painter (lav_amd/data/paint.py, data_paint.py, lmdb_ro.update): the route rewrite, the
painter's dataset against the reference's (tests/golden/data_paint.npz, made by tests/golden/make_golden_paint.py), the
orchestration with injected stages, the CPU painting reference against the reference's own, the CLI.  No GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from lav_amd.data import lmdb_ro
from lav_amd.data.datasets import LiDARPaintedDataset, paint_from_cameras, read_array
from tests import paint_util
from tests.util import crc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pairs(path):
    env = lmdb_ro.open(path)
    try:
        return dict(env.begin().items()), env.stat()
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------- lmdb_ro.update
def test_update_adds_and_replaces_keys_of_a_deep_route_with_overflow_values(tmp_path):
    r = np.random.default_rng(5)
    items = {f"key_{i:05d}".encode(): r.integers(0, 256, int(r.integers(1, 300)), dtype=np.uint8).tobytes() for i in range(3000)}
    for i in range(0, 3000, 97):                                     # overflow values: several pages each
        items[f"key_{i:05d}".encode()] = r.integers(0, 256, int(r.integers(5000, 30000)), dtype=np.uint8).tobytes()
    path = str(tmp_path / "route")
    lmdb_ro.write(path, items.items())
    _, st = pairs(path)
    assert st["depth"] >= 2 and st["entries"] == 3000
    new = {b"key_00007": b"small now", b"key_00097": b"x" * 20000, b"key_00100": b"", b"aaa_first": b"before every key",
           b"key_01500_mid": b"y" * 9000, b"zzz_last": b"after every key", b"key_00194": b"was an overflow value"}
    lmdb_ro.update(path, new.items())
    got, st = pairs(path)
    want = dict(items)
    want.update(new)
    assert st["entries"] == len(want) == 3003 and st["depth"] >= 2
    assert got == want                                               # untouched pairs byte-identical, new values read back
    assert sorted(os.listdir(path)) == ["data.mdb"]                  # no temporary file is left
    env = lmdb_ro.open(path)
    txn = env.begin()
    assert all(txn.get(k) == v for k, v in want.items()) and txn.get(b"key_99999") is None
    assert list(k for k, _ in txn.items()) == sorted(want)
    env.close()
    # update with no items reproduces the pair set - and, being this writer's own layout, the file
    before = open(os.path.join(path, "data.mdb"), "rb").read()
    lmdb_ro.update(path, [])
    assert pairs(path)[0] == want and open(os.path.join(path, "data.mdb"), "rb").read() == before
    # ... which is the file write() gives for the same pairs
    lmdb_ro.write(str(tmp_path / "fresh"), want.items())
    assert open(os.path.join(tmp_path / "fresh", "data.mdb"), "rb").read() == before


def test_update_failure_leaves_the_old_route(tmp_path):
    path = str(tmp_path / "route")
    lmdb_ro.write(path, [(b"a", b"1"), (b"b", b"2")])
    before = open(os.path.join(path, "data.mdb"), "rb").read()
    with pytest.raises(lmdb_ro.Error):
        lmdb_ro.update(path, [(b"k" * 600, b"key too long")])
    assert open(os.path.join(path, "data.mdb"), "rb").read() == before and os.listdir(path) == ["data.mdb"]


# ------------------------------------------------------------------------------------------------------- the dataset
def test_point_paint_dataset_equals_the_reference(tmp_path, golden):
    from lav_amd.data.paint import PointPaintDataset
    g = golden["data_paint"]
    ds = PointPaintDataset(paint_util.paint_fixture_config(str(tmp_path)))
    assert len(ds) == int(g["len"]) == 3
    assert [f"{os.path.basename(ds.nam_map[i])}/{ds.idx_map[i]}" for i in range(len(ds))] == list(g["index"])
    for i in range(3):
        lidar, rgbs = ds[i]
        assert lidar.dtype == np.float32 and rgbs.dtype == np.uint8 and list(rgbs.shape) == list(g[f"f{i}/rgbs_shape"]) == [5, 3, 288, 256]
        assert crc(lidar) == int(g[f"f{i}/lidar_crc"]) and np.array_equal(lidar[::16], g[f"f{i}/lidar_s"])
        assert crc(rgbs) == int(g[f"f{i}/rgbs_crc"]) and np.array_equal(rgbs[:, :, ::16, ::16], g[f"f{i}/rgbs_s"])
        lidar2, bgr = ds.raw(i)
        assert np.array_equal(lidar2, lidar) and np.array_equal(bgr[..., ::-1].transpose(0, 3, 1, 2), rgbs)


# ------------------------------------------------------------------------------------------------------- the CPU reference
def test_paint_from_cameras_equals_the_reference_on_five_cameras(tmp_path, golden):
    """Pins the CPU reference the GPU tests compare with (CameraProjection.pixels / paint_from_cameras) to the reference's own
    CoordConverter / point_painting, for 5 cameras: pixels of three frames and the painting of a random probability map."""
    from lav_amd.data.paint import PointPaintDataset, host_paint
    g = golden["data_paint"]
    config_path = paint_util.paint_fixture_config(str(tmp_path))
    cams = paint_util.painter_cameras(yaml.safe_load(open(config_path)))
    ds = PointPaintDataset(config_path)
    for i in range(3):
        lidar, _ = ds[i]
        assert np.array_equal(paint_util.clip32(np.stack([c.pixels(lidar) for c in cams])), g[f"f{i}/lidar_to_cam"])
    lidar, _ = ds[0]
    sems = paint_util.random_probability_maps(seed=int(g["map/seed"]))
    assert crc(sems[0]) == int(g["map/crc"])
    want = g["map/lidar_painted"]
    got = paint_from_cameras(lidar, sems[0][:, 1:] * (1 - sems[0][:, :1]), cams).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (want != 0).any(1).sum() > 2000
    got = host_paint(lidar, np.array([0, len(lidar)], np.int32), sems, cams)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------------- orchestration
def stub_probs(images):
    """A deterministic stand-in for the segmenter: per pixel, a softmax over five mixtures of the pixel's B, G, R - the same
    values whatever batch an image arrives in."""
    x = images.astype(np.float32)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    logits = np.stack([b, g, r, (b + g) * np.float32(0.5), np.float32(255) - r], axis=1) * np.float32(1 / 64)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def painted_sets(tmp_path_factory):
    """Two ragged routes (500- and 700-point sweeps, num_plan 4 -> 3 indexed frames each) painted through paint_dataset with the
    stub stages at frames_per_batch 1 and 4; `plain` is the unpainted copy."""
    from lav_amd.data.paint import PointPainter, host_paint, paint_dataset
    root = tmp_path_factory.mktemp("paint_orchestration")
    plain = root / "plain"
    plain.mkdir()
    paint_util.paint_fixture_config(str(plain), routes=2, points=[500, 700], num_plan=4, angle_jitter=0)
    out = {"plain": str(plain)}
    for fpb in (1, 4):
        d = root / f"fpb{fpb}"
        shutil.copytree(plain / "data", d / "data")
        cfg = yaml.safe_load(open(plain / "config.yaml"))
        cfg["data_dir"] = str(d / "data")
        with open(d / "config.yaml", "w") as f:
            yaml.safe_dump(cfg, f)
        cams = paint_util.painter_cameras(cfg)
        painter = PointPainter(str(d / "config.yaml"), "cpu", probs=stub_probs, paint=lambda lidar, offsets, sem: host_paint(lidar, offsets, sem, cams))
        calls = []
        inner = painter.paint
        painter.paint = lambda lidars, images: (calls.append(len(lidars)), inner(lidars, images))[1]
        stats = paint_dataset(str(d / "config.yaml"), "cpu", frames_per_batch=fpb, num_workers=0, num_per_log=2, painter=painter, log=lambda m: None)
        assert stats["frames"] == 6 and stats["routes"] == 2
        assert calls == ([1] * 6 if fpb == 1 else [4, 2])           # a batch of 4 holds the route boundary: 3 x 500 + 1 x 700 points
        out[fpb] = str(d)
    return out


def test_paint_dataset_writes_the_direct_per_frame_painting(painted_sets):
    from lav_amd.data.paint import PointPaintDataset
    plain = PointPaintDataset(os.path.join(painted_sets["plain"], "config.yaml"))
    cams = paint_util.painter_cameras(yaml.safe_load(open(os.path.join(painted_sets["plain"], "config.yaml"))))
    assert len(plain) == 6
    direct = {}
    for i in range(len(plain)):
        lidar, bgr = plain.raw(i)
        sems = stub_probs(bgr)
        val = paint_from_cameras(lidar, sems[:, 1:] * (1 - sems[:, :1]), cams).astype(np.float32)
        assert (val != 0).any(1).sum() > len(lidar) // 3
        direct[(os.path.basename(plain.nam_map[i]), f"lidar_sem_{plain.idx_map[i]:05d}".encode())] = val.tobytes()
    results = {}
    for fpb in (1, 4):
        for route in ("route_000", "route_001"):
            old, old_st = pairs(os.path.join(painted_sets["plain"], "data", route))
            new, new_st = pairs(os.path.join(painted_sets[fpb], "data", route))
            assert sorted(os.listdir(os.path.join(painted_sets[fpb], "data", route))) == ["data.mdb"]
            assert sorted(new) == sorted(old) and new_st["entries"] == old_st["entries"]
            painted = {k for (rt, k) in direct if rt == route}
            assert len(painted) == 3
            for k in old:
                if k in painted:
                    assert new[k] == direct[(route, k)] and new[k] != old[k], (route, k)
                else:                               # the unindexed last num_plan frames' lidar_sem_ and every other key
                    assert new[k] == old[k], (route, k)
            assert sum(k.startswith(b"lidar_sem_") for k in old) == 7
            results[(fpb, route)] = new
    assert results[(1, "route_000")] == results[(4, "route_000")] and results[(1, "route_001")] == results[(4, "route_001")]


def test_lidar_painted_dataset_reads_the_painted_values(painted_sets):
    """angle_jitter 0: a 'lidar_painted' sample's rows are a permutation of the sweep (minus the ego's body) with the written
    scores masked to the three middle cameras' fields of view."""
    config_path = os.path.join(painted_sets[4], "config.yaml")
    ds = LiDARPaintedDataset(config_path)
    for idx in (0, 4):
        txn, t = ds.txn_map[idx], ds.idx_map[idx]
        xyzr, sem = ds.drop_ego_points(read_array(txn, "lidar", t).reshape(-1, 4), read_array(txn, "lidar_sem", t).reshape(-1, 4))
        want = np.concatenate([xyzr, sem * paint_from_cameras(xyzr, ds.all_visible, ds.cameras)], axis=1).astype(np.float32)
        torch.manual_seed(idx)
        np.random.seed(idx)
        lidar, num_points = ds[idx][:2]
        assert num_points == len(want)
        got = lidar[:num_points]
        order = lambda a: a[np.lexsort(a[:, :3].T[::-1])]
        assert np.array_equal(order(got), order(want)) and (got[:, 4:] != 0).any(1).sum() > num_points // 5


# ------------------------------------------------------------------------------------------------------- CLI
def test_cli_help_parses_and_cpu_is_refused():
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "data_paint.py"), "--help"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    for flag in ("--config-path", "--device", "--num-per-log", "--num-workers", "--frames-per-batch"):
        assert flag in r.stdout
    assert "decode" in r.stdout and "Ray" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(REPO, "data_paint.py"), "--device", "cpu"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "no CPU path" in r.stderr
