"""The offline point painter on the MI355X: lav_paint_frames and lav_image_u8_to_f32 against the CPU restatement of the
reference (CameraProjection.pixels / paint_from_cameras, pinned to the reference's own modules by tests/test_data_paint_host.py)
and against the reference's recorded results (tests/golden/data_paint.npz), and paint_dataset end to end.

THE EXCLUSION RULE of the bit-for-bit comparisons: a point is left out when, in the CPU reference's float64 values before
truncation, any of u, v, z of any camera lies within 1e-9 of an integer while inside [-1, max(h, w) + 1] - only there can a
last-bit difference between the host BLAS (which may fuse multiply-adds) and the kernel (which never does) move a pixel.  Every
comparison first asserts that the rule leaves out at most 1e-5 of the points it is applied to."""
import ast
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from lav_amd import ops, synth
from lav_amd.data import lmdb_ro
from lav_amd.data.datasets import paint_from_cameras
from tests import paint_util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sweep(r, points):
    """A sweep drawn like lav_amd.data.synthetic_route's."""
    rad, az = r.uniform(2.5, 45, points), r.uniform(-np.pi, np.pi, points)
    return np.stack([rad * np.cos(az), rad * np.sin(az), r.normal(-2.2, 0.15, points), r.uniform(0, 1, points)], 1).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_paint(lidars, sem, cams, want_uvz=True):
    offsets = np.zeros(len(lidars) + 1, np.int32)
    offsets[1:] = np.cumsum([len(l) for l in lidars])
    out = ops.paint_frames(torch.from_numpy(np.concatenate(lidars)).to(DEV), torch.from_numpy(offsets).to(DEV), torch.from_numpy(sem).to(DEV),
                           ops.make_cameras_f64(cams), want_uvz=want_uvz)
    torch.cuda.synchronize()
    return (out[0].cpu().numpy(), out[1].cpu().numpy(), offsets) if want_uvz else (out.cpu().numpy(), offsets)


def test_paint_frames_kernel_equals_the_cpu_reference_bit_for_bit():
    """4 ragged frames of 0, 1, 3 999 and 40 000 points, 5 cameras, random probability maps.  The 3 999-point frame ends in six
    hand-placed points - +-1e30 on each axis pattern, NaN, the camera origin - which are NEVER excluded (stricter than the rule:
    the camera origin projects to exactly (0, 0, 0) through the yaw-0 camera, which the rule would leave out by construction);
    the rule and its 1e-5 condition apply to the 43 994 drawn points."""
    with open(os.path.join(paint_util.GOLD, "dataset_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cams = paint_util.painter_cameras(cfg)
    r = np.random.default_rng(2024)
    special = np.array([[1e30, 1e30, 1e30, 0.5], [-1e30, 1e30, -1e30, 0.5], [1e30, 0, 0, 0.5], [-1e30, -1e30, 0, 0.5],
                        [np.nan, 1.0, -2.0, 0.5], [cfg["camera_x"], 0.0, 0.0, 0.5]], np.float32)
    mid = sweep(r, 3999)
    mid[-len(special):] = special
    lidars = [sweep(r, 0), sweep(r, 1), mid, sweep(r, 40000)]
    sem = paint_util.random_probability_maps(frames=4, seed=31)
    painted, uvz, offsets = gpu_paint(lidars, sem, cams)
    lidar = np.concatenate(lidars)
    drawn = np.ones(len(lidar), bool)
    drawn[offsets[3] - len(special):offsets[3]] = False
    excluded = paint_util.excluded_points(cams, lidar) & drawn
    print(f"paint_frames kernel: {excluded.sum()} of {drawn.sum()} drawn points excluded")
    assert excluded.sum() <= 1e-5 * drawn.sum()
    keep = ~excluded
    with np.errstate(all="ignore"):
        want_uvz = paint_util.clip32(np.stack([c.pixels(lidar) for c in cams]))
        want = np.concatenate([paint_from_cameras(lidars[f], sem[f][:, 1:] * (1 - sem[f][:, :1]), cams) for f in range(4)]).astype(np.float32)
    assert uvz.shape == want_uvz.shape == (5, 44000, 3) and painted.shape == want.shape == (44000, 4)
    bad = (uvz != want_uvz).any(axis=(0, 2)) & keep
    print(f"paint_frames kernel: {bad.sum()} points with a different pixel; {(want != 0).any(1).sum()} painted rows")
    assert not bad.any(), (np.nonzero(bad)[0][:5], uvz[:, bad][:, :5], want_uvz[:, bad][:, :5])
    diff = (bits(painted) != bits(want)).any(axis=1) & keep
    assert not diff.any(), (np.nonzero(diff)[0][:5], painted[diff][:5], want[diff][:5])
    assert (want != 0).any(1).sum() > 20000 and (want_uvz[:, ~drawn] == np.iinfo(np.int32).min).any()
    # the frames' maps differ: a point painted from another frame's maps would not compare equal
    assert not np.array_equal(sem[2], sem[3])


def test_paint_frames_reproduces_the_reference_recorded_painting(tmp_path, golden):
    """The fixture's random probability map on the fixture route's first sweep: the reference's own point_painting result."""
    from lav_amd.data.paint import PointPaintDataset
    g = golden["data_paint"]
    config_path = paint_util.paint_fixture_config(str(tmp_path))
    cams = paint_util.painter_cameras(yaml.safe_load(open(config_path)))
    lidar, _ = PointPaintDataset(config_path)[0]
    sem = paint_util.random_probability_maps(seed=int(g["map/seed"]))
    painted, uvz, _ = gpu_paint([lidar], sem, cams)
    excluded = paint_util.excluded_points(cams, lidar)
    print(f"fixture map: {excluded.sum()} of {len(lidar)} points excluded")
    assert excluded.sum() <= 1e-5 * len(lidar)
    keep = ~excluded
    assert np.array_equal(uvz[:, keep], g["f0/lidar_to_cam"][:, keep])
    assert np.array_equal(bits(painted)[keep], bits(g["map/lidar_painted"])[keep])


def test_paint_frames_refuses_what_it_does_not_take():
    cams = paint_util.painter_cameras(yaml.safe_load(open(os.path.join(paint_util.GOLD, "dataset_config.yaml"))))
    lidar, off = torch.zeros((4, 4), device=DEV), torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="sem_c"):
        ops.paint_frames(lidar, off, torch.zeros((1, 5, 4, 8, 8), device=DEV), ops.make_cameras_f64(cams))
    with pytest.raises(RuntimeError, match="ncam"):
        ops.paint_frames(lidar, off, torch.zeros((1, 9, 5, 8, 8), device=DEV), ops.make_cameras_f64((cams * 2)[:9]))
    with pytest.raises(RuntimeError, match="offsets"):
        ops.paint_frames(lidar, off.long(), torch.zeros((1, 5, 5, 8, 8), device=DEV), ops.make_cameras_f64(cams))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.paint_frames(lidar.cpu(), off, torch.zeros((1, 5, 5, 8, 8), device=DEV), ops.make_cameras_f64(cams))


@pytest.mark.parametrize("c_src", [3, 4])
@pytest.mark.parametrize("shape", [(5, 288, 256), (2, 7, 9)])
def test_image_u8_to_f32_is_exact(c_src, shape):
    """(2, 7, 9): 63 pixels per image - the kernel's one-pixel-per-thread path."""
    r = np.random.default_rng(c_src)
    img = r.integers(0, 256, shape + (c_src,), dtype=np.uint8)
    for reverse in (False, True):
        got = ops.image_u8_to_f32(torch.from_numpy(img).to(DEV), reverse=reverse).cpu().numpy()
        want = (img[..., :3][..., ::-1] if reverse else img[..., :3]).transpose(0, 3, 1, 2).astype(np.float32)
        assert got.dtype == np.float32 and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------- pipeline
@pytest.fixture(scope="module")
def painted(tmp_path_factory):
    """A fresh synthetic data set of 2 routes (route 0 is the fixture's: 4000-point sweeps; route 1: 3000-point sweeps) painted with
    the seeded segmenter through paint_dataset at frames_per_batch 4 (2 decode processes) and, a copy of it, at 1.  The
    probability maps the model returned during the runs are recorded per frame."""
    from lav_amd.data.paint import PointPaintDataset, PointPainter, paint_dataset
    from lav_amd.rgb import RGBSegmentationModel
    root = tmp_path_factory.mktemp("paint_pipeline")
    plain = root / "plain"
    plain.mkdir()
    seg = RGBSegmentationModel([4, 6, 7, 10])
    torch.save(synth.seeded_state_dict(seg, prefix="seg."), root / "seg_seed.th")
    paint_util.paint_fixture_config(str(plain), routes=2, points=[4000, 3000], seg_model_dir=str(root / "seg_seed.th"))
    out = {"plain": str(plain)}
    for fpb, workers in ((4, 2), (1, 0)):
        d = root / f"fpb{fpb}"
        shutil.copytree(plain / "data", d / "data")
        cfg = yaml.safe_load(open(plain / "config.yaml"))
        cfg["data_dir"] = str(d / "data")
        with open(d / "config.yaml", "w") as f:
            yaml.safe_dump(cfg, f)
        painter = PointPainter(str(d / "config.yaml"), DEV)
        maps, gpu_probs = [], painter._probs
        painter._probs = lambda images: (lambda s: (maps.extend(s.view(-1, 5, *s.shape[1:]).cpu().numpy()), s)[1])(gpu_probs(images))
        stats = paint_dataset(str(d / "config.yaml"), DEV, frames_per_batch=fpb, num_workers=workers, num_per_log=2, painter=painter)
        assert stats["frames"] == 6 and stats["routes"] == 2 and len(maps) == 6
        out[fpb] = dict(root=str(d), maps=maps)
    return out


def written(root, ds, i):
    env = lmdb_ro.open(os.path.join(root, "data", os.path.basename(ds.nam_map[i])))
    try:
        return np.frombuffer(env.begin().get(f"lidar_sem_{ds.idx_map[i]:05d}".encode()), np.float32).reshape(-1, 4)
    finally:
        env.close()


def test_pipeline_writes_the_painting_of_the_models_own_maps(painted):
    """(a) what paint_dataset wrote == paint_from_cameras on the host applied to the probability maps the same GPU model returned
    for those images, bit for bit outside the exclusion rule; (c) frames_per_batch 1 writes the same bits as 4."""
    from lav_amd.data.paint import PointPaintDataset
    ds = PointPaintDataset(os.path.join(painted["plain"], "config.yaml"))
    cams = paint_util.painter_cameras(yaml.safe_load(open(os.path.join(painted["plain"], "config.yaml"))))
    assert len(ds) == 6
    for i in range(6):
        lidar, _ = ds.raw(i)
        excluded = paint_util.excluded_points(cams, lidar)
        assert excluded.sum() <= 1e-5 * len(lidar)
        for fpb in (4, 1):
            sem = painted[fpb]["maps"][i]
            assert sem.shape == (5, 5, 288, 256)
            want = paint_from_cameras(lidar, sem[:, 1:] * (1 - sem[:, :1]), cams).astype(np.float32)
            got = written(painted[fpb]["root"], ds, i)
            assert got.shape == want.shape == (len(lidar), 4) and (want != 0).any(1).sum() > len(lidar) // 3
            assert np.array_equal(bits(got)[~excluded], bits(want)[~excluded]), (i, fpb)
        a, b = written(painted[4]["root"], ds, i), written(painted[1]["root"], ds, i)
        print(f"frame {i}: frames_per_batch 1 vs 4: {(bits(a) != bits(b)).any(1).sum()} differing rows, max |diff| {np.abs(a - b).max():.3e}")
        assert np.array_equal(bits(a), bits(b)), f"frame {i}: frames_per_batch 1 and 4 wrote different bits"
    # the unindexed last num_plan frames keep their records
    old = lmdb_ro.open(os.path.join(painted["plain"], "data", "route_000")).begin()
    new = lmdb_ro.open(os.path.join(painted[4]["root"], "data", "route_000")).begin()
    assert new.get(b"lidar_sem_00003") == old.get(b"lidar_sem_00003") and new.get(b"lidar_sem_00002") != old.get(b"lidar_sem_00002")
    assert int(new.get(b"len")) == 23 and new.get(b"rgb_4_00022") == old.get(b"rgb_4_00022")


def test_pipeline_against_the_reference_painting(painted, golden):
    """(b) against the reference's own PointPainter.step on the fixture route (CPU, float32 torch): the pixels are identical and
    the values within 1e-5 max|logit|.  tests/test_gpu_e2e.py holds softmax(ERFNet) to half that (softmax is 1/2-Lipschitz in the
    max norm of the logits, the logits are held to 1e-5 max|logit|); s_c (1 - s_0) has two factors in [0, 1], so the two errors
    add to at most twice the softmax bar.  max|logit| is rgb.npz's logits_s', or these 15 images' own (recorded in the fixture)
    where that is larger."""
    from lav_amd.data.paint import PointPaintDataset
    g = golden["data_paint"]
    scale = max(float(np.abs(golden["rgb"]["logits_s"]).max()), float(g["logit_absmax"]))
    ds = PointPaintDataset(os.path.join(painted["plain"], "config.yaml"))
    cams = paint_util.painter_cameras(yaml.safe_load(open(os.path.join(painted["plain"], "config.yaml"))))
    for i in range(3):
        assert f"{os.path.basename(ds.nam_map[i])}/{ds.idx_map[i]}" == g["index"][i]
        lidar, _ = ds.raw(i)
        excluded = paint_util.excluded_points(cams, lidar)
        assert excluded.sum() <= 1e-5 * len(lidar)
        _, uvz, _ = gpu_paint([lidar], painted[4]["maps"][i][None], cams)
        assert np.array_equal(uvz[:, ~excluded], g[f"f{i}/lidar_to_cam"][:, ~excluded]), f"frame {i}: pixels differ"
        got, want = written(painted[4]["root"], ds, i), g[f"f{i}/lidar_painted"]
        assert np.array_equal((got != 0).any(1)[~excluded], (want != 0).any(1)[~excluded])
        err = np.abs(got.astype(np.float64) - want)[~excluded].max()
        print(f"frame {i}: max |painted - reference| {err:.3e} (bar {1e-5 * scale:.3e}, max|logit| {scale:.1f})")
        assert err <= 1e-5 * scale


def test_train_full_runs_a_step_on_the_painted_routes(painted, tmp_path):
    """train_full_v2.py over the painted set: one epoch (6 frames, batch 2) with a finite loss."""
    from lav_amd.train import LAV, TrainConfig
    seeded = LAV(TrainConfig(), torch.device("cpu"), what="lidar")
    for k, sd in dict(bev=seeded.bev_planner.state_dict(), lidar=seeded.state_dict("lidar"), uniplanner=seeded.state_dict("uniplanner")).items():
        torch.save(sd, tmp_path / f"{k}_seed.th")
    cmd = [sys.executable, os.path.join(REPO, "train_full_v2.py"), "--config-path", os.path.join(painted[4]["root"], "config.yaml"),
           "--batch-size", "2", "--num-epoch", "1", "--num-workers", "0", "--num-per-log", "1", "--save-dir", str(tmp_path / "ck"),
           "--bev", str(tmp_path / "bev_seed.th"), "--lidar", str(tmp_path / "lidar_seed.th"), "--uniplanner", str(tmp_path / "uniplanner_seed.th")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert '"steps": 3' in out.stdout and "6 recorded frames" in out.stdout
    logs = [ast.literal_eval(line.split(" ", 1)[1]) for line in out.stdout.splitlines() if line[:2] in ("0 ", "1 ", "2 ") and "{" in line]
    assert len(logs) == 3 and all("loss" in l and np.isfinite(list(l.values())).all() for l in logs), out.stdout[-2000:]
