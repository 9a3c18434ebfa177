"""train_bra_v2 on the host: the 'bra' loader against the reference BrakePredictionDataset's samples (tests/golden/bra_dataset.npz),
BrakeTrainer.train_bra on CPU against the reference's LAV.train_bra (tests/golden/bra_train.npz), the train_bra_v2.py command line
(one rank and two gloo ranks), the synthetic routes' telephoto images and the agent's loading of 4-class brake checkpoints."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests.util import GOLD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bra_routes(root):
    """tests/golden/make_golden_bra.py:bra_routes (that script imports the reference and cannot be imported here)."""
    from lav_amd.data import synthetic_route
    synthetic_route.make_dataset(os.path.join(root, "data"), routes=2, frames=8, seed=4, points=200, cameras=5, camera_hw=(40, 32),
                                 tel=True, tel_hw=(48, 64))
    with open(os.path.join(GOLD, "dataset_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["data_dir"] = os.path.join(root, "data")
    cfg["num_plan"] = 4
    cfg["crop_tel_bottom"] = 16
    path = os.path.join(root, "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def test_bra_loader_matches_reference_dataset(tmp_path):
    import types
    from lav_amd.data import get_data_loader
    g = dict(np.load(os.path.join(GOLD, "bra_dataset.npz")))
    args = types.SimpleNamespace(config_path=bra_routes(str(tmp_path)), seed=2021, batch_size=2, num_workers=0)
    ds = get_data_loader("bra", args).dataset
    assert len(ds) == int(g["len"]) == ds.num_frames == 8
    where = {(os.path.basename(ds.dir_map[i]), ds.idx_map[i]): i for i in range(ds.num_frames)}
    keys = sorted({k.rsplit("/", 1)[0] for k in g if k != "len"})
    assert len(keys) == 3
    for key in keys:
        route, frame = key.split("/")
        sample = ds[where[(route, int(frame))]]
        for name, a in zip(("rgb", "tel_rgb", "sem", "tel_sem", "bra"), sample):
            ref = g[f"{key}/{name}"]
            np.testing.assert_array_equal(np.asarray(a), ref, err_msg=f"{key}/{name}")
            if name != "bra":
                assert np.asarray(a).dtype == ref.dtype, name
        assert isinstance(sample[4], int)
    rgb, tel_rgb, sem, tel_sem, bra = next(iter(get_data_loader("bra", args)))
    assert rgb.shape == (2, 40, 96, 3) and tel_rgb.shape == (2, 32, 64, 3) and sem.shape == (2, 40, 96) and tel_sem.shape == (2, 32, 64)
    assert rgb.dtype == torch.uint8 and sem.dtype == torch.uint8 and bra.shape == (2,)


def test_rgb_loader_still_not_provided():
    import types
    from lav_amd.data import get_data_loader
    with pytest.raises(NotImplementedError, match="rgb"):
        get_data_loader("rgb", types.SimpleNamespace(config_path="", seed=0, batch_size=1, num_workers=0))


def test_synthetic_route_tel_leaves_other_records_unchanged(tmp_path):
    from lav_amd.data import lmdb_ro, synthetic_route
    synthetic_route.make_route(str(tmp_path / "a"), seed=5, frames=3, points=50, cameras=2)
    synthetic_route.make_route(str(tmp_path / "b"), seed=5, frames=3, points=50, cameras=2, tel=True, tel_hw=(40, 48))
    a = dict(lmdb_ro.open(str(tmp_path / "a")).begin().items())
    b = dict(lmdb_ro.open(str(tmp_path / "b")).begin().items())
    extra = {k for k in b if k not in a}
    assert extra == {f"{s}_{t:05d}".encode() for s in ("tel_rgb", "tel_sem") for t in range(3)}
    assert all(a[k] == b[k] for k in a)


def test_synthetic_bra_batch_contract():
    from lav_amd.train import synthetic_bra_batch
    rgb, tel_rgb, sem, tel_sem, bra = synthetic_bra_batch(3, seed=1, hw=(64, 192), tel_hw=(32, 96))
    assert rgb.shape == (3, 64, 192, 3) and tel_rgb.shape == (3, 32, 96, 3) and sem.shape == (3, 64, 192) and tel_sem.shape == (3, 32, 96)
    assert rgb.dtype == tel_rgb.dtype == sem.dtype == tel_sem.dtype == torch.uint8 and bra.dtype == torch.int64
    assert int(sem.max()) < 4 and int(tel_sem.max()) < 4 and set(bra.tolist()) <= {0, 1}


def bra_reference_run(device):
    """BrakeTrainer for the fixture's three steps (seeded weights, batch 2 of 64 x 192 + 64 x 96)."""
    from lav_amd.train import BrakeTrainer, TrainConfig, synthetic_bra_batch
    g = dict(np.load(os.path.join(GOLD, "bra_train.npz")))
    tr = BrakeTrainer(TrainConfig(), device)
    before = {k: v.detach().double().cpu().clone() for k, v in tr.bra_model.named_parameters()}
    losses, preds = [], []
    for step in range(3):
        info = tr.train_bra(*synthetic_bra_batch(2, seed=400 + step, hw=(64, 192), tel_hw=(64, 96), num_classes=4))
        losses.append(info["loss"])
        preds.append(info["pred_bra"])
        assert info["pred_sem1"].shape == (64, 192) and info["pred_sem2"].shape == (64, 96)
        assert info["rgb1"].shape == (64, 192, 3) and info["rgb2"].shape == (64, 96, 3) and info["bra"] in (0.0, 1.0)
    return g, tr, before, losses, preds, info


def state_sums(sd, names, before):
    sums = np.array([sd[k].double().sum().item() for k in names])
    abs_sums = np.array([sd[k].double().abs().sum().item() for k in names])
    deltas = np.array([(sd[k].double().cpu() - before[k]).abs().sum().item() if k in before else 0.0 for k in names])
    return sums, abs_sums, deltas


def test_train_bra_on_cpu_matches_reference_trainer():
    g, tr, before, losses, preds, info = bra_reference_run("cpu")
    np.testing.assert_allclose(losses, g["losses"], rtol=1e-5)
    np.testing.assert_allclose(np.log(preds), np.log(g["pred_bra"]), rtol=1e-4)
    sd = tr.state_dict("bra")
    names = [str(n) for n in g["names"]]
    assert names == list(sd)
    sums, abs_sums, deltas = state_sums(sd, names, before)
    np.testing.assert_allclose(sums, g["sums"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(abs_sums, g["abs_sums"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(deltas, g["delta_abs_sums"], rtol=1e-3, atol=1e-6)
    assert (info["pred_sem1"] == g["pred_sem1"]).mean() > 0.99 and (info["pred_sem2"] == g["pred_sem2"]).mean() > 0.99


def test_state_dict_keys_and_shapes_are_the_reference_models():
    from lav_amd.train import BrakeTrainer, TrainConfig
    g = dict(np.load(os.path.join(GOLD, "bra_train.npz")))
    sd = BrakeTrainer(TrainConfig(), "cpu").state_dict("bra")
    assert list(sd) == [str(n) for n in g["names"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]
    assert sd["seg_head.upconv.9.weight"].shape[0] == 4


def test_fc_is_frozen_and_adam_sees_every_parameter():
    from lav_amd.train import BrakeTrainer, TrainConfig
    tr = BrakeTrainer(TrainConfig(lr=1e-4), "cpu")
    frozen = {n for n, p in tr.bra_model.named_parameters() if not p.requires_grad}
    assert frozen == {"conv_backbone.fc.weight", "conv_backbone.fc.bias", "normalize.mean", "normalize.std"}
    assert sum(len(gr["params"]) for gr in tr.bra_optim.param_groups) == len(list(tr.bra_model.parameters()))
    assert tr.bra_optim.param_groups[0]["lr"] == 1e-4 and not hasattr(tr, "bra_scheduler")


def test_train_bra_cli_writes_loadable_checkpoint(tmp_path):
    """python train_bra_v2.py --synthetic ... on the CPU: bra_1.th loads strictly into RGBBrakePredictionModel([4, 10, 18])."""
    out = tmp_path / "ck"
    r = subprocess.run([sys.executable, os.path.join(REPO, "train_bra_v2.py"), "--synthetic", "--device", "cpu", "--num-epoch", "1",
                        "--batch-size", "2", "--steps-per-epoch", "1", "--save-dir", str(out), "--config-path", ""],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    from lav_amd.rgb import RGBBrakePredictionModel
    m = RGBBrakePredictionModel([4, 10, 18])
    m.load_state_dict(torch.load(out / "bra_1.th", map_location="cpu"), strict=True)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["what"] == "bra" and res["samples_per_s"] > 0 and res["steps"] == 1


def test_agent_loader_fits_4_class_seg_head_and_rejects_trunk_mismatch():
    from lav_amd import synth
    from lav_amd.lav_agent import fit_bra_seg_head
    from lav_amd.rgb import RGBBrakePredictionModel
    ref = RGBBrakePredictionModel([4, 10, 18])
    sd = synth.seeded_state_dict(ref, prefix="bra.")
    agent_model = RGBBrakePredictionModel([4, 6, 7, 10])          # the agent's seg_channels: 5 classes
    with pytest.raises(RuntimeError, match="seg_head.upconv.9"):
        agent_model.load_state_dict(sd)
    fit_bra_seg_head(agent_model, sd).load_state_dict(sd)
    assert agent_model.seg_head.upconv[9].out_channels == 4
    assert torch.equal(agent_model.attn1.q, sd["attn1.q"])
    # a checkpoint that loads today is left alone (seeded weights of the module itself)
    same = RGBBrakePredictionModel([4, 6, 7, 10])
    head = same.seg_head
    fit_bra_seg_head(same, synth.seeded_state_dict(same, prefix="bra.")).load_state_dict(synth.seeded_state_dict(same, prefix="bra."))
    assert same.seg_head is head
    # any other mismatch still raises
    bad = dict(sd)
    bad["conv_backbone.layer1.0.conv1.weight"] = torch.zeros(64, 64, 5, 5)
    with pytest.raises(RuntimeError, match="layer1.0.conv1"):
        fit_bra_seg_head(RGBBrakePredictionModel([4, 6, 7, 10]), bad).load_state_dict(bad)


def test_world_size_2_gloo_train_bra_replicas_stay_identical(tmp_path):
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29653", os.path.join(REPO, "train_bra_v2.py"), "--synthetic", "--device", "cpu", "--batch-size", "4",
                          "--num-epoch", "1", "--steps-per-epoch", "2", "--save-dir", str(tmp_path / "ck"), "--config-path", ""],
                         cwd=str(tmp_path), capture_output=True, text=True, timeout=900, env=dict(os.environ, LAV_DIST_BACKEND="gloo"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert '"n_gpus": 2' in out.stdout and '"replicas_in_sync": true' in out.stdout and '"steps": 2' in out.stdout, out.stdout[-1500:]
