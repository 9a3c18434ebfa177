"""--state-dir / --resume of the trainers and the health stop, on the CPU: a run that is stopped after two epochs and resumed ends in
the same bits as the run that was never stopped; the default command line writes what it always wrote."""
import json
import os
import subprocess
import sys

import pytest
import torch

from lav_amd.train import state as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, WORLD_SIZE="1", RANK="0")


def _command(trainer, tmp):
    """The command lines of tests/test_train_host.py:70-73, test_train_seg_host.py:108 and test_train_bra_host.py:143, with --augment 0.5
    for the two camera trainers."""
    if trainer == "bev":
        import yaml
        cfgp = tmp / "config_v2.yaml"
        if not cfgp.exists():
            cfgp.write_text(yaml.safe_dump(dict(num_plan=20, num_cmds=6, cmd_weight=0.1, branch_weights=[5, 5, 5, 1, 1, 1], camera_x=1.5)))
        return [sys.executable, os.path.join(REPO, "train_bev_v2.py"), "--synthetic", "--device", "cpu", "--config-path", str(cfgp),
                "--batch-size", "1", "--steps-per-epoch", "1", "--num-per-log", "1"]
    script = {"seg": "train_seg.py", "bra": "train_bra_v2.py"}[trainer]
    return [sys.executable, os.path.join(REPO, script), "--synthetic", "--device", "cpu", "--batch-size", "2", "--steps-per-epoch", "1",
            "--config-path", "", "--augment", "0.5"]


def _run(cmd, tmp, ok=True):
    r = subprocess.run(cmd, cwd=str(tmp), capture_output=True, text=True, timeout=900, env=ENV)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def _same(a, b, where="state"):
    """Equal in every bit, through dicts, lists and tensors."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and torch.equal(a, b), where
    else:
        assert a == b and type(a) is type(b), (where, a, b)


@pytest.mark.parametrize("fused", [False, True], ids=["adam", "fused"])
@pytest.mark.parametrize("trainer", ["bev", "seg", "bra"])
def test_resume_is_exact(tmp_path, trainer, fused):
    """Check 4: --num-epoch 4 --state-dir A against --num-epoch 2 --state-dir B followed by --num-epoch 4 --state-dir B --resume auto.
    The final {name}_4.th and the optimiser, scheduler and global_it entries of state_4.th are equal in every bit; B keeps the two
    newest state files."""
    base = _command(trainer, tmp_path) + (["--fused-optim"] if fused else [])
    a, b = tmp_path / "A", tmp_path / "B"
    _run(base + ["--num-epoch", "4", "--save-dir", str(a), "--state-dir", str(a)], tmp_path)
    _run(base + ["--num-epoch", "2", "--save-dir", str(b), "--state-dir", str(b)], tmp_path)
    assert sorted(f for f in os.listdir(b) if f.startswith("state")) == ["state_1.th", "state_2.th"]
    r = _run(base + ["--num-epoch", "4", "--save-dir", str(b), "--state-dir", str(b), "--resume", "auto"], tmp_path)
    assert "resumed from" in r.stdout and "state_2.th" in r.stdout
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["steps"] == 4 and summary["epochs"] == 4 and ("fused_optim" in summary) == fused
    assert sorted(f for f in os.listdir(b) if f.startswith("state")) == ["state_3.th", "state_4.th"]
    _same(torch.load(a / f"{trainer}_4.th"), torch.load(b / f"{trainer}_4.th"), "checkpoint")
    sa, sb = S.load(a / "state_4.th"), S.load(b / "state_4.th")
    assert sa["global_it"] == 4 and sa["epoch"] == 4
    for k in ("optimizer", "scheduler", "global_it", "steps", "augmenters", "models"):
        _same(sa[k], sb[k], k)
    if fused:
        assert "beta1_power" in sa["optimizer"]["state"][0]
    if trainer != "bev":
        assert sa["augmenters"] and all(n == 8 for n in sa["augmenters"])      # two images per step, four steps


def test_default_is_untouched_refusals_and_empty_resume(tmp_path):
    """Checks 5 and 6 on train_bra_v2.py.  Without the new flags the save directory holds the checkpoints only and the summary has no
    new key; --resume with another --batch-size or --seed exits naming the key; --resume auto on an empty directory trains from
    scratch."""
    base = _command("bra", tmp_path)[:-2]
    ck, st = tmp_path / "ck", tmp_path / "st"
    r = _run(base + ["--num-epoch", "1", "--save-dir", str(ck)], tmp_path)
    assert sorted(os.listdir(ck)) == ["bra_1.th"]
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert list(summary) == ["what", "samples_per_s", "n_gpus", "replicas_in_sync", "global_batch", "steps", "epochs", "data", "lr"]
    assert "grad_norm" not in r.stdout and "state in" not in r.stdout
    r = _run(base + ["--num-epoch", "1", "--save-dir", str(ck), "--state-dir", str(st), "--resume", "auto"], tmp_path)
    assert "resumed from" not in r.stdout and json.loads(r.stdout.strip().splitlines()[-1])["steps"] == 1
    assert os.listdir(st) == ["state_1.th"]
    for flag, value, key in (("--batch-size", "4", "batch_size"), ("--seed", "7", "seed")):
        # (the last occurrence of a flag counts)
        r = _run(base + [flag, value] + ["--num-epoch", "2", "--save-dir", str(ck), "--state-dir", str(st), "--resume", "auto"], tmp_path, ok=False)
        assert r.returncode != 0 and key in r.stderr and value in r.stderr, r.stderr[-2000:]
    r = _run(base + ["--num-epoch", "2", "--save-dir", str(ck), "--resume", str(st / "missing.th")], tmp_path, ok=False)
    assert r.returncode != 0       # an explicit PATH that is not there is an error, not a fresh start


def test_two_ranks_over_gloo_resume(tmp_path):
    """Check 7: train_bra_v2.py --fused-optim on two ranks over gloo, 2 epochs with --state-dir, resumed to 3: replicas_in_sync, and
    bra_3.th equals the straight 3-epoch run's."""
    launch = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29667",
              os.path.join(REPO, "train_bra_v2.py"), "--synthetic", "--device", "cpu", "--batch-size", "4", "--steps-per-epoch", "2", "--config-path", "",
              "--fused-optim"]
    env = dict(os.environ, LAV_DIST_BACKEND="gloo")
    outs = []
    for name, extra in (("A", ["--num-epoch", "3"]), ("D", ["--num-epoch", "2"]), ("D", ["--num-epoch", "3", "--resume", "auto"])):
        d = tmp_path / name
        r = subprocess.run(launch + ["--save-dir", str(d), "--state-dir", str(d)] + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert '"n_gpus": 2' in r.stdout and '"replicas_in_sync": true' in r.stdout and '"fused_optim": true' in r.stdout, r.stdout[-1500:]
        outs.append(r.stdout)
    assert "resumed from" in outs[2] and '"steps": 6' in outs[2]
    assert len(S.load(tmp_path / "D" / "state_3.th")["rng"]) == 2
    _same(torch.load(tmp_path / "A" / "bra_3.th"), torch.load(tmp_path / "D" / "bra_3.th"), "checkpoint")


def test_health_stop(tmp_path):
    """Check 8: the function the trainers' main asks on every log iteration.  It ends the run for a watched buffer that is not finite
    and for more than --max-skipped-steps skipped steps since the last log iteration, naming the newest state file or saying that
    there is none; otherwise it returns the skipped count to remember."""
    ok = dict(applied=90, skipped=10, nonfinite=0, sumsq=4.0, clip=1.0, apply=1, watch_nonfinite=0, grad_norm=2.0)
    assert S.check_health(ok, 0, 10, None) == 10 and S.check_health(dict(ok, skipped=25), 15, 10, str(tmp_path)) == 25
    with pytest.raises(SystemExit) as e:
        S.check_health(dict(ok, skipped=11), 0, 10, str(tmp_path))
    assert e.value.code not in (0, None) and "11 optimiser steps were skipped" in str(e.value.code) and "no state file" in str(e.value.code)
    for epoch in (2, 10, 9):
        S.write(dict(epoch=epoch), str(tmp_path))
    assert [e_ for e_, _ in S.state_files(str(tmp_path))] == [9, 10] and not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    with pytest.raises(SystemExit) as e:
        S.check_health(dict(ok, watch_nonfinite=3), 10, 10, str(tmp_path))
    assert os.path.join(str(tmp_path), "state_10.th") in str(e.value.code) and "not finite" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        S.check_health(dict(ok, skipped=30), 10, 10, str(tmp_path))
    assert "--resume " + os.path.join(str(tmp_path), "state_10.th") in str(e.value.code)
