"""--tensor-stats on the CPU: the specifications of the per-tensor rows and of the blame ring (lav_amd.train.optim.tensor_stats_numpy,
blame_numpy) against hand-counted values, the trainers' command line, the health stop's messages and the reader."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lav_amd.train import optim as O
from lav_amd.train import state as S
from lav_amd.train import tensor_stats as T
from tests.test_state_host import ENV, REPO, _command, _run, _same

F32 = np.float32


def _row(g, n=None, state=0):
    n = len(g) if n is None else n
    return dict(p=np.zeros(n, F32), g=np.asarray(g, F32), m=np.zeros(n, F32), v=np.zeros(n, F32), lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, state=state)


def test_rows_against_hand_counted_values():
    """Twelve elements: NaN, +Inf, -Inf, -0.0, a denormal, FLT_MAX, exactly 2^-40 and its float32 predecessor, exactly 2^22 and its
    predecessor, 1 and +0.  Bin 0 takes the zeros, the denormal and the predecessor of 2^-40; 2^-40 opens bin 1; 1 = 2^0 lies in bin 41;
    the predecessor of 2^22 closes bin 62; 2^22 and FLT_MAX lie in bin 63; the three that are not finite count nowhere else."""
    lo, hi = F32(2.0 ** -40), F32(2.0 ** 22)
    g = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 3.4028235e38, lo, np.nextafter(lo, F32(0)), hi, np.nextafter(hi, F32(0)), 1.0, 0.0], F32)
    t = _row(g)
    t["p"][:] = [np.inf, -3.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4.0]
    rows, wrows = O.tensor_stats_numpy([t], O.new_state(1), [np.array([1.0, np.nan, -9.0, -np.inf], F32), np.zeros(2, F32)])
    r = rows[0]
    want = np.zeros(64, np.int64)
    want[[0, 1, 41, 62, 63]] = [4, 1, 1, 1, 2]
    assert r["hist"].tolist() == want.tolist() and int(r["hist"].sum()) == 9
    assert (int(r["g_nonfinite"]), int(r["g_zeros"])) == (3, 2) and r["g_maxabs"].view(np.uint32) == 0x7F7FFFFF
    fin = g[np.isfinite(g)].astype(np.float64)
    assert r["g_sumsq"] == float(np.sum(fin * fin)) and r["g_sumsq"] > 1e76
    assert (int(r["p_nonfinite"]), float(r["p_sumsq"]), float(r["p_maxabs"])) == (1, 25.0, 4.0)
    assert (float(r["u_sumsq"]), float(r["u_maxabs"])) == (0.0, 0.0)
    assert [(int(w["nonfinite"]), float(w["maxabs"])) for w in wrows] == [(2, 9.0), (0, 0.0)]


def test_u_is_the_term_the_step_subtracted():
    """p starts at 0 and takes one applied step: u == -p in every bit.  A skipped step behind it leaves u alone.  At step 0 u is 0,
    whatever the moments hold."""
    rng = np.random.default_rng(3)
    n = 1000
    t = _row(np.exp(rng.uniform(np.log(1e-12), np.log(1e2), n)) * rng.choice([-1.0, 1.0], n))
    state, glob = O.new_state(1), np.zeros(1, O.GLOBAL_DTYPE)
    t["m"][:] = 1.0         # (a loaded moment under a step count of 0: still no update to describe)
    assert not O.update_term_numpy(t, state[0]).any()
    t["m"][:] = 0.0
    O.fused_adam_numpy([t], state, glob)
    assert glob[0]["applied"] == 1 and np.count_nonzero(t["p"]) == n
    u = O.update_term_numpy(t, state[0])
    assert np.array_equal(u.view(np.uint32), (-t["p"]).view(np.uint32))
    rows, _ = O.tensor_stats_numpy([t], state)
    assert rows[0]["u_maxabs"] == np.abs(t["p"]).max() and rows[0]["u_sumsq"] == rows[0]["p_sumsq"] > 0
    t["g"][7] = np.inf
    O.fused_adam_numpy([t], state, glob)
    assert glob[0]["skipped"] == 1 and np.array_equal(O.update_term_numpy(t, state[0]).view(np.uint32), u.view(np.uint32))


def test_blame_ring():
    """Bad gradients in tensors 2, 5, 6, 7 and 9 give the first four in table order with their counts; an applied step appends nothing;
    the fifth skipped step wraps the 16-record ring; a watched buffer that is not finite is named in its own ring."""
    tensors = [_row(np.full(4, 0.5), state=10 + i) for i in range(11)]
    state, glob, blame = O.new_state(32), np.zeros(1, O.GLOBAL_DTYPE), np.zeros(1, O.BLAME_DTYPE)
    watch = [np.ones(3, F32), np.ones(3, F32)]
    names = ([f"t{i}" for i in range(32)], ["bn.running_mean", "bn.running_var"])

    def step():
        O.fused_adam_numpy(tensors, state, glob, watch=watch)
        O.blame_numpy(tensors, glob, blame, watch)

    step()
    assert glob[0]["applied"] == 1 and blame[0]["written"].tolist() == [0, 0] and not blame.view(np.uint8).any()
    for i in (2, 5, 6, 7, 9):
        tensors[i]["g"][3] = np.nan
    tensors[6]["g"][:2] = -np.inf
    step()
    recs, bufs = O.blame_records(blame, names)
    assert [(r["name"], r["index"], r["nonfinite"], r["step"], r["ordinal"]) for r in recs] == \
        [("t12", 12, 1, 2, 0), ("t15", 15, 1, 2, 1), ("t16", 16, 3, 2, 2), ("t17", 17, 1, 2, 3)] and bufs == []
    for _ in range(3):
        step()
    assert blame[0]["written"].tolist() == [16, 0] and [r["step"] for r in O.blame_records(blame)[0]] == [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4
    watch[1][2] = np.inf
    step()
    recs, bufs = O.blame_records(blame, names)
    assert blame[0]["written"].tolist() == [20, 1] and [r["ordinal"] for r in recs] == list(range(4, 20))
    assert [r["step"] for r in recs] == [3] * 4 + [4] * 4 + [5] * 4 + [6] * 4 and blame[0]["ring"][0][0]["step"] == 6 and blame[0]["ring"][0][4]["step"] == 3
    assert [(r["name"], r["index"], r["nonfinite"], r["step"]) for r in bufs] == [("bn.running_var", 1, 1, 6)]
    for t in tensors:
        t["g"][:] = 0.5
    step()
    assert glob[0]["applied"] == 2 and blame[0]["written"].tolist() == [20, 1]       # applied, the buffer still bad: nothing is written


def _lines(path):
    return [json.loads(x) for x in open(path)]


@pytest.mark.parametrize("trainer", ["bev", "seg", "bra"])
def test_command_line(tmp_path, trainer):
    """--tensor-stats 2 over five iterations writes the iterations 0, 2 and 4; every name is a key of the checkpoint the trainer saves;
    the checkpoints equal those of the run without the flag in every bit, which writes no such file; --resume appends."""
    base = _command(trainer, tmp_path)
    if trainer != "bev":
        base = base + ["--num-per-log", "1"]
    a, b = tmp_path / "A", tmp_path / "B"
    r = _run(base + ["--num-epoch", "5", "--save-dir", str(a), "--state-dir", str(a), "--tensor-stats", "2"], tmp_path)
    _run(base + ["--num-epoch", "5", "--save-dir", str(b), "--fused-optim"], tmp_path)
    assert not (b / T.FILE).exists() and "tensor stats it" in r.stdout and '"fused_optim": true' in r.stdout
    lines = _lines(a / T.FILE)
    assert [ln["global_it"] for ln in lines] == [0, 2, 4]
    saved = torch.load(a / f"{trainer}_5.th")
    for ln in lines:
        assert ln["applied"] is True and ln["grad_norm"] > 0 and ln["clip"] == 1.0 and len(ln["tensors"]) > 10
        for name, t in list(ln["tensors"].items()) + list(ln["buffers"].items()):
            assert name.split("/", 1)[0] == trainer and name.split("/", 1)[1] in saved, name
        assert all(sum(t["grad_hist"]["bins"]) + t["grad_nonfinite"] == t["numel"] and t["weight_norm"] > 0 for t in ln["tensors"].values())
        assert all(t["update_ratio"] == t["update_norm"] / t["weight_norm"] for t in ln["tensors"].values())
    assert len(lines[0]["buffers"]) > 0 and all(b_["nonfinite"] == 0 for b_ in lines[0]["buffers"].values())
    _same(saved, torch.load(b / f"{trainer}_5.th"), "checkpoint")
    r = _run(base + ["--num-epoch", "7", "--save-dir", str(a), "--state-dir", str(a), "--tensor-stats", "2", "--resume", "auto"], tmp_path)
    assert "resumed from" in r.stdout
    assert [ln["global_it"] for ln in _lines(a / T.FILE)] == [0, 2, 4, 6]


def test_two_ranks_write_one_file(tmp_path):
    """train_bra_v2.py --tensor-stats 2 on two ranks over gloo: rank 0 alone writes, once per watched iteration; the replicas stay in
    sync."""
    launch = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29671",
              os.path.join(REPO, "train_bra_v2.py"), "--synthetic", "--device", "cpu", "--batch-size", "4", "--steps-per-epoch", "2", "--config-path", "",
              "--tensor-stats", "2", "--num-epoch", "2", "--save-dir", str(tmp_path / "ck")]
    r = subprocess.run(launch, cwd=str(tmp_path), capture_output=True, text=True, timeout=900, env=dict(os.environ, LAV_DIST_BACKEND="gloo"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert '"n_gpus": 2' in r.stdout and '"replicas_in_sync": true' in r.stdout
    assert sorted(os.listdir(tmp_path / "ck")) == ["bra_1.th", "bra_2.th", T.FILE]
    assert [ln["global_it"] for ln in _lines(tmp_path / "ck" / T.FILE)] == [0, 2]


def test_health_stop_names_the_tensors(tmp_path):
    """check_health with a blame names tensor, count and iteration in both messages; without one its messages are the old text."""
    ok = dict(applied=90, skipped=10, nonfinite=0, sumsq=4.0, clip=1.0, apply=1, watch_nonfinite=0, grad_norm=2.0)
    blame = ([dict(name="lidar/backbone.conv1.0.weight", nonfinite=7, global_it=41), dict(name="lidar/head.bias", nonfinite=1, global_it=42)],
             [dict(name="lidar/backbone.bn1.running_var", nonfinite=2, global_it=42)])
    old_skipped = ("training stopped: 11 optimiser steps were skipped for gradients that are not finite since the last log iteration "
                   "(--max-skipped-steps 10); there is no state file to --resume from (run with --state-dir)")
    old_watch = ("training stopped: 3 values of the watched buffers (BatchNorm running statistics) are not finite; "
                 "there is no state file to --resume from (run with --state-dir)")
    for kw, health, old, named in ((dict(), dict(ok, skipped=11), old_skipped, None), (dict(), dict(ok, watch_nonfinite=3), old_watch, None),
                                   (dict(blame=None), dict(ok, skipped=11), old_skipped, None), (dict(blame=([], [])), dict(ok, watch_nonfinite=3), old_watch, None),
                                   (dict(blame=blame), dict(ok, skipped=11), None, "lidar/backbone.conv1.0.weight (7 at iteration 41), lidar/head.bias (1 at iteration 42)"),
                                   (dict(blame=blame), dict(ok, watch_nonfinite=3), None, "lidar/backbone.bn1.running_var (2 at iteration 42)")):
        with pytest.raises(SystemExit) as e:
            S.check_health(health, 0, 10, None, **kw)
        if old is not None:
            assert str(e.value.code) == old
        else:
            assert named in str(e.value.code) and "no state file" in str(e.value.code) and "running_var" in str(e.value.code) or "conv1" in str(e.value.code)
    assert S.check_health(ok, 0, 10, None, blame=blame) == 10


def test_reader(tmp_path):
    """A file written by TensorStatsLog from a CPU FusedAdam, with a tensor whose gradient is always zero and a step that a NaN made
    skip: the reader lists both, the update ratios and the exponent ranges."""
    params = [torch.nn.Parameter(torch.full((50 if i < 2 else 200,), 1.0 + i)) for i in range(3)]
    opt = O.FusedAdam(params, lr=1e-2, watch=[torch.ones(4)], names=(["m/a.weight", "m/dead.weight", "m/c.weight"], ["m/bn.running_mean"]))
    log = T.TensorStatsLog(str(tmp_path), 1, first_it=100)
    for s in range(4):
        params[0].grad = torch.full((50,), 0.75)               # every element in [2^-1, 2^0)
        params[1].grad = torch.zeros(50)
        params[2].grad = torch.cat([torch.full((199,), 3.0), torch.tensor([2.0 ** -30])])     # 99.5 % in [2^1, 2^2)
        if s == 2:
            params[2].grad[5] = float("nan")
        opt.step()
        log.after_step(opt, 100 + s)
    blame = log.blamed(opt.blame())
    assert [(r["name"], r["nonfinite"], r["global_it"]) for r in blame[0]] == [("m/c.weight", 1, 102)]
    log.close()
    lines = _lines(tmp_path / T.FILE)
    assert [ln.get("global_it") for ln in lines] == [100, 101, 102, 102, 103] and lines[2]["applied"] is False
    assert lines[3] == dict(global_it=102, skipped=[dict(name="m/c.weight", nonfinite=1)], buffers=[])
    assert lines[0]["tensors"]["m/a.weight"]["grad_hist"] == dict(first=40, bins=[50]) and lines[0]["tensors"]["m/dead.weight"]["grad_zero_frac"] == 1.0
    r = subprocess.run([sys.executable, "-m", "lav_amd.train.tensor_stats", str(tmp_path / T.FILE), "--top", "5"], cwd=REPO, capture_output=True,
                       text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    assert "4 watched steps, iterations 100 .. 103" in out
    assert "gradient all zero in every line: 1\n  m/dead.weight\n" in out
    assert "m/a.weight: 2^-1 .. 2^0" in out and "m/c.weight: 2^1 .. 2^2" in out and "m/dead.weight: 0 .. 2^-40" in out
    assert "blamed steps: 1\n  it 102: m/c.weight (1)" in out
    med = float(np.median([ln["tensors"]["m/a.weight"]["update_ratio"] for ln in lines if "tensors" in ln]))
    assert f"{med:.3e} {lines[-1]['tensors']['m/a.weight']['update_ratio']:.3e} m/a.weight" in out
