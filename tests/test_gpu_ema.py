"""The fused Adam step with a moving average of the weights (csrc/optim.hip, lav_optim_adam_ema_step) against its specification
lav_amd.train.optim.fused_adam_numpy(..., ema_decay=) on an MI355X, in every stored bit and at every misalignment of the five
pointers; --ema and --val-data-dir of train_bev_v2.py and train_seg.py: the files, val.jsonl against the evaluation tools' own
command lines, and a run that ends in the same bits with and without its validation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lav_amd.train import optim as O
from tests import ema_util as E
from tests import optim_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, WORLD_SIZE="1", RANK="0")
DECAY = 0.9


class Device:
    """The flat buffers named in `keys` and the words of an EmaWorld in HBM."""

    def __init__(self, world, keys):
        self.w, self.keys = world, keys
        self.flat = {k: torch.from_numpy(world.flat[k].copy()).to(DEV) for k in keys}
        assert all(t.data_ptr() % 16 == 0 for t in self.flat.values())
        self.state, self.glob = U.to_device(world.state, DEV), U.to_device(world.glob, DEV)
        self.bases = {k: t.data_ptr() for k, t in self.flat.items()}

    def table(self, rows):
        t, chunks = self.w.device_table(self.bases, rows)
        return U.to_device(t, DEV), len(t), chunks

    def words(self):
        return self.glob.cpu().numpy().view(O.GLOBAL_DTYPE)[0]

    def bits(self):
        out = {k: self.flat[k].cpu().numpy().view(np.uint32) for k in self.keys if k != "g"}
        out["state"] = U.bits(self.state.cpu().numpy()).reshape(-1, 32)
        out["global"] = U.bits(self.words())
        return out


def _differ(a, b):
    return int(np.count_nonzero(np.asarray(a) != np.asarray(b)))


def test_ema_step_equals_the_specification_and_the_plain_step_in_every_bit():
    """Check e.  Four steps over tests.ema_util.EmaWorld (315 tensors: 1 .. 5, 63 .. 65, 255 .. 257, chunk - 1 .. chunk + 1, 2 chunk + 3,
    then 300 of 1 .. 7 elements; p, g, m, v, e at the six misalignment rows of MISALIGN5) through ops.optim_adam_ema_step: apply; apply
    with one tensor (chunk + 1 elements) left out of the table; skip (a NaN in the last element of the last tensor: data for the guard);
    apply.  After each step p, m, v and e - gaps and guard elements too - and every word equal the specification in every bit (the
    float64 sum of squares, whose order is the kernel's, is handed to the specification as in tests/test_gpu_optim.py), and p, m, v and
    the words equal those of ops.optim_adam_step on a twin of the world without shadows."""
    from lav_amd import ops
    chunk = O.chunk_length()
    w = E.EmaWorld(chunk)
    d, twin = Device(w, "pgmve"), Device(w, "pgmv")
    everything = list(range(len(w.rows)))
    assert [w.sizes[i] for i in (11, 12, 13, 14)] == [chunk - 1, chunk, chunk + 1, 2 * chunk + 3]
    plan = [(everything, False), ([i for i in everything if i != 13], False), (everything, True), (everything, False)]
    for step, (rows, nan) in enumerate(plan, 1):
        w.draw_gradients()
        if nan:
            w.rows[-1]["g"][-1] = np.nan
        for dev in (d, twin):
            dev.flat["g"].copy_(torch.from_numpy(w.flat["g"]))
        table, nt, chunks = d.table(rows)
        shadow = U.to_device(w.shadow_pointers(d.bases["e"], rows), DEV)
        ops.optim_adam_ema_step(table, nt, chunks, None, 0, 0, d.state, d.glob, shadow, DECAY)
        ttable, _, _ = twin.table(rows)
        ops.optim_adam_step(ttable, nt, chunks, None, 0, 0, twin.state, twin.glob)
        got, plain = d.bits(), twin.bits()
        before_e = w.flat["e"].copy()
        O.fused_adam_numpy([w.rows[i] for i in rows], w.state, w.glob, sumsq=float(d.words()["sumsq"]), ema_decay=DECAY)
        want = dict({k: w.flat[k].view(np.uint32) for k in "pmve"}, state=U.bits(w.state).reshape(-1, 32), **{"global": U.bits(w.glob)})
        for k in want:
            assert _differ(got[k], want[k]) == 0, f"step {step}: {k} differs from the specification at {_differ(got[k], want[k])} places"
        for k in plain:
            assert _differ(got[k], plain[k]) == 0, f"step {step}: {k} differs from optim_adam_step's at {_differ(got[k], plain[k])} places"
        moved = _differ(before_e.view(np.uint32), w.flat["e"].view(np.uint32))
        assert (moved == 0) == nan, f"step {step}: {moved} shadow elements moved"
        assert int(w.glob[0]["apply"]) == int(not nan) and int(w.glob[0]["nonfinite"]) == int(nan)
    assert w.glob[0]["applied"] == 3 and w.glob[0]["skipped"] == 1
    assert w.state["step"][13] == 2 and w.state["step"][0] == 3
    with pytest.raises(RuntimeError, match="ema_decay"):
        ops.optim_adam_ema_step(table, nt, chunks, None, 0, 0, d.state, d.glob, shadow, 1.0)


def test_fused_adam_with_shadows_on_the_device_equals_the_host():
    """FusedAdam(ema_decay=) on cuda parameters against the same optimiser on CPU copies, three steps with the second skipped: shadows,
    parameters and moments in every bit; the pointer array rides behind the tables of one pinned blob."""
    g = torch.Generator().manual_seed(3)
    host = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (5, 4097, 300, 8200)]
    dev = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in host]
    oh, od = O.FusedAdam(host, lr=1e-2, ema_decay=DECAY), O.FusedAdam(dev, lr=1e-2, ema_decay=DECAY)
    for s in range(3):
        for ph, pd in zip(host, dev):
            ph.grad = torch.randn(ph.shape, generator=g)
            if s == 1 and ph is host[2]:
                ph.grad[7] = float("inf")
            pd.grad = ph.grad.to(DEV)
        oh.step()
        od.step()
    assert od.health()["skipped"] == 1 and od.health()["applied"] == 2
    for ph, pd in zip(host, dev):
        for a, b in ((ph, pd), (oh.state[ph]["ema"], od.state[pd]["ema"]), (oh.state[ph]["exp_avg_sq"], od.state[pd]["exp_avg_sq"])):
            assert torch.equal(a.detach().view(torch.int32), b.detach().cpu().view(torch.int32))
        assert not torch.equal(od.state[pd]["ema"], pd.detach())


# ------------------------------------------------------------------------------------------------------------ the trainers
def _run(script, tmp, *flags):
    r = subprocess.run([sys.executable, os.path.join(REPO, script)] + [str(f) for f in flags], cwd=str(tmp), capture_output=True, text=True,
                       timeout=900, env=ENV)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _val_lines(save_dir):
    with open(os.path.join(save_dir, "val.jsonl")) as f:
        return [json.loads(line) for line in f]


def _same_tensors(a, b):
    x, y = torch.load(a), torch.load(b)
    assert list(x) == list(y)
    for k in x:
        assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), f"{os.path.basename(a)}: {k}"


def test_train_bev_validates_each_save_and_ends_in_the_same_bits(tmp_path):
    """Check f.  train_bev_v2.py --synthetic --deterministic --ema 0.9, two epochs of two steps, --val-data-dir on a recorded route,
    --val-max 4: val.jsonl has a raw and an ema line per epoch whose counters are eval_bev_v2's own on the same file and directory;
    bev_2.th and bev_ema_2.th equal those of the same run without --val-data-dir in every tensor bit."""
    from lav_amd.train import evaluate_bev
    from tests.util import dataset_fixture_config
    cfg = dataset_fixture_config(str(tmp_path), routes=1, frames=25)
    data = os.path.join(str(tmp_path), "data")
    a, b = tmp_path / "A", tmp_path / "B"
    base = ["--synthetic", "--deterministic", "--ema", DECAY, "--num-epoch", 2, "--steps-per-epoch", 2, "--batch-size", 2, "--config-path", cfg,
            "--num-per-log", 1, "--num-workers", 0]
    r = _run("train_bev_v2.py", tmp_path, *base, "--save-dir", a, "--val-data-dir", data, "--val-max", 4)
    _run("train_bev_v2.py", tmp_path, *base, "--save-dir", b)
    assert not (b / "val.jsonl").exists()
    lines = _val_lines(a)
    assert [(l["epoch"], l["weights"], l["global_it"]) for l in lines] == [(1, "raw", 2), (1, "ema", 2), (2, "raw", 4), (2, "ema", 4)]
    assert sum(line.startswith("val epoch") and "buffers: live" in line for line in r.stdout.splitlines()) == 4
    assert json.loads(r.stdout.strip().splitlines()[-1])["ema_decay"] == DECAY
    for l in lines:
        name = "bev_{}.th" if l["weights"] == "raw" else "bev_ema_{}.th"
        path = str(a / name.format(l["epoch"]))
        assert l["checkpoints"] == [path] and l["buffers"] == "live" and l["counters"]["frames"] == 4
        own = evaluate_bev.main(["--config-path", cfg, "--data-dir", data, "--bev", path, "--max-frames", "4", "--num-workers", "0"])
        assert len(own) == 1 and own[0]["counters"] == l["counters"] and own[0]["precision"] == l["precision"], (l["epoch"], l["weights"])
    assert lines[0]["counters"] != lines[1]["counters"] or lines[2]["counters"] != lines[3]["counters"]
    for f in ("bev_2.th", "bev_ema_2.th", "bev_1.th", "bev_ema_1.th"):
        _same_tensors(str(a / f), str(b / f))


def test_train_seg_on_camera_routes_validates_raw_and_ema(tmp_path):
    """Check g.  train_seg.py over a camera route set (72 x 64 images) with --ema and --val-data-dir: two lines per epoch, each with
    `weights` and buffers: live; the raw line's counters are eval_seg's on seg_{e}.th."""
    from lav_amd.train import evaluate_camera
    from tests.test_train_seg_host import seg_routes
    cfg = seg_routes(str(tmp_path))
    data = os.path.join(str(tmp_path), "data")
    out = tmp_path / "S"
    r = _run("train_seg.py", tmp_path, "--config-path", cfg, "--batch-size", 20, "--num-epoch", 2, "--num-workers", 0, "--ema", DECAY,
             "--save-dir", out, "--val-data-dir", data, "--val-max", 30)
    lines = _val_lines(out)
    assert [(l["epoch"], l["weights"]) for l in lines] == [(1, "raw"), (1, "ema"), (2, "raw"), (2, "ema")]
    assert sum(line.startswith("val epoch") and "buffers: live" in line for line in r.stdout.splitlines()) == 4
    for l in lines:
        assert l["buffers"] == "live" and l["what"] == "eval_seg" and l["checkpoints"] == [str(out / ("seg_{}.th" if l["weights"] == "raw" else "seg_ema_{}.th").format(l["epoch"]))]
        if l["weights"] == "raw":
            own = evaluate_camera.main("seg", ["--config-path", cfg, "--data-dir", data, "--seg", l["checkpoints"][0], "--max-images", "30", "--num-workers", "0"])
            assert len(own) == 1 and own[0]["counters"] == l["counters"], l["epoch"]
    raw, ema = torch.load(out / "seg_2.th"), torch.load(out / "seg_ema_2.th")
    assert list(raw) == list(ema) and any(not torch.equal(raw[k], ema[k]) for k in raw)
    assert all(torch.equal(raw[k], ema[k]) for k in raw if "running_" in k or "num_batches" in k)


def test_validation_directory_without_routes_is_refused_before_the_first_step(tmp_path):
    from tests.test_train_seg_host import seg_routes
    cfg = seg_routes(str(tmp_path))
    empty = tmp_path / "empty"
    empty.mkdir()
    r = subprocess.run([sys.executable, os.path.join(REPO, "train_seg.py"), "--synthetic", "--config-path", cfg, "--batch-size", "2", "--steps-per-epoch", "1",
                        "--num-epoch", "1", "--save-dir", str(tmp_path / "S"), "--val-data-dir", str(empty)], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=600, env=ENV)
    assert r.returncode != 0 and "--val-data-dir" in r.stderr and "no recorded images" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "S").exists() and "saved to" not in r.stdout


def test_two_ranks_validate_on_rank_0_and_stay_in_step(tmp_path):
    """train_bev_v2.py on two gloo ranks that share the GPU, --ema and --val-data-dir: rank 0 validates behind each save while rank 1
    waits for its verdict, the evaluation's own models issue no collective (a DistributedDataParallel built there would), so both
    epochs run, val.jsonl has its four lines and the replicas end in sync.  (Not run here: a validation that fails on rank 0, whose
    message the other ranks receive in the same collective and end with.)"""
    from tests.util import dataset_fixture_config
    cfg = dataset_fixture_config(str(tmp_path), routes=1, frames=25)
    out = tmp_path / "ck"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29673", os.path.join(REPO, "train_bev_v2.py"), "--synthetic", "--config-path", cfg, "--batch-size", "2",
                        "--num-epoch", "2", "--steps-per-epoch", "1", "--num-workers", "0", "--ema", str(DECAY), "--save-dir", str(out),
                        "--val-data-dir", os.path.join(str(tmp_path), "data"), "--val-max", "2"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, LAV_DIST_BACKEND="gloo"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert '"n_gpus": 2' in r.stdout and '"replicas_in_sync": true' in r.stdout and '"steps": 2' in r.stdout, r.stdout[-1500:]
    assert [(l["epoch"], l["weights"]) for l in _val_lines(out)] == [(1, "raw"), (1, "ema"), (2, "raw"), (2, "ema")]
