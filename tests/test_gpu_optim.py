"""The multi-tensor statistics and Adam kernels (csrc/optim.hip, lav_optim_grad_stats / lav_optim_adam_step) against their
specification lav_amd.train.optim.fused_adam_numpy on an MI355X: every stored bit of p, m, v and of the words at sizes around a lane,
a wave, a workgroup and a chunk, at every misalignment of the four pointers; the guard; FusedAdam in the trainer."""
import math

import numpy as np
import pytest
import torch

from lav_amd.train import optim as O
from tests import optim_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


class DeviceWorld:
    """tests.optim_util.World with a copy of its four flat buffers and of its words in HBM."""

    def __init__(self, seed=0):
        from lav_amd import ops
        self.ops, self.chunk = ops, O.chunk_length()
        self.w = U.World(self.chunk, seed=seed)
        self.flat = {k: torch.from_numpy(self.w.flat[k].copy()).to(DEV) for k in "pgmv"}
        assert all(t.data_ptr() % 16 == 0 for t in self.flat.values())
        self.state = U.to_device(self.w.state, DEV)
        self.glob = U.to_device(self.w.glob, DEV)
        self.bases = {k: t.data_ptr() for k, t in self.flat.items()}
        self.tables = {}

    def table(self, rows=None):
        key = None if rows is None else tuple(rows)
        if key not in self.tables:
            t, chunks = self.w.device_table(self.bases, rows)
            self.tables[key] = (U.to_device(t, DEV), len(t), chunks)
        return self.tables[key]

    def new_gradients(self):
        self.w.draw_gradients()
        self.flat["g"].copy_(torch.from_numpy(self.w.flat["g"]))

    def words(self):
        return self.glob.cpu().numpy().view(O.GLOBAL_DTYPE)[0]

    def assert_equal(self, what):
        for k in "pmv":
            got = self.flat[k].cpu().numpy()
            bad = np.flatnonzero(got.view(np.uint32) != self.w.flat[k].view(np.uint32))
            assert bad.size == 0, f"{what}: {k} differs at {bad.size} elements, first {bad[:5]}: {got[bad[:5]]} != {self.w.flat[k][bad[:5]]}"
        got = self.state.cpu().numpy().view(O.STATE_DTYPE)
        bad = np.flatnonzero(np.any(U.bits(got).reshape(-1, 32) != U.bits(self.w.state).reshape(-1, 32), axis=1))
        assert bad.size == 0, f"{what}: the words of {bad.size} tensors differ, first {bad[:3]}: {got[bad[:3]]} != {self.w.state[bad[:3]]}"
        assert U.bits(self.words()).tolist() == U.bits(self.w.glob).tolist(), f"{what}: global words {self.words()} != {self.w.glob[0]}"


def _fsum_sq(world, rows=None):
    idx = range(len(world.rows)) if rows is None else rows
    vals = np.concatenate([world.rows[i]["g"] for i in idx]).astype(np.float64)
    vals = vals[np.isfinite(vals)]
    return math.fsum((vals * vals).tolist()), vals.size


def test_kernels_equal_the_specification_in_every_bit():
    """Check 9.  Three consecutive steps over tests.optim_util.World's table (1 115 tensors: 1 .. 5, 63 .. 65, 255 .. 257, chunk - 1 ..
    chunk + 1, 2 chunk + 3, then 1 100 of 1 .. 7 elements; p, g, m, v at the eight misalignment rows of MISALIGN; +-0, 1e-20, 1e-25
    gradients, v = 0 under g = 0, negative moments): after each, p, m, v (the gaps and the guard elements behind them too), every
    tensor's words and the global words equal fused_adam_numpy's in every bit.  The float64 sum of squares is the one word whose order
    of summation is the kernel's: it is held to n * 2^-53 relative of math.fsum, then handed to the specification.  Before the first
    step two statistics launches give the same words and move nothing else.  Step 2 leaves two tensors out (their step counts stay
    behind), step 3 clips at a third of the norm."""
    d = DeviceWorld()
    w = d.w
    everything = list(range(len(w.rows)))
    some = [i for i in everything if i not in (5, 20)]
    for step, (rows, clip) in enumerate([(everything, False), (some, False), (everything, True)], 1):
        d.new_gradients()
        exact, n = _fsum_sq(w, rows)
        max_norm = math.sqrt(exact) / 3 if clip else None
        table, nt, chunks = d.table(None if rows is everything else rows)
        if step == 1:
            before = U.bits(d.words()).copy()
            d.ops.optim_grad_stats(table, nt, chunks, None, 0, 0, d.glob, None)
            first = d.words().copy()
            d.ops.optim_grad_stats(table, nt, chunks, None, 0, 0, d.glob, None)
            assert U.bits(first).tolist() == U.bits(d.words()).tolist()
            assert first["applied"] == 0 and first["skipped"] == 0 and first["nonfinite"] == 0 and first["apply"] == 1 and first["clip"] == 1.0
            assert abs(first["sumsq"] - exact) <= n * 2.0 ** -53 * exact
            d.glob.copy_(torch.from_numpy(before))
        d.ops.optim_adam_step(table, nt, chunks, None, 0, 0, d.state, d.glob, max_norm)
        got = d.words()
        print(f"step {step}: sumsq {got['sumsq']!r} fsum {exact!r} relative {abs(got['sumsq'] - exact) / exact:.3e} bound {n * 2.0 ** -53:.3e} clip {got['clip']!r}")
        assert abs(got["sumsq"] - exact) <= n * 2.0 ** -53 * exact
        O.fused_adam_numpy([w.rows[i] for i in rows], w.state, w.glob, max_norm, sumsq=float(got["sumsq"]))
        if clip:
            assert 0.33 < float(w.glob[0]["clip"]) < 0.34
        d.assert_equal(f"step {step}")
    assert w.state["step"][5] == 2 and w.state["step"][20] == 2 and w.state["step"][0] == 3 and w.glob[0]["applied"] == 3


def _fused_over(d, watch=()):
    """FusedAdam over parameters that ARE the misaligned views of the device world (moments too)."""
    w = d.w
    params, groups = [], []
    for i, (n, offs) in enumerate(zip(w.sizes, w.offsets)):
        view = lambda k, a: d.flat[k][offs[a]:offs[a] + n]
        p = torch.nn.Parameter(view("p", 0))
        p.grad = view("g", 1)
        params.append(p)
        groups.append(dict(params=[p], lr=w.rows[i]["lr"]))
    opt = O.FusedAdam(groups, lr=1e-2, watch=watch)
    for i, p in enumerate(params):
        n, offs = w.sizes[i], w.offsets[i]
        opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=d.flat["m"][offs[2]:offs[2] + n], exp_avg_sq=d.flat["v"][offs[3]:offs[3] + n])
    return opt, params


def test_guard_skips_without_storing_a_bit():
    """Check 10, through FusedAdam over the same table.  A NaN in the last element of the last tensor, then also +Inf in element 0 of
    the first, then also -Inf in the 4-byte tail of the chunk + 1 tensor: nonfinite is 1, 2, 3, `skipped` goes up by one each time, p, m,
    v and every tensor's words keep every bit, and _version of every parameter moves (as it does on the applied steps).  A watched buffer
    with one NaN is counted.  The clean step behind them equals the specification's, which never saw the bad ones."""
    d = DeviceWorld(seed=1)
    w = d.w
    watched = torch.zeros(d.chunk + 5, device=DEV)
    watched[d.chunk + 1] = float("nan")
    opt, params = _fused_over(d, watch=(watched, torch.ones(3, device=DEV)))
    d.state, d.glob = None, None

    def check(what):
        d.state, d.glob = opt._words, opt._global
        d.assert_equal(what)

    def step():
        v0 = [p._version for p in params]
        opt.step()
        assert all(p._version > a for p, a in zip(params, v0)), "a parameter's _version did not move"

    d.new_gradients()
    step()
    O.fused_adam_numpy(w.rows, w.state, w.glob, sumsq=opt.health()["sumsq"])
    w.glob[0]["watch_nonfinite"] = 1
    assert opt.health()["watch_nonfinite"] == 1 and opt.health()["applied"] == 1
    check("applied step")
    d.new_gradients()
    last, c1 = len(w.sizes) - 1, 13
    assert w.sizes[c1] == d.chunk + 1
    plants = [(last, w.sizes[last] - 1, float("nan")), (0, 0, float("inf")), (c1, d.chunk, float("-inf"))]
    for k, (i, e, value) in enumerate(plants, 1):
        d.flat["g"][w.offsets[i][1] + e] = value
        step()
        h = opt.health()
        assert (h["nonfinite"], h["skipped"], h["applied"], h["apply"]) == (k, k, 1, 0), h
        w.glob[0]["nonfinite"], w.glob[0]["skipped"], w.glob[0]["apply"], w.glob[0]["sumsq"] = k, k, 0, h["sumsq"]
        check(f"skipped step {k}")
    d.new_gradients()
    step()
    O.fused_adam_numpy(w.rows, w.state, w.glob, sumsq=opt.health()["sumsq"])
    w.glob[0]["watch_nonfinite"] = 1
    check("clean step behind the skipped ones")
    assert opt.health()["applied"] == 2 and int(w.state["step"].min()) == 2


def _lidar_trainer(fused):
    from lav_amd.train import LAV, TrainConfig
    torch.manual_seed(0)
    return LAV(TrainConfig(log_inference=False, fused_optim=fused), DEV, what="lidar")


def _moments(lav):
    opt = lav.lidar_optim
    return [opt.state[p][k] for g in opt.param_groups for p in g["params"] if p in opt.state for k in ("exp_avg", "exp_avg_sq")]


def test_resume_on_the_device_is_exact():
    """Check 11, in-process through lav_amd.train.state: two deterministic train_lidar steps with FusedAdam, capture, two more - against
    a fresh trainer, restore, the same two steps.  Every trained parameter and both moments of each agree in every bit."""
    import argparse
    from lav_amd.train import state as S
    from lav_amd.train import synthetic_lidar_batch
    from lav_amd.train.run import set_deterministic
    batches = [synthetic_lidar_batch(2, seed=40 + i, max_points=20000, num_objs=3) for i in range(2)]
    args = argparse.Namespace(batch_size=2, seed=0, lr=3e-4, synthetic=True, steps_per_epoch=2, fused_optim=True, max_grad_norm=None)

    def steps(lav, first):
        for s in range(first, first + 2):
            torch.manual_seed(1000 + s)
            lav.train_lidar(*batches[s % 2])

    set_deterministic(True)
    try:
        a = _lidar_trainer(True)
        assert isinstance(a.lidar_optim, O.FusedAdam) and len(a.lidar_optim.watch) > 0
        steps(a, 0)
        saved = S.capture(a, "lidar", args, 1, 2, (), 0, 1)
        saved = {k: (v if k != "models" else {n: {kk: vv.clone() for kk, vv in sd.items()} for n, sd in v.items()}) for k, v in saved.items()}
        saved["optimizer"] = __import__("copy").deepcopy(saved["optimizer"])
        steps(a, 2)
        torch.manual_seed(5)
        b = _lidar_trainer(True)
        assert S.restore(saved, b, "lidar", args, (), 0, 1) == (1, 2)
        steps(b, 2)
    finally:
        set_deterministic(False)
    assert a.lidar_optim.health()["applied"] == 4 and a.lidar_optim.health()["skipped"] == 0
    assert b.lidar_optim.health()["applied"] == 2
    pa, pb = list(a.student.parameters()), list(b.student.parameters())
    assert len(pa) == len(pb) and all(torch.equal(x, y) for x, y in zip(pa, pb))
    ma, mb = _moments(a), _moments(b)
    assert len(ma) == len(mb) > 100 and all(torch.equal(x, y) for x, y in zip(ma, mb))
    wa, wb = a.lidar_optim._rows_host(), b.lidar_optim._rows_host()
    assert U.bits(wa).tolist() == U.bits(wb).tolist()


def test_trainer_with_the_fused_step():
    """Check 12.  Three deterministic train_lidar steps with FusedAdam and with torch.optim.Adam from the same seeded weights.  The
    gradients of step 1 are identical, so after it every parameter is within the specification's distance from torch.optim.Adam
    (tests.optim_util.BAR at one step).  The losses of steps 2 and 3 are finite and within 1e-3 relative of each other: a sanity
    bound on two trainings that have begun to differ in the last bits, not a parity claim."""
    from lav_amd.train import synthetic_lidar_batch
    from lav_amd.train.run import set_deterministic
    batches = [synthetic_lidar_batch(2, seed=40 + i, max_points=20000, num_objs=3) for i in range(2)]
    set_deterministic(True)
    try:
        out = []
        for fused in (True, False):
            lav = _lidar_trainer(fused)
            losses, after1 = [], None
            for s in range(3):
                torch.manual_seed(1000 + s)
                losses.append(lav.train_lidar(*batches[s % 2])["loss"])
                if s == 0:
                    after1 = [p.detach().cpu().numpy().copy() for g in lav.lidar_optim.param_groups for p in g["params"]]
            out.append((losses, after1, lav.lidar_optim.param_groups[0]["lr"]))
    finally:
        set_deterministic(False)
    (lf, pf, lr), (lt, pt, _) = out
    assert lf[0] == lt[0]
    worst = max(U.ratio(x, y, 1, lr) for x, y in zip(pf, pt))
    print("worst ratio after step 1:", worst, "losses", lf, lt)
    assert worst <= U.BAR
    for x, y in zip(lf[1:], lt[1:]):
        assert math.isfinite(x) and math.isfinite(y) and abs(x - y) <= 1e-3 * abs(y)
