"""The specification of the fused Adam step (lav_amd.train.optim.fused_adam_numpy) and FusedAdam's CPU path, without a GPU: its
distance from torch.optim.Adam, the guard's semantics, the state_dict round trips between the two classes, the refusals."""
import copy

import numpy as np
import pytest
import torch

from lav_amd.train import optim as O
from tests import optim_util as U


@pytest.mark.parametrize("lr", [3e-4, 1e-2])
def test_specification_against_torch_adam(lr):
    """Check 1: one 200 000-element tensor, 200 steps, parameters of magnitude 1e-4 .. 10, gradients of magnitude 1e-12 .. 1e2 re-drawn
    every step, a fifth of them zero on every seventh.  The two are not bit-identical (torch uses lerp, divides by sqrt(bias
    correction 2) and takes beta ** step).  After every step s, max |p_spec - p_torch| / (s (ulp(p) + 2^-22 lr)) stays under
    tests.optim_util.BAR, twice the worst ratio measured (1.1475 at lr 3e-4, 1.1364 at lr 1e-2, both at s = 2)."""
    rng = np.random.default_rng(1)
    n = 200000
    p0 = U.log_uniform(rng, 1e-4, 10.0, n)
    row, st, gl = U.one_tensor(p0, lr=lr), O.new_state(1), np.zeros(1, O.GLOBAL_DTYPE)
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([q], lr=lr)
    worst = 0.0
    for s in range(1, 201):
        g = U.wide_gradient(rng, n, s)
        U.spec_step([row], st, gl, [g])
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        worst = max(worst, U.ratio(row["p"], q.detach().numpy(), s, lr))
    print(f"lr {lr}: worst ratio {worst}")
    assert st["step"][0] == 200 and gl[0]["applied"] == 200 and gl[0]["skipped"] == 0
    assert worst <= U.BAR
    assert U.MEASURED_RATIO <= 2


def _small(rng, sizes=(5, 64, 1000)):
    rows = [U.one_tensor(U.log_uniform(rng, 1e-3, 10.0, n), m=rng.standard_normal(n) * 0.1, v=rng.random(n) * 1e-2, lr=1e-2, state=i)
            for i, n in enumerate(sizes)]
    return rows, O.new_state(len(rows)), np.zeros(1, O.GLOBAL_DTYPE)


def _snapshot(rows, st):
    return [U.bits(r[k]).copy() for r in rows for k in "pmv"] + [U.bits(st).copy()]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_specification_guard_semantics():
    """Check 2: a planted NaN, +Inf or -Inf leaves p, m, v and every tensor's step count and powers unchanged in every bit, counts
    exactly the planted elements and adds one to `skipped`; the next clean step equals a run that never saw the bad one; a tensor
    without a gradient keeps its own step count."""
    rng = np.random.default_rng(2)
    rows, st, gl = _small(rng)
    twin, st2, gl2 = copy.deepcopy(rows), st.copy(), gl.copy()
    clean = [U.log_uniform(rng, 1e-6, 10.0, r["p"].size) for r in rows]
    U.spec_step(rows, st, gl, clean)
    U.spec_step(twin, st2, gl2, clean)
    before = _snapshot(rows, st)
    planted = 0
    for k, (i, e, value) in enumerate([(2, 999, np.nan), (0, 0, np.inf), (1, 63, -np.inf)], 1):
        bad = [g.copy() for g in clean]
        bad[i][e] = value
        bad[2][5] = value                   # a second element of the same kind
        U.spec_step(rows, st, gl, bad)
        assert gl[0]["nonfinite"] == 2 and gl[0]["skipped"] == k and gl[0]["applied"] == 1 and gl[0]["apply"] == 0
        assert _same(before, _snapshot(rows, st)), f"a skipped step stored something ({value})"
    nxt = [U.log_uniform(rng, 1e-6, 10.0, r["p"].size) for r in rows]
    U.spec_step(rows, st, gl, nxt)
    U.spec_step(twin, st2, gl2, nxt)
    assert _same(_snapshot(rows, st), _snapshot(twin, st2)) and gl[0]["applied"] == 2 == gl2[0]["applied"] and gl2[0]["skipped"] == 0
    # a tensor without a gradient is left out of the step and keeps its own count
    U.spec_step(rows, st, gl, [nxt[0], None, nxt[2]])
    assert st["step"].tolist() == [3, 2, 3] and st["beta1_power"][1] == 0.9 * 0.9 and st["beta1_power"][0] == 0.9 * 0.9 * 0.9
    assert np.array_equal(U.bits(rows[1]["p"]), U.bits(twin[1]["p"]))


def test_specification_clip_equals_clip_grad_norm_then_adam():
    """Check 2, the clip: max_norm = norm / 3 scales as clip_grad_norm_ followed by torch.optim.Adam does, within check 1's bar."""
    rng = np.random.default_rng(3)
    sizes, lr = (5, 64, 1000), 1e-2
    rows = [U.one_tensor(U.log_uniform(rng, 1e-3, 10.0, n), lr=lr, state=i) for i, n in enumerate(sizes)]
    st, gl = O.new_state(3), np.zeros(1, O.GLOBAL_DTYPE)
    qs = [torch.nn.Parameter(torch.from_numpy(r["p"].copy())) for r in rows]
    opt = torch.optim.Adam(qs, lr=lr)
    for s in range(1, 6):
        gs = [U.log_uniform(rng, 1e-3, 10.0, n) for n in sizes]
        norm = float(np.sqrt(sum(np.sum(g.astype(np.float64) ** 2) for g in gs)))
        U.spec_step(rows, st, gl, gs, max_norm=norm / 3)
        assert abs(float(gl[0]["clip"]) - 1 / 3) < 1e-6
        for q, g in zip(qs, gs):
            q.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grad_norm_(qs, norm / 3)
        opt.step()
        worst = max(U.ratio(r["p"], q.detach().numpy(), s, lr) for r, q in zip(rows, qs))
        assert worst <= U.BAR, (s, worst)


def _params(rng, sizes=((7, 3), (64,), (10, 10, 10))):
    return [U.log_uniform(rng, 1e-3, 10.0, int(np.prod(s))).reshape(s) for s in sizes]


def _run(cls, values, grads, state=None, lr=1e-2):
    """Steps a fresh optimiser of `cls` over copies of `values` through `grads`; returns (optimiser, parameters)."""
    ps = [torch.nn.Parameter(torch.from_numpy(v.copy())) for v in values]
    opt = cls(ps, lr=lr)
    if state is not None:
        opt.load_state_dict(copy.deepcopy(state))
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
    return opt, ps


def _values(ps):
    return [p.detach().numpy().copy() for p in ps]


def test_state_dict_round_trips_between_the_two_classes():
    """Check 3: torch.optim.Adam -> FusedAdam -> torch.optim.Adam, and FusedAdam -> torch.optim.Adam -> FusedAdam (which keeps the two
    powers without complaint).  After the round trip the next step agrees with the uninterrupted one: bit for bit within the same
    class, within check 1's bar across classes.  The layout is torch's: step, exp_avg, exp_avg_sq, plus beta1_power / beta2_power."""
    rng = np.random.default_rng(4)
    values, lr = _params(rng), 1e-2
    grads = [[U.log_uniform(rng, 1e-4, 10.0, v.size).reshape(v.shape) for v in values] for _ in range(4)]
    for cls, other in ((torch.optim.Adam, O.FusedAdam), (O.FusedAdam, torch.optim.Adam)):
        _, straight = _run(cls, values, grads)
        three, ps3 = _run(cls, values, grads[:3])
        sd3, at3 = copy.deepcopy(three.state_dict()), _values(ps3)
        if cls is O.FusedAdam:
            assert set(sd3["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "beta1_power", "beta2_power"}
            assert sd3["state"][0]["beta1_power"] == 0.9 * 0.9 * 0.9 and float(sd3["state"][0]["step"]) == 3.0
        middle, crossed = _run(other, at3, grads[3:], state=sd3)                    # the other class takes the fourth step
        worst = max(U.ratio(a.detach().numpy(), b.detach().numpy(), 1, lr) for a, b in zip(crossed, straight))
        assert worst <= U.BAR, (cls.__name__, worst)
        there, _ = _run(other, at3, [], state=sd3)
        _, back = _run(cls, at3, grads[3:], state=there.state_dict())             # round trip, then the fourth step
        assert all(np.array_equal(U.bits(a.detach().numpy()), U.bits(b.detach().numpy())) for a, b in zip(back, straight)), cls.__name__
    # a torch.optim.Adam state has no powers: they are beta ** step
    adam, _ = _run(torch.optim.Adam, values, grads[:3])
    fused, _ = _run(O.FusedAdam, values, [], state=adam.state_dict())
    rows = fused._rows_host()
    assert rows["step"].tolist() == [3, 3, 3] and rows["beta1_power"][0] == 0.9 ** 3 and rows["beta2_power"][0] == 0.999 ** 3


def test_fused_adam_cpu_path_is_the_specification_and_counts_per_tensor():
    rng = np.random.default_rng(5)
    values = _params(rng)
    grads = [[U.log_uniform(rng, 1e-4, 10.0, v.size).reshape(v.shape) for v in values] for _ in range(3)]
    ps = [torch.nn.Parameter(torch.from_numpy(v.copy())) for v in values]
    buf = torch.ones(9)
    opt = O.FusedAdam(ps, lr=1e-2, max_grad_norm=1.0, watch=(buf,))
    rows = [U.one_tensor(v.reshape(-1), lr=1e-2, state=i) for i, v in enumerate(values)]
    st, gl = O.new_state(3), np.zeros(1, O.GLOBAL_DTYPE)
    for k, gs in enumerate(grads):
        gs = list(gs)
        if k == 1:
            gs[1] = None                        # no gradient this step
        for p, g in zip(ps, gs):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        versions = [p._version for p in ps]
        opt.step()
        U.spec_step(rows, st, gl, [None if g is None else g.reshape(-1) for g in gs], max_norm=1.0)
        assert [p._version > v for p, v in zip(ps, versions)] == [g is not None for g in gs]
    assert all(np.array_equal(U.bits(p.detach().numpy().reshape(-1)), U.bits(r["p"])) for p, r in zip(ps, rows))
    h = opt.health()
    assert h["applied"] == 3 and h["skipped"] == 0 and h["clip"] < 1 and h["grad_norm"] == float(np.sqrt(gl[0]["sumsq"]))
    assert [int(opt.state_dict()["state"][i]["step"]) for i in range(3)] == [3, 2, 3]
    buf[4] = float("inf")
    ps[0].grad[0, 0] = float("nan")
    before = _values(ps)
    opt.step()
    h = opt.health()
    assert (h["skipped"], h["nonfinite"], h["watch_nonfinite"], h["apply"]) == (1, 1, 1, 0)
    assert all(np.array_equal(U.bits(a), U.bits(b)) for a, b in zip(before, _values(ps)))


def test_fused_adam_refusals():
    p = torch.nn.Parameter(torch.zeros(4))
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(weight_decay=1e-4)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            O.FusedAdam([p], **kw)
    with pytest.raises(ValueError, match="max_grad_norm"):
        O.FusedAdam([p], max_grad_norm=0.0)
    with pytest.raises(TypeError, match="float32"):
        O.FusedAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="dense"):
        O.FusedAdam([torch.nn.Parameter(torch.zeros(4, 4).t())])
    opt = O.FusedAdam([p])
    opt.param_groups[0]["weight_decay"] = 0.1       # (a loaded state, or a caller, may set it later)
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="weight_decay"):
        opt.step()


def test_optim_abi_sizes():
    """Host side of the C ABI: the chunk length is exported, the workspace grows with the chunks and refuses counts the calls refuse."""
    from lav_amd import _lib
    lib = _lib.load()
    chunk = O.chunk_length()
    assert chunk >= 256 and chunk % 4 == 0
    assert lib.lav_optim_workspace_bytes(1000, 10) >= 1010 * 12 and lib.lav_optim_workspace_bytes(0, 0) > 0
    assert lib.lav_optim_workspace_bytes(-1, 0) == 0 and lib.lav_optim_workspace_bytes(2 ** 31, 0) == 0
    rows = np.zeros(3, O.TENSOR_DTYPE)
    rows["numel"] = [1, chunk, chunk + 1]
    assert O.fill_chunks(rows, chunk) == 4 and rows["chunk0"].tolist() == [0, 1, 2]
