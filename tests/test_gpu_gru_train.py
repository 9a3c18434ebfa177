"""The training GRU (lav_amd/csrc/gru_seq.hip: lav_gru_seq_forward / lav_gru_seq_backward), its autograd function ops._GruSeq and the
train-mode decoders PlannerBase._cast_torch / _plan_torch against float64 (tests/gru_train_ref_util.py), at the shapes where the wave
split, the clamped re-reads, the row clamp and the buffer ping-pong take another path each.

Every bar is grad_bound of the float64 reference - 4 x max(one fp32 ulp of its largest value, the largest error of three float32
evaluations of the same inputs in other summation orders) - or torch.equal.  tests/test_gru_train_ref_host.py shows on the CPU that
two further float32 evaluations stay inside these bounds and that single mistakes move a compared tensor by more than 100 of them.
Every comparison prints a GRU_TRAIN_RATIO line: max|got - ref64| in units of that max(...) (limit 4).  Largest measured per group:
    kernels through the C ABI   1.42  (dh0, R3-T3-I4-H16-shared)
    ops.gru_seq and backward    3.64  (dw_ih, R5-T20-I4-H48-steps; next 3.27, dw_hh of R37-T7-I4-H512-steps)
    plan decoder                1.78  (dw_ih, plan-B5-nc2-cmd-1-T7-it2)
    cast decoder                1.60  (dw_ih, cast-B17-nc6-T10)"""
import math

import pytest
import torch
import torch.nn.functional as F

import lav_amd
from lav_amd import _lib, ops
from tests import gru_train_ref_util as U
from tests.gru_ref_util import CROP, PPM, W_KEYS, err_of, to

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GUARD, GUARD_FLOATS = 777.0, 4096
LAV_EWORKSPACE = -3
_ids = dict(ids=lambda c: c.id)


@pytest.fixture(autouse=True)
def _hip_gru(monkeypatch):
    monkeypatch.delenv("LAV_TRAIN_GRU", raising=False)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _within(got, m, what):
    assert tuple(got.shape) == tuple(m.ref64.shape), f"{what}: shape {tuple(got.shape)}, expected {tuple(m.ref64.shape)}"
    err = err_of(got.detach().cpu(), m.ref64)
    ratio = U.ratio_of(err, m)
    print(f"GRU_TRAIN_RATIO {what} err={err:.3e} bound={m.bound:.3e} ratio={ratio:.3f}")
    assert err <= m.bound, f"{what}: max|got - ref64| = {err:.3e} > bound {m.bound:.3e} (ratio {ratio:.2f}, limit 4)"


def _guarded(*shape):
    """(whole, view): a float32 buffer of `shape` followed by GUARD_FLOATS more floats, all of it filled with GUARD."""
    whole = torch.full((math.prod(shape) + GUARD_FLOATS,), GUARD, device=DEV)
    return whole, whole[:math.prod(shape)].view(shape)


def _guards_intact(bufs):
    return all(bool((whole[view.numel():] == GUARD).all()) for whole, view in bufs.values())


def _untouched(bufs):
    return all(bool((whole == GUARD).all()) for whole, _ in bufs.values())


_dev_cache = {}


def _dev(case):
    """The case's float32 inputs on the device; created once, never modified."""
    if case not in _dev_cache:
        inp = U.seq_case(case).inp if isinstance(case, U.SeqCase) else U.dec_case(case).inp
        _dev_cache[case] = to(inp, device=DEV)
    return _dev_cache[case]


# ------------------------------------------------------------------------------------------------ a. the kernels through the C ABI
def _forward_raw(d, R, T, H, per_step, bufs, x=True, tape=True):
    return _lib.load().lav_gru_seq_forward(d["x"].data_ptr() if x else None, int(per_step), d["h0"].data_ptr(), d["w_hh"].data_ptr(),
                                           d["b_hh"].data_ptr(), R, T, H, bufs["out"][1].data_ptr(), bufs["tape"][1].data_ptr() if tape else None,
                                           _stream())


def _backward_raw(d, fwd, R, T, H, bufs, ws_bytes, dout=True, ws=True):
    return _lib.load().lav_gru_seq_backward(d["dout"].data_ptr() if dout else None, fwd["tape"][1].data_ptr(), fwd["out"][1].data_ptr(),
                                            d["h0"].data_ptr(), d["w_hh_t"].data_ptr(), R, T, H, bufs["dx"][1].data_ptr(), bufs["dgh"][1].data_ptr(),
                                            bufs["dh0"][1].data_ptr(), bufs["ws"][1].data_ptr() if ws else None, ws_bytes, _stream())


def _buffers(R, T, H):
    need = _lib.load().lav_gru_seq_backward_workspace_bytes(R, H)
    assert need >= 2 * R * H * 4 and need % 4 == 0
    fwd = dict(out=_guarded(R, T, H), tape=_guarded(R, T, 4, H))
    bwd = dict(dx=_guarded(R, T, 3 * H), dgh=_guarded(R, T, 3 * H), dh0=_guarded(R, H), ws=_guarded(need // 4))
    return fwd, bwd, need


@pytest.mark.parametrize("case", U.SEQ_CASES, **_ids)
def test_kernels_equal_float64_and_stay_inside_their_buffers(case):
    """out, the tape and the raw dx, dgh, dh0 element by element; the backward runs on the kernel's own tape and out, as in training.
    The workspace is handed over filled with the guard pattern, not zeros: a read of a dh z buffer before its write would show."""
    m, d = U.seq_case(case).kernel, dict(_dev(case))
    R, T, H = case.R, case.T, case.H
    d["w_hh_t"] = d["w_hh"].t().contiguous()
    fwd, bwd, need = _buffers(R, T, H)
    assert _forward_raw(d, R, T, H, not case.shared, fwd) == 0, _lib.load().lav_last_error()
    assert _backward_raw(d, fwd, R, T, H, bwd, need) == 0, _lib.load().lav_last_error()
    torch.cuda.synchronize()
    for k in ("out", "tape"):
        _within(fwd[k][1], m[k], f"kernel {case.id} {k}")
    for k in ("dx", "dgh", "dh0"):
        _within(bwd[k][1], m[k], f"kernel {case.id} {k}")
    assert _guards_intact(fwd) and _guards_intact(bwd), "a kernel wrote behind the last element of a buffer"


# ------------------------------------------------------------------------------------------------ b. autograd
def _autograd_run(d, T):
    leaves = [d[k].detach().clone().requires_grad_(True) for k in U.AUTOGRAD_LEAVES]
    u, h0, w_ih, w_hh, b_ih, b_hh = leaves
    out = ops.gru_seq(F.linear(u, w_ih, b_ih), h0, w_hh, b_hh, T)
    grads = torch.autograd.grad((out * d["dout"]).sum(), leaves)
    return dict(out=out.detach(), **{"d" + k: g for k, g in zip(U.AUTOGRAD_LEAVES, grads)})


@pytest.mark.parametrize("case", U.SEQ_CASES, **_ids)
def test_gru_seq_and_its_gradients_equal_float64_autograd_twice(case):
    m, d = U.seq_case(case).autograd, _dev(case)
    got = _autograd_run(d, case.T)
    assert set(got) == set(m)
    for k in m:
        _within(got[k], m[k], f"autograd {case.id} {k}")
    again = _autograd_run(d, case.T)
    for k in m:
        assert torch.equal(got[k], again[k]), f"{k} differs between two runs by {float((got[k] - again[k]).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------------ c. bit-for-bit properties
def _seq_bits(d, T, dout=None, rows=slice(None)):
    """(out, dx, dh0) of ops.gru_seq on the projected input d["x"]; no synchronisation."""
    x, h0 = d["x"][rows].clone().requires_grad_(True), d["h0"][rows].clone().requires_grad_(True)
    out = ops.gru_seq(x, h0, d["w_hh"], d["b_hh"], T)
    dx, dh0 = torch.autograd.grad(out, [x, h0], grad_outputs=d["dout"][rows] if dout is None else dout)
    return out.detach(), dx, dh0


@pytest.mark.parametrize("case", [U.SEQ_CASES[i] for i in (1, 3, 6)], **_ids)
def test_forward_without_a_tape_is_the_taped_forward(case):
    d = _dev(case)
    taped = _seq_bits(d, case.T)[0]
    with torch.no_grad():
        plain = ops.gru_seq(d["x"], d["h0"], d["w_hh"], d["b_hh"], case.T)
    assert not plain.requires_grad and torch.equal(plain, taped)


@pytest.mark.parametrize("case", [c for c in U.SEQ_CASES if c.shared], **_ids)
def test_shared_input_is_the_expanded_input(case):
    d = _dev(case)
    assert d["x"].dim() == 2
    with torch.no_grad():
        shared = ops.gru_seq(d["x"], d["h0"], d["w_hh"], d["b_hh"], case.T)
        per_step = ops.gru_seq(d["x"][:, None].expand(-1, case.T, -1).contiguous(), d["h0"], d["w_hh"], d["b_hh"], case.T)
    assert torch.equal(shared, per_step)


def test_rows_do_not_depend_on_their_batch():
    """R = 17: the full row tile and the one-row second workgroup, each as a batch of its own (the one row then sits in lane 0 of a
    tile whose other rows are clamped re-reads of it)."""
    case = U.SEQ_CASES[3]
    assert case.R == 17
    d = _dev(case)
    full = _seq_bits(d, case.T)
    for rows in (slice(0, 16), slice(16, 17)):
        part = _seq_bits(d, case.T, rows=rows)
        for name, a, b in zip(("out", "dx", "dh0"), part, full):
            assert torch.equal(a, b[rows]), f"{name} of rows {rows} depends on the rest of the batch"


def test_a_strided_dout_is_its_contiguous_copy():
    case = U.SEQ_CASES[3]
    d = _dev(case)
    strided = d["dout"].transpose(0, 1).contiguous().transpose(0, 1)
    assert not strided.is_contiguous() and torch.equal(strided, d["dout"])
    want = _seq_bits(d, case.T)
    for a, b in zip(_seq_bits(d, case.T, dout=strided), want):
        assert torch.equal(a, b)
    # and a strided x and h0 (ops._GruSeq.forward's copies)
    x, h0 = (t.transpose(0, 1).contiguous().transpose(0, 1).requires_grad_(True) for t in (d["x"], d["h0"]))
    assert not x.is_contiguous() and not h0.is_contiguous()
    out = ops.gru_seq(x, h0, d["w_hh"], d["b_hh"], case.T)
    dx, dh0 = torch.autograd.grad(out, [x, h0], grad_outputs=d["dout"])
    for a, b in zip((out.detach(), dx, dh0), want):
        assert torch.equal(a, b)


def test_a_growing_workspace_changes_no_bits():
    """A small case, a large one and the small one again, back to back on a stream of their own: the backward's workspace is created
    for the first and replaced for the second, and each launch computes what it computes alone."""
    small, big = U.SEQ_CASES[1], U.SEQ_CASES[7]
    lib = _lib.load()
    assert lib.lav_gru_seq_backward_workspace_bytes(small.R, small.H) < lib.lav_gru_seq_backward_workspace_bytes(big.R, big.H)
    alone = {}
    for case in (small, big):
        alone[case] = _seq_bits(_dev(case), case.T)
        torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        key = ("gru_seq_bwd", alone[small][0].device, side.cuda_stream)
        assert key not in ops._workspaces
        runs = [(case, _seq_bits(_dev(case), case.T)) for case in (small, big, small)]
        side.synchronize()
        assert ops._workspaces[key].numel() >= lib.lav_gru_seq_backward_workspace_bytes(big.R, big.H)
        for i, (case, got) in enumerate(runs):
            for name, a, b in zip(("out", "dx", "dh0"), got, alone[case]):
                assert torch.equal(a, b), f"launch {i + 1} ({case.id}): {name} differs from the launch alone"


# ------------------------------------------------------------------------------------------------ d. empty and refused calls
@pytest.mark.parametrize("shared", [False, True])
def test_an_empty_batch_is_an_empty_result_with_zero_weight_gradients(shared):
    T, I, H = 5, 4, 32
    d = to(U.seq_inputs(1, T, I, H, shared, seed=31), device=DEV)
    d.update(u=d["u"][:0], h0=d["h0"][:0], dout=d["dout"][:0])
    got = _autograd_run(d, T)
    torch.cuda.synchronize()
    assert got["out"].shape == (0, T, H) and got["du"].shape == d["u"].shape and got["dh0"].shape == (0, H)
    for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
        assert got["d" + k].shape == d[k].shape and not got["d" + k].any(), k


def test_an_empty_batch_needs_no_pointers():
    lib = _lib.load()
    assert lib.lav_gru_seq_forward(None, 1, None, None, None, 0, 3, 16, None, None, _stream()) == 0
    assert lib.lav_gru_seq_backward(None, None, None, None, None, 0, 3, 16, None, None, None, None, 0, _stream()) == 0
    torch.cuda.synchronize()


_OK = dict(R=3, T=3, H=16)
_BAD_SIZES = [dict(H=0), dict(H=8), dict(H=24), dict(T=0), dict(R=-1)]
_over_ids = dict(ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))


def _refusal_setup(over):
    """Inputs and guard-filled outputs large enough for the valid call and for the refused sizes (were they launched)."""
    a = dict(_OK, **{k: v for k, v in over.items() if k in _OK})
    R, T, H = max(a["R"], _OK["R"]), max(a["T"], _OK["T"]), 32
    d = to(U.seq_inputs(R, T, 4, H, False, seed=32), device=DEV)
    d["w_hh_t"] = d["w_hh"].t().contiguous()
    return (a, d) + _buffers(R, T, H)


def _refused(rc, name, bufs, code=None):
    msg = _lib.load().lav_last_error()
    torch.cuda.synchronize()
    assert rc < 0 and (code is None or rc == code), f"{name} returned {rc}"
    assert msg and name.encode() in msg, f"{name} refused with the message {msg!r}"
    assert _untouched(bufs), f"{name} wrote although it refused the call"


@pytest.mark.parametrize("over", _BAD_SIZES + [dict(x=False)], **_over_ids)
def test_forward_refuses_before_any_launch(over):
    a, d, fwd, _, _ = _refusal_setup(over)
    rc = _forward_raw(d, a["R"], a["T"], a["H"], True, fwd, x=over.get("x", True))
    _refused(rc, "lav_gru_seq_forward", fwd)


@pytest.mark.parametrize("over", _BAD_SIZES + [dict(dout=False), dict(ws=False), dict(ws_short=1)], **_over_ids)
def test_backward_refuses_before_any_launch(over):
    a, d, fwd, bwd, _ = _refusal_setup(over)
    need = _lib.load().lav_gru_seq_backward_workspace_bytes(_OK["R"], _OK["H"])
    rc = _backward_raw(d, fwd, a["R"], a["T"], a["H"], bwd, need - over.get("ws_short", 0), dout=over.get("dout", True), ws=over.get("ws", True))
    _refused(rc, "lav_gru_seq_backward", bwd, code=LAV_EWORKSPACE if "ws_short" in over else None)


def test_gru_seq_raises_on_shapes_that_do_not_fit():
    case = U.SEQ_CASES[1]
    d, (R, T, H) = _dev(case), (case.R, case.T, case.H)
    per_step = d["x"][:, None].expand(-1, T, -1).contiguous()
    before = dict(ops.train_work)
    for x in (d["x"][:, :-1], per_step[:, :-1], per_step[:, :, :-1], per_step[None], d["x"][:-1]):
        with pytest.raises(RuntimeError, match="gru_seq"):
            ops.gru_seq(x, d["h0"], d["w_hh"], d["b_hh"], T)
    for w_hh in (d["w_hh"].t().contiguous(), d["w_hh"][:-1], d["w_hh"][:, :-1]):
        with pytest.raises(RuntimeError, match="gru_seq"):
            ops.gru_seq(d["x"], d["h0"], w_hh, d["b_hh"], T)
    assert ops.train_work == before   # refused in Python: no call was made


# ------------------------------------------------------------------------------------------------ e. the train-mode decoders
_GRU_NAMES = dict(w_ih="weight_ih_l0", w_hh="weight_hh_l0", b_ih="bias_ih_l0", b_hh="bias_hh_l0")


def _planner(case):
    kw = dict(num_plan_iter=case.iters) if isinstance(case, U.PlanDecCase) else {}
    model = lav_amd.BEVPlanner(num_plan=case.T, num_cmds=case.num_cmds, **kw).train().to(DEV)
    assert model.plan_gru.hidden_size == U.PLAN_H and model.cast_grus[0].hidden_size == U.CAST_H and model.cast_grus[0].input_size == U.CAST_E
    return model


def _grad_of(p):
    return torch.zeros_like(p) if p.grad is None else p.grad


def _no_gradient(modules):
    return all(p.grad is None or not p.grad.any() for mod in modules for p in mod.parameters())


@pytest.mark.parametrize("case", U.PLAN_DEC_CASES, **_ids)
def test_train_mode_plan_equals_float64_autograd(case):
    """The plan GRU and its Linear are shared by all commands, so cmd >= 0 leaves none of their parameters out: it takes one
    command's rows, and the gradients of all six tensors are compared in full.  What a plan call does leave out are the cast decoders
    (cast_locs is a constant): their parameters get no gradient, as on the reference's side, where they do not occur."""
    m, d = U.dec_case(case).m, _dev(case)
    model = _planner(case)
    with torch.no_grad():
        for k, name in _GRU_NAMES.items():
            getattr(model.plan_gru, name).copy_(d["w"][k])
        model.plan_mlp.weight.copy_(d["w"]["mlp_w"])
        model.plan_mlp.bias.copy_(d["w"]["mlp_b"])
    embd, nxp = d["embd"].clone().requires_grad_(True), d["nxp"].clone().requires_grad_(True)
    before = ops.train_work["gru_seq_forward_flops"]
    out = model.plan(embd, nxp, d["cast_locs"], PPM, CROP, case.cmd)
    assert ops.train_work["gru_seq_forward_flops"] > before, "the plan decoder did not run lav_gru_seq_forward"
    (out * d["dout"]).sum().backward()
    got = dict(out=out, dembd=embd.grad, dnxp=nxp.grad, dmlp_w=_grad_of(model.plan_mlp.weight), dmlp_b=_grad_of(model.plan_mlp.bias),
               **{"d" + k: _grad_of(getattr(model.plan_gru, name)) for k, name in _GRU_NAMES.items()})
    assert set(got) == set(m)
    for k in m:
        _within(got[k], m[k], f"decoder {case.id} {k}")
    assert _no_gradient([model.cast_grus, model.cast_mlps, model.cast_cmd_pred, model.bev_conv_emb])


@pytest.mark.parametrize("case", U.CAST_DEC_CASES, **_ids)
def test_train_mode_cast_equals_float64_autograd(case):
    """Six GRUs run as one with a block-diagonal recurrent matrix: every command's own parameters against the reference's stacked ones."""
    m, d = U.dec_case(case).m, _dev(case)
    model = _planner(case)
    with torch.no_grad():
        for c in range(case.num_cmds):
            for k, name in _GRU_NAMES.items():
                getattr(model.cast_grus[c], name).copy_(d["w"][k][c])
            model.cast_mlps[c].weight.copy_(d["w"]["mlp_w"][c])
            model.cast_mlps[c].bias.copy_(d["w"]["mlp_b"][c])
    embd = d["embd"].clone().requires_grad_(True)
    before = ops.train_work["gru_seq_forward_flops"]
    out = model.cast(embd)
    assert ops.train_work["gru_seq_forward_flops"] > before, "the cast decoders did not run lav_gru_seq_forward"
    (out * d["dout"]).sum().backward()
    stack = lambda params: torch.stack([_grad_of(p) for p in params])
    got = dict(out=out, dembd=embd.grad, dmlp_w=stack(mod.weight for mod in model.cast_mlps), dmlp_b=stack(mod.bias for mod in model.cast_mlps),
               **{"d" + k: stack(getattr(mod, name) for mod in model.cast_grus) for k, name in _GRU_NAMES.items()})
    assert set(got) == set(m) and tuple(W_KEYS) == tuple(d["w"])
    for k in m:
        _within(got[k], m[k], f"decoder {case.id} {k}")
    assert _no_gradient([model.plan_gru, model.plan_mlp, model.cast_cmd_pred, model.bev_conv_emb])
