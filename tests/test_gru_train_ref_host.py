"""The float64 references of the training GRU (tests/gru_train_ref_util.py) checked on the CPU, before any kernel is held to them:
the hand-written tape and backward equal torch.nn.GRU in double and float64 autograd; re-evaluated in float32 with hidden units and
rows renumbered at two further seeds they stay within grad_bound for every tensor of every case of the GPU tables (margin); and every
single mistake a kernel or its glue could make moves at least one compared tensor by more than 100 bounds (selectivity).  The wrong
variants below are copies of the references, never the project's code.  Run with -s for the GRU_TRAIN_MARGIN / GRU_TRAIN_MOVED lines."""
import pytest
import torch

from tests import gru_train_ref_util as U
from tests.gru_ref_util import err_of, floor_of, gru_seq_ref, to

F32, F64 = U.F32, U.F64


# ------------------------------------------------------------------------------------------------ against nn.GRU and autograd
@pytest.mark.parametrize("R,T,I,H", [(5, 9, 4, 48), (3, 20, 24, 32)])
def test_tape_and_backward_refs_equal_nn_gru_and_autograd_in_double(R, T, I, H):
    d = to(U.seq_inputs(R, T, I, H, False, seed=21), F64)
    x = d["u"] @ d["w_ih"].T + d["b_ih"]
    out, tape = U.gru_tape_ref(x, d["h0"], d["w_hh"], d["b_hh"])
    dx, dgh, dh0 = U.gru_backward_ref(d["dout"], tape, out, d["h0"], d["w_hh"])
    h_prev = torch.cat([d["h0"][:, None], out[:, :-1]], 1)
    got = dict(out=out, dx=dx, dh0=dh0, dw_hh=dgh.flatten(0, 1).T @ h_prev.flatten(0, 1), db_hh=dgh.sum((0, 1)))
    # float64 autograd of gru_seq_ref on the projected input: W_ih = 1, b_ih = 0 makes its u the x of the kernels
    xl, h0l, wl, bl = (t.clone().requires_grad_(True) for t in (x, d["h0"], d["w_hh"], d["b_hh"]))
    o = gru_seq_ref(xl, h0l, torch.eye(3 * H, dtype=F64), wl, torch.zeros(3 * H, dtype=F64), bl)
    want = dict(zip(("dx", "dh0", "dw_hh", "db_hh"), torch.autograd.grad((o * d["dout"]).sum(), (xl, h0l, wl, bl))), out=o.detach())
    for k, v in want.items():
        assert got[k].shape == v.shape and (got[k] - v).abs().max().item() <= 1e-12, k
    # torch.nn.GRU in double
    gru = torch.nn.GRU(I, H, batch_first=True).double()
    with torch.no_grad():
        for p, k in zip(gru.parameters(), ("w_ih", "w_hh", "b_ih", "b_hh")):
            p.copy_(d[k])
    ul, h0l = d["u"].clone().requires_grad_(True), d["h0"].clone().requires_grad_(True)
    o, _ = gru(ul, h0l[None])
    (o * d["dout"]).sum().backward()
    want = dict(out=o.detach(), du=ul.grad, dh0=h0l.grad, dw_hh=gru.weight_hh_l0.grad, db_hh=gru.bias_hh_l0.grad, dw_ih=gru.weight_ih_l0.grad,
                db_ih=gru.bias_ih_l0.grad)
    got.update(du=dx @ d["w_ih"], dw_ih=dx.flatten(0, 1).T @ d["u"].flatten(0, 1), db_ih=dx.sum((0, 1)))
    for k, v in want.items():
        assert got[k].shape == v.shape and (got[k] - v).abs().max().item() <= 1e-12, k
    assert tape.shape == (R, T, 4, H) and torch.equal(tape[:, :, 2], torch.tanh(x[:, :, 2 * H:] + tape[:, :, 0] * tape[:, :, 3]))


def test_both_sequence_levels_are_one_function():
    """The autograd level from u and the kernel level from the float32 x differ only by the rounding of x: in float64, fed the same
    x, the kernel level's tensors give the autograd level's; checked on the shared-input case, where dx is summed over the steps."""
    case = U.SeqCase(3, 5, 8, 32, True, seed=22)
    inp = U.seq_inputs(*case)
    inp["x"] = None
    d = to(inp, F64)
    d["x"] = d["u"] @ d["w_ih"].T + d["b_ih"]
    got, want = _glue(U.kernel_eval(d, F64), d, None), U.autograd_eval({k: v for k, v in inp.items() if k != "x"}, F64)
    for k, v in want.items():
        assert err_of(got[k], v) <= floor_of(v), k   # (float64 on both sides: another order of the same terms)


# ------------------------------------------------------------------------------------------------ margin
def _margin(name, case, evaluate, renumber, inp, m):
    worst = 0.0
    for seed in U.MARGIN_SEEDS:
        again = U.renumbered(evaluate, renumber, inp, seed)
        assert set(again) == set(m)
        for k, mm in m.items():
            err = err_of(again[k], mm.ref64)
            ratio = U.ratio_of(err, mm)
            worst = max(worst, ratio)
            print(f"GRU_TRAIN_MARGIN {name} {case.id} {k} seed={seed} err={err:.3e} samples={'/'.join(f'{e:.2e}' for e in mm.errs32)} "
                  f"floor={mm.floor:.3e} ratio={ratio:.3f}")
            assert err <= mm.bound, f"{name} {case.id} {k}, renumbering {seed}: {err:.3e} > bound {mm.bound:.3e} (ratio {ratio:.2f}, limit 4)"
    print(f"GRU_TRAIN_MARGIN_WORST {name} {case.id} {worst:.3f}")


@pytest.mark.parametrize("case", U.SEQ_CASES, ids=lambda c: c.id)
def test_sequence_bounds_hold_for_two_more_summation_orders(case):
    m = U.seq_case(case)
    _margin("kernel", case, U.kernel_eval, U.renumber_seq, m.inp, m.kernel)
    _margin("autograd", case, U.autograd_eval, U.renumber_seq, m.inp, m.autograd)


@pytest.mark.parametrize("case", U.DEC_CASES, ids=lambda c: c.id)
def test_decoder_bounds_hold_for_two_more_summation_orders(case):
    m = U.dec_case(case)
    _margin("decoder", case, *U.dec_level(case), m.inp, m.m)


def test_renumbering_is_exact_in_its_bookkeeping():
    """In float64 a renumbered evaluation, put back, is the reference to float64 rounding (far inside one fp32 ulp, the bar here):
    the index maps of renumber_* are right (a wrong map would show as a margin failure of order one, but this names it)."""
    case = U.SEQ_CASES[4]
    m = U.seq_case(case)
    for evaluate, meas in ((U.kernel_eval, m.kernel), (U.autograd_eval, m.autograd)):
        new, back = U.renumber_seq(m.inp, 5)
        for k, v in back(evaluate(new, F64)).items():
            assert err_of(v, meas[k].ref64) <= meas[k].floor, k
    for case in (U.PLAN_DEC_CASES[2], U.CAST_DEC_CASES[0]):
        m = U.dec_case(case)
        evaluate, renumber = U.dec_level(case)
        new, back = renumber(m.inp, 5)
        for k, v in back(evaluate(new, F64)).items():
            assert err_of(v, m.m[k].ref64) <= m.m[k].floor, k


# ------------------------------------------------------------------------------------------------ selectivity
FORWARD_MISTAKES = ("gates_r_z_exchanged", "update_weights_exchanged")
BACKWARD_MISTAKES = ("da_z_from_the_state_after_the_step", "da_r_with_n_for_gh_n", "dgh_n_without_r", "dh_z_carry_dropped",
                     "dh_z_carry_from_the_other_buffer")
GLUE_MISTAKES = ("dx_not_summed_over_steps",)


def _tape_wrong(x, h0, w_hh, b_hh, wrong):
    """gru_tape_ref with one mistake."""
    H = h0.shape[1]
    h, hs, tape = h0, [], []
    for t in range(x.shape[1]):
        gh = h @ w_hh.T + b_hh
        r = torch.sigmoid(x[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(x[:, t, H:2 * H] + gh[:, H:2 * H])
        if wrong == "gates_r_z_exchanged":
            r, z = z, r
        n = torch.tanh(x[:, t, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * h + z * n if wrong == "update_weights_exchanged" else (1 - z) * n + z * h
        hs.append(h)
        tape.append(torch.stack([r, z, n, gh[:, 2 * H:]], 1))
    return torch.stack(hs, 1), torch.stack(tape, 1)


def _backward_wrong(dout, tape, out, h0, w_hh, wrong):
    """gru_backward_ref with one mistake.  The carry into step t is dh z of step t + 1 plus dgh_{t+1} W_hh; the kernel keeps the
    first part in two buffers that alternate, so "the other buffer" holds dh z of step t + 2 (zeros, as the workspace is created,
    before its first write)."""
    T = dout.shape[1]
    dhz = [torch.zeros_like(h0), torch.zeros_like(h0)]   # [0]: of the step just done, [1]: of the one before
    gemm = torch.zeros_like(h0)
    dx, dgh = [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        dh = dout[:, t] + gemm + _carry(dhz, wrong)
        r, z, n, ghn = tape[:, t].unbind(1)
        hp = out[:, t - 1] if t else h0
        da_n = dh * (1 - z) * (1 - n * n)
        da_z = dh * ((out[:, t] if wrong == "da_z_from_the_state_after_the_step" else hp) - n) * z * (1 - z)
        da_r = da_n * (n if wrong == "da_r_with_n_for_gh_n" else ghn) * r * (1 - r)
        dx[t] = torch.cat([da_r, da_z, da_n], 1)
        dgh[t] = torch.cat([da_r, da_z, da_n if wrong == "dgh_n_without_r" else da_n * r], 1)
        dhz, gemm = [dh * z, dhz[0]], dgh[t] @ w_hh
    return torch.stack(dx, 1), torch.stack(dgh, 1), gemm + _carry(dhz, wrong)


def _carry(dhz, wrong):
    return 0 if wrong == "dh_z_carry_dropped" else dhz[1] if wrong == "dh_z_carry_from_the_other_buffer" else dhz[0]


def _kernel_wrong(inp, wrong):
    d = to(inp, F64)
    out, tape = _tape_wrong(U._per_step(d["x"], d["dout"].shape[1]), d["h0"], d["w_hh"], d["b_hh"], wrong)
    dx, dgh, dh0 = _backward_wrong(d["dout"], tape, out, d["h0"], d["w_hh"], wrong)
    return dict(out=out, tape=tape, dx=dx, dgh=dgh, dh0=dh0)


def _glue(k, d, wrong):
    """What the autograd function and F.linear's backward make of the kernel level's tensors (ops._GruSeq's arithmetic, restated)."""
    shared = d["u"].dim() == 2
    dxs = k["dx"] if not shared else k["dx"][:, 0] if wrong == "dx_not_summed_over_steps" else k["dx"].sum(1)
    h_prev = torch.cat([d["h0"][:, None], k["out"][:, :-1]], 1)
    flat = lambda t: t.reshape(-1, t.shape[-1])
    return dict(out=k["out"], du=dxs @ d["w_ih"], dh0=k["dh0"], dw_ih=flat(dxs).T @ flat(d["u"]), dw_hh=flat(k["dgh"]).T @ flat(h_prev),
                db_ih=flat(dxs).sum(0), db_hh=flat(k["dgh"]).sum(0))


def _moved(got, m):
    """The largest movement of a compared tensor in bounds, and its name."""
    return max((U.ratio_of(err_of(got[k], mm.ref64), mm) / 4.0, k) for k, mm in m.items())


def _mistakes(case):
    """The mistakes that are not the identity at this case's shape.  Both forward mistakes and the first four backward mistakes
    change a term that every step has, so they are the identity at no shape.  The carry from the other buffer is the identity at no
    shape either: even at T = 1 the last launch reads dh z of step 0 from the buffer that step did not write.  (A mix-up that only
    exchanges the two buffers' roles consistently is the identity at every T and is not a mistake; what T > 2 adds is that the wrong
    buffer then holds a live earlier value, not zeros.)  dx not summed over the steps is the identity when the input is per step
    or T = 1."""
    return FORWARD_MISTAKES + BACKWARD_MISTAKES + (GLUE_MISTAKES if case.shared and case.T > 1 else ())


def test_the_wrong_copies_are_the_references_without_their_mistake():
    for case in (U.SEQ_CASES[3], U.SEQ_CASES[4]):
        m = U.seq_case(case)
        got = _kernel_wrong(m.inp, None)
        for k, mm in m.kernel.items():   # (the copy adds the two parts of the carry one by one: float64 rounding apart)
            assert err_of(got[k], mm.ref64) <= mm.floor, k
        d = to(m.inp, F64)
        d["x"] = d["u"] @ d["w_ih"].T + d["b_ih"]
        for k, v in _glue(_kernel_wrong(d, None), d, None).items():
            assert err_of(v, m.autograd[k].ref64) <= m.autograd[k].floor, k   # (another summation order of the same float64 terms)


@pytest.mark.parametrize("case", U.SEQ_CASES, ids=lambda c: c.id)
def test_sequence_bounds_tell_every_mistake(case):
    m = U.seq_case(case)
    d = to(m.inp, F64)
    d["x"] = d["u"] @ d["w_ih"].T + d["b_ih"]   # the autograd level projects in float64
    for wrong in _mistakes(case):
        at_kernel = _moved(_kernel_wrong(m.inp, wrong), m.kernel) if wrong not in GLUE_MISTAKES else None
        at_autograd = _moved(_glue(_kernel_wrong(d, wrong), d, wrong), m.autograd)
        print(f"GRU_TRAIN_MOVED {case.id} {wrong}: kernel level {at_kernel}, autograd level {at_autograd} (bounds, tensor)")
        assert at_kernel is None or at_kernel[0] > 100, f"{wrong} moves no kernel-level tensor by 100 bounds: {at_kernel}"
        assert at_autograd[0] > 100, f"{wrong} moves no autograd-level tensor by 100 bounds: {at_autograd}"
        if wrong in BACKWARD_MISTAKES + GLUE_MISTAKES:   # (the forward is untouched: only gradients can tell these)
            assert err_of(_kernel_wrong(m.inp, wrong)["out"], m.kernel["out"].ref64) == 0


# ---- decoders: the glue around the GRU (block-diagonal assembly of the cast GRUs, branch-major batching of the plan GRU)
def _cast_wrong(embd, w, T, wrong):
    """cast_ref on a (B, E) embedding with one mistake."""
    B, E = embd.shape
    nc = w["w_ih"].shape[0]
    u = embd[:, None, :].expand(B, T, E)
    per_cmd = []
    for c in range(nc):
        ch = (c + 1) % nc if wrong == "recurrent_block_of_the_next_command" else c
        cm = (c + 1) % nc if wrong == "mlp_of_the_next_command" else c
        hs = gru_seq_ref(u, embd.new_zeros(B, w["w_hh"].shape[2]), w["w_ih"][c], w["w_hh"][ch], w["b_ih"][c], w["b_hh"][c])
        per_cmd.append(torch.cumsum(hs @ w["mlp_w"][cm].T + w["mlp_b"][cm], 1))
    return torch.stack(per_cmd, 1)


def _plan_wrong(embd, nxp, cast_locs, w, iters, cmd, ppm, crop, wrong):
    """plan_ref with one mistake of the branch-major batching: rows ordered (command, sample) read back as (sample, command)."""
    B, H = embd.shape
    T = cast_locs.shape[2]
    cmds = [cmd] if cmd >= 0 else list(range(cast_locs.shape[1]))
    NC = len(cmds)
    target = (nxp * ppm / crop * 2 - 1)[:, None, None, :].expand(B, NC, T, 2)
    h0 = embd[:, None, :].expand(B, NC, H).reshape(B * NC, H)
    loc, res = cast_locs[:, cmds], []
    for _ in range(iters):
        u = torch.cat([target, loc], -1).reshape(B * NC, T, 4)
        hs = gru_seq_ref(u, h0, w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"])
        step = torch.cumsum(hs @ w["mlp_w"].T + w["mlp_b"], 1)
        step = step.reshape(NC, B, T, 2).transpose(0, 1) if wrong == "rows_read_back_command_major" else step.reshape(B, NC, T, 2)
        loc = step + loc
        res.append(loc)
    return torch.stack(res, 1)


def _dec_wrong(case, inp, wrong):
    d = U._leaf(U._copy(inp, F64))
    if isinstance(case, U.PlanDecCase):
        out = _plan_wrong(d["embd"], d["nxp"], d["cast_locs"], d["w"], case.iters, case.cmd, U.PPM, U.CROP, wrong)
    else:
        out = _cast_wrong(d["embd"], d["w"], case.T, wrong)
    return U._dec_grads(out, d["dout"], d)


def _dec_mistakes(case):
    """Exchanging commands is the identity with one command, and that of the recurrent blocks also at T = 1, where the only step
    starts from h0 = 0; reading the rows back in the other order is the identity with one sample or one command."""
    if isinstance(case, U.PlanDecCase):
        return ("rows_read_back_command_major",) if case.B > 1 and case.NC > 1 else ()
    return (("recurrent_block_of_the_next_command",) if case.T > 1 else ()) + ("mlp_of_the_next_command",) if case.num_cmds > 1 else ()


@pytest.mark.parametrize("case", U.DEC_CASES, ids=lambda c: c.id)
def test_decoder_bounds_tell_every_mistake(case):
    m = U.dec_case(case)
    for k, v in _dec_wrong(case, m.inp, None).items():
        assert torch.equal(v, m.m[k].ref64), k
    for wrong in _dec_mistakes(case):
        got = _dec_wrong(case, m.inp, wrong)
        moved = _moved(got, m.m)
        grads = _moved({k: v for k, v in got.items() if k != "out"}, {k: v for k, v in m.m.items() if k != "out"})
        print(f"GRU_TRAIN_MOVED {case.id} {wrong}: {moved}, gradients alone {grads} (bounds, tensor)")
        assert moved[0] > 100 and grads[0] > 100, f"{wrong}: {moved}, {grads}"
