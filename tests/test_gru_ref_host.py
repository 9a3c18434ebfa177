"""The float64 reference of the GRU decoders (tests/gru_ref_util.py) checked on the CPU, before any kernel is held to it:
it equals the oracle and torch.nn.GRU in double; re-evaluated in fp32 with the hidden units renumbered it stays within the
bound of every case of the GPU tables (margin); and every single-index or single-sign mistake a kernel could make moves it by
more than 100 bounds (selectivity).  The wrong variants below are copies of the reference, never the project's code."""
import pytest
import torch

from oracle import bev as obev
from tests import gru_ref_util as U

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ against the oracle and nn.GRU
@pytest.mark.parametrize("H,B,num_cmds,T,iters", [(128, 3, 4, 9, 2), (64, 2, 6, 20, 3)])
def test_plan_ref_equals_the_oracle_in_float64(H, B, num_cmds, T, iters):
    d = U.to(U.plan_inputs(H, num_cmds, T, B, seed=11), F64)
    w = d["w"]
    sd = {"plan_gru.weight_ih_l0": w["w_ih"], "plan_gru.weight_hh_l0": w["w_hh"], "plan_gru.bias_ih_l0": w["b_ih"],
          "plan_gru.bias_hh_l0": w["b_hh"], "plan_mlp.weight": w["mlp_w"], "plan_mlp.bias": w["mlp_b"]}
    want = obev.plan(d["embd"], d["nxp"], d["cast_locs"], sd, pixels_per_meter=U.PPM, crop_size=U.CROP, num_cmds=num_cmds,
                     num_plan=T, num_plan_iter=iters)
    got = U.plan_ref(d["embd"], d["nxp"], d["cast_locs"], w, iters, -1, U.PPM, U.CROP)
    assert got.dtype == F64 and got.shape == (B, iters, num_cmds, T, 2)
    assert (got - want).abs().max().item() <= 1e-12
    for c in (0, num_cmds - 1):
        one = U.plan_ref(d["embd"], d["nxp"], d["cast_locs"], w, iters, c, U.PPM, U.CROP)
        assert one.shape == (B, iters, 1, T, 2) and (one[:, :, 0] - want[:, :, c]).abs().max().item() <= 1e-12


@pytest.mark.parametrize("E,B,num_cmds,T,hw", [(96, 3, 4, 9, (2, 3)), (320, 2, 6, 20, (1, 1))])
def test_cast_ref_equals_the_oracle_in_float64(E, B, num_cmds, T, hw):
    """oracle.bev.cast starts from a float32 h0 and does not run on float64 tensors as written: its parts do (gru_sequence,
    cast_cmd_pred, transform_points)."""
    d = U.to(U.cast_inputs(E, num_cmds, T, B, hw, seed=12), F64)
    w = d["w"]
    embd, cast, cmds = U.cast_ref(d["feat"], w, T, d["cmd_w"], d["cmd_b"], d["oris"], d["locs"])
    want_embd = d["feat"].mean((2, 3))
    assert (embd - want_embd).abs().max().item() <= 1e-12
    u = want_embd[:, None, :].expand(B, T, E)
    plain = torch.stack([torch.cumsum(obev.gru_sequence(u, torch.zeros(B, 64, dtype=F64), w["w_ih"][c], w["w_hh"][c], w["b_ih"][c], w["b_hh"][c])
                                      @ w["mlp_w"][c].T + w["mlp_b"][c], 1) for c in range(num_cmds)], 1)
    assert (U.cast_ref(d["feat"], w, T)[1] - plain).abs().max().item() <= 1e-12
    want = obev.transform_points(plain, d["oris"][:, None].expand(B, num_cmds)) + d["locs"][:, None, None]
    assert (cast - want).abs().max().item() <= 1e-12
    want_cmds = obev.cast_cmd_pred(want_embd, {"cast_cmd_pred.0.weight": d["cmd_w"], "cast_cmd_pred.0.bias": d["cmd_b"]})
    assert (cmds - want_cmds).abs().max().item() <= 1e-12
    # a (B, E) input is the embedding itself
    assert torch.equal(U.cast_ref(want_embd, w, T)[1], U.cast_ref(want_embd[:, :, None, None], w, T)[1])


@pytest.mark.parametrize("I,H,R,T", [(4, 128, 5, 9), (96, 64, 3, 20)])
def test_gru_step_equals_nn_gru_in_double(I, H, R, T):
    g = torch.Generator().manual_seed(13)
    gru = torch.nn.GRU(I, H, batch_first=True).double()
    u, h0 = torch.randn(R, T, I, generator=g, dtype=F64), torch.randn(R, H, generator=g, dtype=F64)
    with torch.no_grad():
        want, _ = gru(u, h0[None])
        got = U.gru_seq_ref(u, h0, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)
    assert (got - want).abs().max().item() <= 1e-12


# ------------------------------------------------------------------------------------------------ margin
@pytest.mark.parametrize("case", U.PLAN_CASES, ids=lambda c: c.id)
def test_plan_bound_holds_for_another_summation_order(case):
    m = U.plan_case(case)
    for seed in (1, 2):
        again = U.plan_eval(U.permute_plan_hidden(m.inp, seed), case, torch.float32)
        err = U.err_of(again, m.ref64)
        assert err <= m.bound, f"permutation {seed}: {err:.3e} > bound {m.bound:.3e} (restatement {m.err32:.3e}, floor {m.floor:.3e})"


@pytest.mark.parametrize("case", U.CAST_CASES, ids=lambda c: c.id)
def test_cast_bound_holds_for_another_summation_order(case):
    m = U.cast_case(case)
    for seed in (1, 2):
        inp, back = U.permute_cast_hidden(m.inp, seed)
        embd, cast, cmds = U.cast_eval(inp, case, torch.float32)
        for name, got in (("embd", embd[:, back]), ("cast", cast), ("cmds", cmds)):
            mm = getattr(m, name)
            if mm is not None:
                err = U.err_of(got, mm.ref64)
                assert err <= mm.bound, f"{name}, permutation {seed}: {err:.3e} > bound {mm.bound:.3e} (restatement {mm.err32:.3e})"


# ------------------------------------------------------------------------------------------------ selectivity
def _gru_seq_wrong(u, h0, w_ih, w_hh, b_ih, b_hh, wrong):
    H = h0.shape[1]
    h, hs = h0, []
    for t in range(u.shape[1]):
        gi = u[:, t] @ w_ih.T + b_ih
        gh = h @ w_hh.T + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        if wrong == "gates_r_z_exchanged":
            r, z = z, r
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * h + z * n if wrong == "update_weights_exchanged" else (1 - z) * n + z * h
        hs.append(h)
    return torch.stack(hs, 1)


def _plan_wrong(embd, nxp, cast_locs, w, iters, cmd, ppm, crop, wrong):
    """plan_ref with one mistake."""
    B, H = embd.shape
    T = cast_locs.shape[2]
    if wrong == "sample_modulo_B_minus_1":
        idx = torch.arange(B) % (B - 1)
        embd, nxp, cast_locs = embd[idx], nxp[idx], cast_locs[idx]
    cmds = [cmd] if cmd >= 0 else list(range(cast_locs.shape[1]))
    NC = len(cmds)
    target = (nxp * ppm / crop * 2 - 1)[:, None, None, :].expand(B, NC, T, 2)
    h0 = embd[:, None, :].expand(B, NC, H).reshape(B * NC, H)
    loc, res = cast_locs[:, list(range(NC)) if wrong == "ci_for_c" else cmds], []
    earlier = torch.arange(T).sub(1).clamp(min=0)
    for _ in range(iters):
        fed = loc[:, :, earlier] if wrong == "waypoint_of_t_minus_1" else loc
        u = torch.cat([target, fed], -1).reshape(B * NC, T, 4)
        hs = _gru_seq_wrong(u, h0, w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"], wrong)
        step = (hs @ w["mlp_w"].T + w["mlp_b"]).reshape(B, NC, T, 2)
        loc = (step if wrong == "no_cumsum" else torch.cumsum(step, 2)) + loc
        res.append(loc)
    return torch.stack(res, 1)


def _cast_wrong(feat, w, T, cmd_w, cmd_b, oris, locs, wrong):
    """cast_ref with one mistake."""
    hw = feat.shape[2] * feat.shape[3]
    embd = feat.flatten(2).sum(2) / (hw - 1 if wrong == "mean_over_hw_minus_1" else hw)
    B, E = embd.shape
    if wrong == "sample_modulo_B_minus_1":
        embd = embd[torch.arange(B) % (B - 1)]
    u = embd[:, None, :].expand(B, T, E)
    per_cmd = []
    for c in range(w["w_ih"].shape[0]):
        hs = _gru_seq_wrong(u, embd.new_zeros(B, w["w_hh"].shape[2]), w["w_ih"][c], w["w_hh"][c], w["b_ih"][c], w["b_hh"][c], wrong)
        step = hs @ w["mlp_w"][c].T + w["mlp_b"][c]
        per_cmd.append(step if wrong == "no_cumsum" else torch.cumsum(step, 1))
    cast = torch.stack(per_cmd, 1)
    if oris is not None:
        co, si = torch.cos(oris)[:, None, None], torch.sin(oris)[:, None, None]
        if wrong == "sine_sign":
            si = -si
        cast = torch.stack([cast[..., 0] * co - cast[..., 1] * si, cast[..., 0] * si + cast[..., 1] * co], -1)
    if locs is not None:
        cast = cast + locs[:, None, None, :]
    return embd, cast, None if cmd_w is None else torch.sigmoid(embd @ cmd_w.T + cmd_b)


def _plan_mistakes(case):
    """The mistakes that are not the identity at this case's shape."""
    out = ["gates_r_z_exchanged", "update_weights_exchanged"]
    if case.T > 1:
        out += ["waypoint_of_t_minus_1", "no_cumsum"]   # (waypoint 0 has no predecessor: at T = 1 there is nothing to shift or sum)
    if case.cmd > 0:
        out.append("ci_for_c")
    if case.B > 1:
        out.append("sample_modulo_B_minus_1")
    return out


def _cast_mistakes(case):
    out = ["gates_r_z_exchanged", "update_weights_exchanged"]
    if case.T > 1:
        out.append("no_cumsum")
    if case.B > 1:
        out.append("sample_modulo_B_minus_1")
    if case.pose in ("oris", "both"):
        out.append("sine_sign")
    if case.hw != (1, 1):
        out.append("mean_over_hw_minus_1")
    return out


def test_the_wrong_copies_are_the_reference_without_their_mistake():
    case = U.PLAN_CASES[14]
    d = U.to(U.plan_case(case).inp, F64)
    assert torch.equal(_plan_wrong(d["embd"], d["nxp"], d["cast_locs"], d["w"], case.iters, case.cmd, U.PPM, U.CROP, None), U.plan_case(case).ref64)
    case = U.CAST_CASES[0]
    m = U.cast_case(case)
    d = U.to(m.inp, F64)
    got = _cast_wrong(d["feat"], d["w"], case.T, wrong=None, **U.cast_call_args(case, d))
    assert torch.equal(got[0], m.embd.ref64) and torch.equal(got[1], m.cast.ref64) and torch.equal(got[2], m.cmds.ref64)


@pytest.mark.parametrize("case", U.PLAN_CASES, ids=lambda c: c.id)
def test_plan_bound_tells_every_mistake(case):
    m = U.plan_case(case)
    d = U.to(m.inp, F64)
    for wrong in _plan_mistakes(case):
        moved = U.err_of(_plan_wrong(d["embd"], d["nxp"], d["cast_locs"], d["w"], case.iters, case.cmd, U.PPM, U.CROP, wrong), m.ref64)
        assert moved > 100 * m.bound, f"{wrong} moves the plan by {moved:.3e}, bound {m.bound:.3e}"


@pytest.mark.parametrize("case", U.CAST_CASES, ids=lambda c: c.id)
def test_cast_bound_tells_every_mistake(case):
    m = U.cast_case(case)
    d = U.to(m.inp, F64)
    for wrong in _cast_mistakes(case):
        embd, cast, cmds = _cast_wrong(d["feat"], d["w"], case.T, wrong=wrong, **U.cast_call_args(case, d))
        moved = U.err_of(cast, m.cast.ref64)
        assert moved > 100 * m.cast.bound, f"{wrong} moves the waypoints by {moved:.3e}, bound {m.cast.bound:.3e}"
        if wrong in ("mean_over_hw_minus_1", "sample_modulo_B_minus_1"):   # the mistakes that reach the embedding and the scores
            assert U.err_of(embd, m.embd.ref64) > 100 * m.embd.bound
            assert cmds is None or U.err_of(cmds, m.cmds.ref64) > 100 * m.cmds.bound
