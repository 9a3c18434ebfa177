"""The GRU waypoint decoders (lav_amd/csrc/gru.hip) on every launch path against a float64 reference (tests/gru_ref_util.py):
the persistent plan kernel in all four instantiations (1 or up to 6 state rows, H = 512 or generic), the VALU step kernel, the MFMA
step path, k_plan_out and the cast kernel, over the range of H, T, iters, num_cmds, cmd, embd_dim and hw that include/lav_amd.h
promises.  ops.gru_plan / gru_cast / embed_cast are called directly with seeded tensors: no model, no golden file.

The bound of a case is 4 x max(error of a plain fp32 evaluation of the same inputs against float64, one fp32 ulp of the largest
reference value): the kernels are a second fp32 evaluation in another summation order, not the same one.  Largest measured
max|got - ref64| in units of that max(...) over the tables (limit 4):
    persistent, one state row      1.78
    persistent, 2 to 6 state rows  1.46
    VALU step kernel               2.30
    MFMA step path                 1.50
    cast / embed-cast              1.49
(every test prints its own figure as a GRU_RATIO line; the file's 112 cases take 3.4 s).
tests/test_gru_ref_host.py shows on the CPU that the reference itself meets this bound under another summation order and that a single
wrong index or sign moves it by more than 100 bounds."""
import ctypes as C
import functools

import pytest
import torch

from lav_amd import _lib, ops
from tests import gru_ref_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = 777.0


@pytest.fixture(autouse=True)
def _default_plan_knobs(monkeypatch):
    monkeypatch.delenv("LAV_PLAN_IMPL", raising=False)
    monkeypatch.delenv("LAV_PLAN_SPIN_LIMIT", raising=False)


@functools.lru_cache(maxsize=None)
def _plan_dev(case):
    return U.to(U.plan_inputs(case.H, case.num_cmds, case.T, case.B, case.seed), device=DEV)


def _w(d):
    return [d["w"][k] for k in U.W_KEYS]


def _plan(case, impl="auto", d=None, cmd=None):
    d = _plan_dev(case) if d is None else d
    return ops.gru_plan(d["embd"], d["nxp"], d["cast_locs"], *_w(d), case.iters, case.cmd if cmd is None else cmd, U.PPM, U.CROP, impl=impl)


def _completed(case):
    """The last persistent launch of this case's sizes on the current stream ran to its end in every workgroup."""
    status = ops.gru_plan_status(case.B, case.H, case.num_cmds, case.cmd, DEV)
    diag = ops.gru_plan_diag(case.B, case.H, case.num_cmds, case.cmd, DEV)
    assert status == 0 and diag["status"] == 0 and diag["entered"] == diag["completed"] == case.H // 8 and diag["abort_wg_plus1"] == 0, \
        f"{case.id}: persistent launch did not complete: status {status}, {diag}"


def _within(got, m, what):
    assert got.shape == m.ref64.shape
    err, unit = U.err_of(got.cpu(), m.ref64), max(m.err32, m.floor)
    print(f"GRU_RATIO {what} err={err:.3e} restatement={m.err32:.3e} floor={m.floor:.3e} ratio={err / unit:.3f}")
    assert err <= m.bound, (f"{what}: max|got - ref64| = {err:.3e} > bound {m.bound:.3e}; fp32 restatement {m.err32:.3e}, ulp floor {m.floor:.3e}, "
                            f"ratio {err / unit:.2f} (limit 4)")


# ------------------------------------------------------------------------------------------------ a. plan against float64
# (case, how): every row as ops.gru_plan launches it; persistent rows again on the step path; MFMA rows again on the VALU step kernel
_PLAN_RUNS = [(c, "auto") for c in U.PLAN_CASES] + [(c, "steps") for c in U.PLAN_CASES if c.path.startswith("persistent")] + \
             [(c, "valu_knob") for c in U.PLAN_CASES if c.path == "mfma"]


@pytest.mark.parametrize("case,how", _PLAN_RUNS, ids=[f"{c.id}-{how}" for c, how in _PLAN_RUNS])
def test_plan_equals_float64_on_every_path(case, how, monkeypatch):
    """An MFMA row and the same row under LAV_PLAN_IMPL=v agree only within the bound, not bit for bit: the MFMA step sums the
    recurrent product in four quarters of the reduction dimension (one per wave, 16x16x4 blocks) that meet in LDS, the VALU kernel
    in 8-term chains per lane and a 6-level butterfly; the input projection and the gates follow, on different partial sums.
    That they do differ is asserted: a default launch that silently fell back to the VALU kernel (16 or more state rows whose
    workspace the library no longer takes for large enough) is inside every bound above, and only this tells it from the MFMA step."""
    if how == "valu_knob":
        default = _plan(case).clone()
        monkeypatch.setenv("LAV_PLAN_IMPL", "v")
    got = _plan(case, impl="steps" if how == "steps" else "auto")
    path = case.path if how == "auto" else "valu"
    if path.startswith("persistent"):
        _completed(case)
    _within(got, U.plan_case(case), f"plan {path} {case.id}")
    if how == "valu_knob":
        assert not torch.equal(got, default), f"{case.id}: the default launch equals the VALU step kernel bit for bit: it did not run the MFMA step"


# ------------------------------------------------------------------------------------------------ b. path identities
@pytest.mark.parametrize("case", [c for c in U.PLAN_CASES if c.path.startswith("persistent")], ids=lambda c: c.id)
def test_persistent_plan_equals_the_step_path_bit_for_bit(case):
    want = _plan(case, impl="steps")
    got = _plan(case)
    _completed(case)
    assert torch.equal(got, want), f"{case.id}: persistent and step path differ by {float((got - want).abs().max()):.3e}"


_STEP_SHAPES = [U.PlanCase(192, 5, 3, -1, 7, 3, seed=311), U.PlanCase(512, 2, 6, -1, 20, 2, seed=312), U.PlanCase(64, 5, 2, -1, 64, 1, seed=313)]
_MFMA_SHAPES = [U.PlanCase(192, 20, 3, -1, 7, 2, seed=321), U.PlanCase(512, 20, 2, -1, 20, 1, seed=322), U.PlanCase(64, 20, 5, -1, 33, 2, seed=323)]


def _rows(d, rows):
    return dict(d, embd=d["embd"][rows].contiguous(), nxp=d["nxp"][rows].contiguous(), cast_locs=d["cast_locs"][rows].contiguous())


@pytest.mark.parametrize("case", _STEP_SHAPES, ids=lambda c: c.id)
def test_step_path_one_command_is_that_slice_of_all_commands(case):
    assert case.R < U.MFMA_MIN_ROWS
    full = _plan(case, impl="steps")
    for c in (0, case.num_cmds - 1):
        one = _plan(case, impl="steps", cmd=c)
        assert one.shape == (case.B, case.iters, 1, case.T, 2) and torch.equal(one, full[:, :, c:c + 1]), f"cmd {c}"


@pytest.mark.parametrize("case", [c for c in _STEP_SHAPES if c.B == 5], ids=lambda c: c.id)
def test_step_path_sample_is_independent_of_its_batch(case):
    full = _plan(case, impl="steps")
    for b in (0, 4):
        one = _plan(case, impl="steps", d=_rows(_plan_dev(case), slice(b, b + 1)))
        assert torch.equal(one, full[b:b + 1]), f"sample {b}"


@pytest.mark.parametrize("case", _MFMA_SHAPES, ids=lambda c: c.id)
def test_mfma_path_rows_are_independent_of_batch_and_command_set(case):
    """Both sides of every comparison run the MFMA step path (16 or more state rows)."""
    d16 = _rows(_plan_dev(case), slice(0, 16))
    full20, full16 = _plan(case), _plan(case, d=d16)
    assert torch.equal(full16, full20[:16]), "B = 16 against the first 16 samples of B = 20"
    for c in (0, case.num_cmds - 1):
        one = _plan(case, d=d16, cmd=c)   # 16 rows
        assert torch.equal(one, full16[:, :, c:c + 1]), f"cmd {c}"


# ------------------------------------------------------------------------------------------------ c. one workspace, many shapes
def test_one_plan_workspace_serves_shapes_and_paths_back_to_back():
    """The step path writes its h sequence as floats over the bytes the next persistent launch reads as {epoch, value} granules, and a
    smaller shape reuses the larger one's workspace: every launch must compute what it computes on a drained stream."""
    big = U.PlanCase(512, 1, 6, -1, 20, 5, seed=331)
    runs = [(big, "auto"), (U.PlanCase(192, 8, 5, -1, 64, 1, seed=332), "steps"), (U.PlanCase(64, 2, 3, 1, 7, 3, seed=333), "auto"),
            (big._replace(seed=334), "auto"), (big, "auto")]
    assert [c.R for c, _ in runs] == [6, 40, 2, 6, 6]
    with torch.cuda.stream(torch.cuda.Stream()):
        first = []
        for case, impl in runs:
            torch.cuda.synchronize()
            first.append(_plan(case, impl=impl).clone())
            if impl == "auto":
                _completed(case)
        torch.cuda.synchronize()
        second = [_plan(case, impl=impl) for case, impl in runs]   # back to back, nothing in between
        _completed(big)
        for i, (a, b) in enumerate(zip(first, second)):
            assert torch.equal(a, b), f"launch {i + 1} ({runs[i][0].id}, {runs[i][1]}) differs from its first pass by {float((a - b).abs().max()):.3e}"
        assert torch.equal(first[0], first[4]) and not torch.equal(first[0], first[3])
        third = []
        for case, impl in runs:   # once more, with the status read after each persistent launch
            third.append(_plan(case, impl=impl))
            if impl == "auto":
                _completed(case)
        assert all(torch.equal(a, b) for a, b in zip(first, third))
        assert ops.gru_plan_diag(big.B, big.H, big.num_cmds, big.cmd, DEV)["aborted_launches"] == 0


# ------------------------------------------------------------------------------------------------ d. cast and embed-cast
@functools.lru_cache(maxsize=None)
def _cast_dev(case):
    return U.to(U.cast_case(case).inp, device=DEV)


@pytest.mark.parametrize("case", U.CAST_CASES, ids=lambda c: c.id)
def test_embed_cast_equals_float64(case):
    m, d = U.cast_case(case), _cast_dev(case)
    embd, cast, cmds = ops.embed_cast(d["feat"], *_w(d), case.T, want_embd=case.want_embd, **U.cast_call_args(case, d))
    _within(cast, m.cast, f"cast waypoints {case.id}")
    assert (embd is None) == (not case.want_embd) and (cmds is None) == (not case.scores)
    if embd is not None:
        _within(embd, m.embd, f"cast embedding {case.id}")
    if cmds is not None:
        _within(cmds, m.cmds, f"cast scores {case.id}")


@pytest.mark.parametrize("case", [c._replace(hw=(1, 1), pose="neither", scores=False, seed=c.seed + 50) for c in U.CAST_CASES[:5]], ids=lambda c: c.id)
def test_gru_cast_equals_float64_and_embed_cast_of_a_1x1_map(case):
    m, d = U.cast_case(case), _cast_dev(case)
    embd = d["feat"].flatten(1)
    got = ops.gru_cast(embd, *_w(d), case.T)
    _within(got, m.cast, f"cast gru_cast {case.id}")
    e2, c2, _ = ops.embed_cast(embd, *_w(d), case.T)
    assert torch.equal(c2, got) and torch.equal(e2, embd)
    assert torch.equal(ops.embed_cast(d["feat"], *_w(d), case.T, want_embd=False)[1], got)


def _embed_cast_raw(d, case, B, embd_out, cmds_out, out, E=None, H=64, num_cmds=None, T=None, hw=None, cmd_w=True):
    """lav_embed_cast on caller-owned buffers."""
    w = d["w"]
    p = lambda t: None if t is None else t.data_ptr()
    return _lib.load().lav_embed_cast(p(d["feat"]), B, case.E if E is None else E, case.hw[0] * case.hw[1] if hw is None else hw, p(embd_out), H,
                                      case.num_cmds if num_cmds is None else num_cmds, case.T if T is None else T, p(w["w_ih"]), p(w["w_hh"]),
                                      p(w["b_ih"]), p(w["b_hh"]), p(w["mlp_w"]), p(w["mlp_b"]), p(d["cmd_w"]) if cmd_w else None,
                                      p(d["cmd_b"]) if cmd_w else None, p(cmds_out), p(d["oris"]), p(d["locs"]), p(out),
                                      torch.cuda.current_stream().cuda_stream)


def _cast_buffers(case, B=None):
    B = case.B if B is None else B
    full = lambda *s: torch.full(s, SENTINEL, device=DEV)
    return full(B, case.E), full(B, case.num_cmds), full(B, case.num_cmds, case.T, 2)


@pytest.mark.parametrize("case", [U.CAST_CASES[0], U.CAST_CASES[4]], ids=lambda c: c.id)
def test_embed_cast_under_a_batch_limit_leaves_the_other_rows_alone(case):
    d = _cast_dev(case)
    want = _cast_buffers(case)
    assert _embed_cast_raw(d, case, case.B, *want) == 0
    assert not any((t == SENTINEL).any() for t in want)
    for n in (0, 2, 3):
        got = _cast_buffers(case)
        with ops.batch_limit(torch.tensor([n], dtype=torch.int32, device=DEV)):
            assert _embed_cast_raw(d, case, case.B, *got) == 0
        for g, w in zip(got, want):
            assert torch.equal(g[:n], w[:n]), f"limit {n}: live rows differ"
            assert (g[n:] == SENTINEL).all(), f"limit {n}: rows at or above the limit were written"
    again = _cast_buffers(case)
    assert _embed_cast_raw(d, case, case.B, *again) == 0 and all(torch.equal(a, w) for a, w in zip(again, want))


# ------------------------------------------------------------------------------------------------ e. what the entry points refuse
def _refused(rc, name, outs, code=None):
    msg = _lib.load().lav_last_error()
    torch.cuda.synchronize()
    assert rc < 0 and (code is None or rc == code), f"{name} returned {rc}"
    assert msg and name.encode() in msg, f"{name} refused with the message {msg!r}"
    assert all((t == SENTINEL).all() for t in outs), f"{name} wrote its output although it refused the call"


_PLAN_OK = dict(B=2, H=64, num_cmds=3, T=4, iters=2, cmd=-1)


def _plan_raw(fn, ws_bytes="exact", null_ws=False, **over):
    """One of the two plan entry points with the arguments of _PLAN_OK, some of them replaced; buffers sized for the larger of both."""
    a = dict(_PLAN_OK, **over)
    size = {k: max(a[k], _PLAN_OK[k]) for k in ("B", "H", "num_cmds", "T", "iters")}
    d = U.to(U.plan_inputs(size["H"], size["num_cmds"], size["T"], size["B"], seed=341), device=DEV)
    out = torch.full((size["B"], size["iters"], size["num_cmds"], size["T"], 2), SENTINEL, device=DEV)
    R = a["B"] * (1 if a["cmd"] >= 0 else a["num_cmds"])
    need = a["T"] * R * a["H"] * 4 + 512
    ws = torch.zeros(max(_lib.load().lav_gru_plan_workspace_bytes(size["B"], size["H"], size["num_cmds"], size["T"]), need), dtype=torch.uint8, device=DEV)
    nbytes = {"exact": need, "short": need - 1, "all": ws.numel()}[ws_bytes]
    rc = getattr(_lib.load(), fn)(d["embd"].data_ptr(), d["nxp"].data_ptr(), d["cast_locs"].data_ptr(), a["B"], a["H"], a["num_cmds"], a["T"], a["iters"],
                                  a["cmd"], U.PPM, U.CROP, *[t.data_ptr() for t in _w(d)], out.data_ptr(), None if null_ws else ws.data_ptr(), nbytes,
                                  torch.cuda.current_stream().cuda_stream)
    return rc, out


@pytest.mark.parametrize("fn", ["lav_gru_plan", "lav_gru_plan_steps"])
@pytest.mark.parametrize("over", [dict(H=0), dict(H=96), dict(H=576), dict(T=0), dict(T=65), dict(iters=0), dict(cmd=3), dict(cmd=-2)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_plan_refuses_sizes_outside_its_arrays(fn, over):
    rc, out = _plan_raw(fn, ws_bytes="all", **over)
    _refused(rc, "lav_gru_plan", [out], code=-1)


@pytest.mark.parametrize("fn", ["lav_gru_plan", "lav_gru_plan_steps"])
def test_plan_refuses_a_short_or_missing_workspace(fn):
    for kw in (dict(ws_bytes="short"), dict(null_ws=True), dict(ws_bytes="short", B=8)):
        rc, out = _plan_raw(fn, **kw)
        _refused(rc, "lav_gru_plan", [out], code=-3)   # LAV_EWORKSPACE
    rc, out = _plan_raw(fn, B=8)   # T*R*H*4 + 512 bytes exactly: the step path's h sequence fits (24 rows, no room for the MFMA path's extras)
    torch.cuda.synchronize()
    assert rc == 0 and torch.isfinite(out).all() and not (out == SENTINEL).any()


_CAST_REFUSALS = [dict(H=32), dict(H=128), dict(E=0), dict(E=1025), dict(num_cmds=0), dict(T=0), dict(B=65536)]


@pytest.mark.parametrize("over", _CAST_REFUSALS + [dict(cmd_w=True)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_embed_cast_refuses_sizes_outside_its_arrays(over):
    case = U.CastCase(64, 1, 1, 1, (1, 1), "both", True, True, seed=342)
    B = over.get("B", 1)
    d = U.to(U.cast_inputs(max(over.get("E", 0), case.E), case.num_cmds, case.T, B, case.hw, case.seed, H=max(over.get("H", 0), 64)), device=DEV)
    embd_out, cmds_out, out = _cast_buffers(case._replace(E=max(over.get("E", 0), case.E)), B)
    if "cmd_w" in over:   # scores asked for, nowhere to put them
        rc = _embed_cast_raw(d, case, 1, embd_out, None, out)
    else:
        rc = _embed_cast_raw(d, case, B, embd_out, cmds_out, out, **{k: v for k, v in over.items() if k != "B"})
    _refused(rc, "lav_embed_cast", [embd_out, cmds_out, out], code=-1)


@pytest.mark.parametrize("over", _CAST_REFUSALS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_gru_cast_refuses_sizes_outside_its_arrays(over):
    a = dict(dict(B=1, E=64, H=64, num_cmds=1, T=1), **over)
    d = U.to(U.cast_inputs(max(a["E"], 64), 1, 1, a["B"], (1, 1), seed=343, H=max(a["H"], 64)), device=DEV)
    out = torch.full((a["B"], 1, 1, 2), SENTINEL, device=DEV)
    rc = _lib.load().lav_gru_cast(d["feat"].data_ptr(), a["B"], a["E"], a["H"], a["num_cmds"], a["T"], *[t.data_ptr() for t in _w(d)], out.data_ptr(),
                                  None, 0, torch.cuda.current_stream().cuda_stream)
    _refused(rc, "lav_gru_cast", [out], code=-1)


def test_an_empty_batch_is_an_empty_result():
    d = U.to(U.plan_inputs(64, 3, 4, 1, seed=344), device=DEV)
    for impl in ("auto", "steps"):
        for cmd, nc in ((-1, 3), (1, 1)):
            got = ops.gru_plan(d["embd"][:0], d["nxp"][:0], d["cast_locs"][:0], *_w(d), 2, cmd, U.PPM, U.CROP, impl=impl)
            assert got.shape == (0, 2, nc, 4, 2)
    c = U.to(U.cast_inputs(100, 2, 5, 1, (2, 3), seed=345), device=DEV)
    assert ops.gru_cast(c["feat"][:0, :, 0, 0], *_w(c), 5).shape == (0, 2, 5, 2)
    embd, cast, cmds = ops.embed_cast(c["feat"][:0], *_w(c), 5, cmd_w=c["cmd_w"], cmd_b=c["cmd_b"], oris=c["oris"][:0], locs=c["locs"][:0])
    assert embd.shape == (0, 100) and cast.shape == (0, 2, 5, 2) and cmds.shape == (0, 2)
    torch.cuda.synchronize()
