"""The pillar pipeline (csrc/pillar.hip through ops.pillar_scatter / ops.pillar_decorate) bit for bit against float64 at every point
width (4, 8, 11), on the smallest grids at which each of its paths exists, and on general float32 clouds within a derived bound.

Class X data (tests/pillar_exact_util.py; checked on the host by tests/test_pillar_exact_host.py) makes every partial sum of the
pipeline representable, so the float64 canvas is the only correct one: every comparison of class X is np.array_equal / torch.equal,
whatever the path (MFMA or VALU, 16-byte or scalar stores, zeros from k_rows or from k_bin, 32-, 48- or 64-byte records), the job split,
the group, the clamp layer, the overflow list or what the workspace held before.  Class G compares with the bound the util derives."""
import collections
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import torch

from lav_amd import _lib, ops
from tests import pillar_exact_util as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = collections.Counter()      # launches of the canvas pair per built variant: (D, build, stores, zeros, record bytes)
_refs, _weights = {}, {}


def variant(case, impl, env=None):
    env = env or {}
    rec = 32 if case.D == 4 else (48 if env.get("LAV_PILLAR_REC") == "48" else 64)
    return (case.D, impl, "vec4" if case.grid.nx % 4 == 0 else "scalar", "zeros in k_bin" if env.get("LAV_PILLAR_ZERO") == "bin" else "zeros in k_rows", rec)


@pytest.fixture(scope="module", autouse=True)
def census():
    t0 = time.time()
    yield
    print(f"\n[pillar exact] {time.time() - t0:.1f} s; launches per built variant (point width, build, stores, zeros, record bytes):")
    for k in sorted(CENSUS):
        print(f"[pillar exact]   {k}: {CENSUS[k]}")
    _refs.clear()          # (the B33 references are 34 MB each: not kept for the rest of the session)
    _weights.clear()
    P.x_case.cache_clear()
    P.g_case.cache_clear()


def ref_of(case):
    """The float64 reference of a class X case, once: (canvas as float32 - the preconditions say it converts exactly -, the Ref without
    its canvas)."""
    if case.name not in _refs:
        if case.cls == "X":
            ref = P.preconditions(case)
            _refs[case.name] = (ref.canvas.astype(np.float32), ref._replace(canvas=None))
        else:
            ref = P.forward64(case)
            _refs[case.name] = (ref.canvas, ref)
    return _refs[case.name]


def run(case, impl="mfma", want_indices=True, amax=None):
    key = (case.name, id(case))
    if key not in _weights:
        _weights[key] = (case, [torch.from_numpy(a).to(DEV) for a in (case.w1, case.b1, case.w2, case.b2)])
    os.environ["LAV_PILLAR_IMPL"] = impl
    try:
        out = ops.pillar_scatter(torch.from_numpy(case.points).to(DEV), case.n, ops.make_grid(*case.grid.args), *_weights[key][1],
                                 want_indices=want_indices, amax=amax)
    finally:
        os.environ.pop("LAV_PILLAR_IMPL", None)
    canvas = out[0] if want_indices else out
    assert canvas.data_ptr() % 16 == 0
    CENSUS[variant(case, impl)] += 1
    return out


def check_exact(case, out, what=""):
    canvas, uc, inv = out
    want, ref = ref_of(case)
    P.assert_exact(uc.cpu().numpy(), ref.unique_coords, f"{case.name}{what}: unique_coords")
    P.assert_exact(inv.cpu().numpy(), ref.inverse, f"{case.name}{what}: inverse")
    P.assert_exact(canvas.cpu().numpy(), want, f"{case.name}{what}: canvas")


X_RUNS = [c + ("mfma",) for c in P.x_cases()] + [c + ("valu",) for c in P.x_cases() if c[1] == 11]


@pytest.mark.parametrize("grid,D,kind,impl", X_RUNS, ids=lambda v: str(v))
def test_class_x_is_exact(grid, D, kind, impl):
    case = P.x_case(grid, D, kind)
    if grid == "B33":      # more units than 8 per workgroup: the classes have a second group
        assert case.batch * case.grid.ny * case.grid.upr > 8 * _lib.load().lav_pillar_amax_count(case.batch, ops.make_grid(*case.grid.args))
    out = run(case, impl)
    check_exact(case, out)
    again = run(case, impl)
    assert all(torch.equal(a, b) for a, b in zip(out, again)), f"{case.name}: a repeated call gives other bits"
    perm = run(case.permuted(), impl)
    assert torch.equal(out[0], perm[0]) and torch.equal(out[1], perm[1]), f"{case.name}: a permuted cloud gives other bits"


G_RUNS = [c + ("mfma",) for c in P.g_cases()] + [c + ("valu",) for c in P.g_cases() if c[1] == 11]


@pytest.mark.parametrize("grid,D,kind,impl", G_RUNS, ids=lambda v: str(v))
def test_class_g_is_within_the_derived_bound(grid, D, kind, impl):
    case = P.g_case(grid, D, kind)
    _, ref = ref_of(case)
    canvas, uc, inv = run(case, impl)
    P.assert_exact(uc.cpu().numpy(), ref.unique_coords, f"{case.name}: unique_coords")
    P.assert_exact(inv.cpu().numpy(), ref.inverse, f"{case.name}: inverse")
    got = canvas.cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref.canvas)
    print(f"[pillar exact] {case.name} {impl}: worst error / bound {float((err / np.where(ref.tol > 0, ref.tol, np.inf)).max()):.3f}")
    P.assert_within(got, ref, f"{case.name} {impl}")
    perm = run(case.permuted(), impl)
    assert torch.equal(canvas, perm[0]) and torch.equal(uc, perm[1]), f"{case.name}: a permuted cloud gives other bits"


@pytest.mark.parametrize("max_points", [1023, 1024, 1025, 0])
def test_scans_around_one_tile(max_points):
    """S31 at batch 2: 2048 cells = one scan tile; 2 x max_points rows = one below, on and one above a tile; and no rows at all."""
    case = P.x_scan_case(max_points)
    assert case.points.shape[1] == max_points and 2 * (case.grid.nx + 1) * (case.grid.ny + 1) == P.SCAN_TILE
    out = run(case)
    check_exact(case, out)
    assert torch.equal(run(case, want_indices=False), out[0])
    if max_points == 0:
        assert not out[0].any() and out[1].shape == (0, 3) and out[2].shape == (0,)


def test_refusals_leave_the_next_call_right():
    """86 clamp layers, batch 65 and point width 5 are refused; after each refusal a valid call (for the width: on the same batch and
    grid, whose workspace the refusal dropped) is exact."""
    good = P.x_case("S36", 4, "spread")
    check_exact(good, run(good))
    w4 = _weights[(good.name, id(good))][1]
    r = P.REFUSED_GRID
    pts = torch.from_numpy(P.x_case("S32", 4, "spread").points).to(DEV)            # (x in [0, 16), y in [-8, 8): inside R100 where y >= 0)
    with pytest.raises(RuntimeError, match="clamp layers"):
        ops.pillar_scatter(pts, [pts.shape[1]], ops.make_grid(*r.args), *w4)
    check_exact(good, run(good), " after the refused grid")
    with pytest.raises(RuntimeError, match="batch 65"):
        ops.pillar_scatter(torch.from_numpy(np.repeat(good.points[:, :8], 65, axis=0)).to(DEV), [8] * 65, ops.make_grid(*good.grid.args), *w4)
    check_exact(good, run(good), " after batch 65")
    w5 = [torch.zeros((10, 64), device=DEV)] + w4[1:]
    with pytest.raises(RuntimeError, match="D=5"):
        ops.pillar_scatter(torch.zeros((1, 16, 5), device=DEV), [16], ops.make_grid(*good.grid.args), *w5)
    check_exact(good, run(good), " after point width 5")
    dense = P.x_case("S36", 11, "dense")
    check_exact(dense, run(dense), " (dense) after point width 5")


def test_workspace_sequence():
    """One workspace per (batch, grid) serves every point width and max_points: both counter sets and both overflow counts in turn, a
    stale pairing hint from a very different cloud, overflowing calls followed by calls that must not see their records."""
    outs = []
    for step, (grid, D, kind, v) in enumerate(P.SEQUENCE, 1):
        case = P.x_case(grid, D, kind, v)
        outs.append(run(case))
        check_exact(case, outs[-1], f" (step {step})")
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[-1]))


AMAX_CASES = [(g, D, k) for g in ("S34", "W40") for D in (4, 11) for k in ("sparse", "spread", "dense")] + [("B33", D, "spread") for D in (4, 11)]


@pytest.mark.parametrize("grid,D,kind", AMAX_CASES, ids=lambda v: str(v))
def test_canvas_bound(grid, D, kind):
    case = P.x_case(grid, D, kind)
    plain = run(case, want_indices=False)
    am = ops.Amax(DEV, capacity=2048)
    with_b = run(case, want_indices=False, amax=am)
    assert torch.equal(with_b, plain), f"{case.name}: asking for the bound changes the canvas"
    P.assert_exact(with_b.cpu().numpy(), ref_of(case)[0], f"{case.name}: canvas")
    assert ops.amax_of(with_b) is am and am.count == _lib.load().lav_pillar_amax_count(case.batch, ops.make_grid(*case.grid.args))
    parts = am.buf[:am.count].cpu().numpy()
    top = float(with_b.max())
    assert np.isfinite(parts).all() and (parts >= 0).all() and parts.max() >= top
    if not P.reach(case)["collisions"]:       # (a pillar that a later one replaces on a clamped cell still counts)
        assert parts.max() == top
    else:
        assert grid == "W40"


@pytest.mark.parametrize("grid,D,kind", [(g, D, k) for g, D, k in AMAX_CASES if k != "sparse"] + [("B33", D, "dense") for D in (4, 8, 11)]
                         + [(g, 8, k) for g in ("S34", "W40") for k in ("spread", "dense")] + [("B33", 8, "spread")], ids=lambda v: str(v))
def test_decorate(grid, D, kind):
    case = P.x_case(grid, D, kind)
    _, ref = ref_of(case)
    dec, uc, inv, src = ops.pillar_decorate(torch.from_numpy(case.points).to(DEV), case.n, ops.make_grid(*case.grid.args))
    P.assert_exact(uc.cpu().numpy(), ref.unique_coords, f"{case.name}: unique_coords")
    P.assert_exact(inv.cpu().numpy(), ref.inverse, f"{case.name}: inverse")
    s = src.cpu().numpy()
    assert np.all(np.diff(s) > 0)
    P.assert_exact(s, ref.kept, f"{case.name}: kept_src")
    P.assert_exact(dec.cpu().numpy(), ref.dec, f"{case.name}: decorated")


@pytest.mark.parametrize("D", [2, 16])
def test_decorate_refuses_other_widths(D):
    g = P.GRIDS["S34"]
    with pytest.raises(RuntimeError, match="bad points"):
        ops.pillar_decorate(torch.zeros((1, 8, D), device=DEV), [8], ops.make_grid(*g.args))
    case = P.x_case("S34", 4, "spread")
    dec, _, _, _ = ops.pillar_decorate(torch.from_numpy(case.points).to(DEV), case.n, ops.make_grid(*g.args))
    P.assert_exact(dec.cpu().numpy(), ref_of(case)[1].dec, f"{case.name}: decorated after the refusal")


def test_decorate_without_points():
    """S31 at batch 2 without a kept row - max_points = 0, then 16 rows per cloud that all lie outside the grid: every output is empty
    (the kept-row total comes from a memset in the first call, from the scan in the second); a call with points after them is exact."""
    empty = P.x_scan_case(0)
    grid, D = ops.make_grid(*empty.grid.args), empty.D
    assert empty.points.shape == (2, 0, D) and (empty.grid.nx, empty.grid.ny) == (31, 31)
    outside = torch.full((2, 16, D), 100.0, device=DEV)
    for what, pts, n in (("max_points 0", torch.from_numpy(empty.points).to(DEV), empty.n), ("rows outside the grid", outside, [16, 16])):
        dec, uc, inv, src = ops.pillar_decorate(pts, n, grid)
        assert (dec.shape, uc.shape, inv.shape, src.shape) == ((0, D + 5), (0, 3), (0,), (0,)), what
    case = P.x_case("S34", 4, "spread")
    dec, uc, inv, src = ops.pillar_decorate(torch.from_numpy(case.points).to(DEV), case.n, ops.make_grid(*case.grid.args))
    ref = ref_of(case)[1]
    for got, want, name in ((uc, ref.unique_coords, "unique_coords"), (inv, ref.inverse, "inverse"), (src, ref.kept, "kept_src"), (dec, ref.dec, "decorated")):
        P.assert_exact(got.cpu().numpy(), want, f"{case.name} after the empty calls: {name}")


KNOB_ENVS = [{"LAV_PILLAR_ZERO": "bin"}, {"LAV_PILLAR_REC": "48"}, {"LAV_PILLAR_WG_PER_CU": "1"}, {"LAV_PILLAR_ZERO": "bin", "LAV_PILLAR_WG_PER_CU": "1"}]


def test_knobs_read_once_per_process():
    """The three knobs that change the built kernel, each in a fresh child process (tests/_pillar_knob_worker.py), one after the
    other; the first child that does not exit 0 ends the test."""
    runs = [c + ("mfma",) for c in P.KNOB_CASES] + P.KNOB_EXTRA
    for knobs in KNOB_ENVS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("LAV_PILLAR_")}
        env.update(knobs)
        with tempfile.TemporaryDirectory(prefix="lav_pillar_knobs_") as tmp:
            r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "_pillar_knob_worker.py"), tmp], env=env, cwd=REPO,
                               capture_output=True, text=True, timeout=120)     # a torch import, 28 small launches, six 34 MB canvases: 4 s
            assert r.returncode == 0, f"{knobs}: the worker exited {r.returncode}\n{r.stderr[-3000:]}"
            with np.load(os.path.join(tmp, "out.npz")) as z:
                for grid, D, kind, impl in runs:
                    case = P.x_case(grid, D, kind)
                    want, ref = ref_of(case)
                    key = f"{grid}/{D}/{kind}/{impl}"
                    P.assert_exact(z[key + "/uc"], ref.unique_coords, f"{knobs} {case.name}: unique_coords")
                    P.assert_exact(z[key + "/inv"], ref.inverse, f"{knobs} {case.name}: inverse")
                    P.assert_exact(z[key + "/canvas"], want, f"{knobs} {case.name} {impl}: canvas")
                    CENSUS[variant(case, impl, knobs)] += 1


def test_every_built_variant_is_launched():
    """Every instantiation launch_canvas can select outside the trace build, in this process: point widths 4, 8, 11 on the matrix cores and
    11 on the VALU, 16-byte and scalar stores (the knob variants: test_knobs_read_once_per_process)."""
    for grid in ("S36", "S34"):
        for D, impl in ((4, "mfma"), (8, "mfma"), (11, "mfma"), (11, "valu")):
            case = P.x_case(grid, D, "spread")
            check_exact(case, run(case, impl), f" {impl}")
            assert CENSUS[variant(case, impl)] >= 1
