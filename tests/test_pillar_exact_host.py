"""The cases of tests/test_gpu_pillar_exact.py, checked on the host: class X data really is exactly representable
(tests/pillar_exact_util.py's preconditions), the float32 oracle and a second float32 evaluation in another k order then return the
float64 result bit for bit (class G: within the derived bound), the data is SENSITIVE - the reference with one defect (a point missing
from a cell, a mean over the unit, swapped weight rows or tiles, the bias feature one k further, the earlier pillar winning a clamped cell, the
overflow records dropped, the border unit's last columns left zero, un-swapped cell origins; arithmetic in numpy, nothing is injected
into a kernel) changes the canvas - and every case reaches the path it is there for.  No GPU."""
import numpy as np
import pytest

from tests import pillar_exact_util as P

X_CASES = P.x_cases() + [c for c in P.KNOB_CASES if c not in P.x_cases()]
_seen_faults = set()


def applicable(case, ref, fault):
    """A fault applies when the case has what it breaks: a multi-point cell, a clamp collision, an overflowing unit, an occupied
    right-border unit narrower than 32 columns."""
    r = P.reach(case)
    g = case.grid
    if fault in ("drop_point", "unit_mean"):
        return bool(len(ref.inverse)) and np.bincount(ref.inverse).max() >= 2
    if fault == "earlier_wins":
        return r["collisions"]
    if fault == "drop_overflow":
        return len(r["overflowing"]) > 0
    if fault == "border_zero":
        return g.nx % P.UW != 0 and bool(ref.canvas[..., 4 * ((g.nx - 1) // 4):].any())
    return len(ref.inverse) > 0


def check_reach(case, grid, kind):
    r = P.reach(case)
    if kind == "dense":
        # a unit that overflows at whatever bucket capacity the workspace chose, beside other occupied units ...
        assert len(r["overflowing"]) >= 1 and r["occupied_units"] > len(r["overflowing"]), case.name
        if grid == "B33":
            # ... and, where a class owns more than one unit at all (more units than workgroups: B33 only), another occupied unit in
            # the overflowing unit's own group - at two workgroups per CU and at one
            for W in (512, 256):
                assert min(P.reach(case, W)["group_mates"]) >= 1, f"{case.name}: W = {W}"
    if kind == "sparse":
        jobs = (r["group_load"] + 15) // 16
        assert (jobs == 1).any() and (jobs == 2).any(), f"{case.name}: no group of one job (four-way split) or of two (two-way)"
    if grid in ("W40", "T40") and kind != "sparse":
        assert r["layers"] >= 5, f"{case.name}: {r['layers']} occupied layers"
    if grid in ("W40", "T40") and kind == "dense":
        _, uniq, inv, _ = P.indices(case)
        rows, cols, units = P.landing(case.grid, uniq)
        cell = (uniq[:, 0] * case.grid.ny + rows) * case.grid.nx + cols
        crowded = np.isin(cell, np.flatnonzero(np.bincount(cell) >= 5))
        assert np.isin(units[crowded], r["overflowing"]).any(), f"{case.name}: the overflowing unit carries no clamp layers"
    if grid == "B33":
        assert all(case.n[b] == 0 for b in P.B33_EMPTY)
        if kind != "sparse":
            g = case.grid
            tail = case.points[P.B33_TRUNCATED, case.n[P.B33_TRUNCATED]:]
            kept, _, _ = P.opillar.grid_locations(tail, *g.args)
            assert len(tail) >= 4 and len(kept) == len(tail), "cloud 7's tail rows must hold in-range points"
        assert case.batch * case.grid.ny * case.grid.upr > 8 * 512


@pytest.mark.parametrize("grid,D,kind", X_CASES, ids=lambda v: str(v))
def test_class_x_cases(grid, D, kind):
    case = P.x_case(grid, D, kind)
    ref = P.preconditions(case)
    assert ref.canvas.any(), f"{case.name}: an all-zero canvas checks nothing"
    o32, dec32 = P.oracle32(case)
    P.assert_exact(dec32, ref.dec, f"{case.name}: oracle.decorate (float32 running sums)")
    P.assert_exact(o32, ref.canvas, f"{case.name}: the float32 oracle")
    P.assert_exact(P.permuted32(case), ref.canvas, f"{case.name}: float32 in a permuted k order")
    for fault in P.FAULTS:
        if applicable(case, ref, fault):
            _seen_faults.add(fault)
            assert not np.array_equal(P.forward64(case, fault, want_tol=False).canvas, ref.canvas), f"{case.name}: {fault} changes no canvas element"
    check_reach(case, grid, kind)
    # a permuted cloud is the same problem
    assert np.array_equal(P.forward64(case.permuted(), want_tol=False).canvas, ref.canvas)


def test_class_x_sequence_and_scan_cases():
    """The workspace sequence's cases (the dense unit elsewhere, the empty cloud) and the scan cases."""
    for grid, D, kind, variant in P.SEQUENCE:
        case = P.x_case(grid, D, kind, variant)
        ref = P.preconditions(case)
        assert ref.canvas.any() == (kind != "empty")
    a, b = P.x_case("S36", 11, "dense", 0), P.x_case("S36", 11, "dense", 1)
    assert a.dense_unit != b.dense_unit and not np.array_equal(P.forward64(a).canvas, P.forward64(b).canvas)
    g = P.GRIDS["S31"]
    assert 2 * (g.nx + 1) * (g.ny + 1) == P.SCAN_TILE          # batch 2 on S31: the cells fill exactly one scan tile
    for mp in (1023, 1024, 1025, 0):
        case = P.x_scan_case(mp)
        ref = P.preconditions(case)
        assert case.points.shape == (2, mp, 4) and case.n[1] == mp and (mp == 0 or case.n[0] < mp)
        assert len(ref.inverse) == sum(case.n), "every live row is in range, so the kept count is the live count"
        if mp:
            P.assert_exact(P.oracle32(case)[0], ref.canvas, f"{case.name}: the float32 oracle")
    assert P.REFUSED_GRID.clamp_layers == 86 > P.MAX_LAYERS and all(g.clamp_layers <= P.MAX_LAYERS for g in P.GRIDS.values())
    assert P.GRIDS["W40"].clamp_layers == 10 == P.GRIDS["T40"].clamp_layers


def test_grids_reach_what_the_table_claims():
    """The paths of csrc/pillar.hip each grid is there for, from its numbers (W = min(workgroups, units); 512 or 256 workgroups)."""
    G = P.GRIDS
    units = lambda g, B=1: B * g.ny * g.upr
    assert (G["S32"].nx, G["S32"].ny, G["S32"].upr, units(G["S32"])) == (32, 32, 1, 32) and G["S32"].nx % 4 == 0       # W = 32, one slot each, VEC4
    assert (G["S31"].nx, G["S31"].ny, units(G["S31"]) % 2, G["S31"].nx % 4) == (31, 31, 1, 3)                           # odd W, scalar stores, unit 31 wide
    assert (G["S34"].nx, G["S34"].ny, G["S34"].upr, G["S34"].nx % 4, G["S34"].nx - 32) == (34, 34, 2, 2, 2)             # scalar stores, right unit 2 wide
    assert (G["S36"].nx, G["S36"].ny, G["S36"].upr, G["S36"].nx % 4, G["S36"].nx - 32) == (36, 36, 2, 0, 4)             # VEC4, right unit one quad
    assert (G["W40"].nx, G["W40"].ny, G["W40"].clamp_layers) == (40, 32, 10) and (G["T40"].nx, G["T40"].ny, G["T40"].clamp_layers) == (32, 40, 10)
    assert all(units(G[name]) < 256 for name in P.SMALL)             # fewer units than persistent workgroups: nwg = units, one slot per class
    assert (G["B33"].nx, G["B33"].ny) == (64, 64) and units(G["B33"], 33) == 4224 > 8 * 512
    for name, g in G.items():
        assert g.ppm in (2, 4) and float(g.min_x).is_integer() and float(g.min_y).is_integer()
        assert (g.max_x - g.min_x) * g.ppm == g.nx and (g.max_y - g.min_y) * g.ppm == g.ny


@pytest.mark.parametrize("grid,D,kind", P.g_cases(), ids=lambda v: str(v))
def test_class_g_cases(grid, D, kind):
    case = P.g_case(grid, D, kind)
    ref = P.forward64(case)
    g = case.grid
    # the edge rows do what they are there for
    assert ref.unique_coords[:, 1].max() >= g.nx - 1 and ref.unique_coords[:, 2].max() >= g.ny - 1
    assert len(ref.inverse) < case.n[0], "some rows must be dropped"
    assert {3, 5, 7} <= set(np.bincount(ref.inverse).tolist())
    assert np.isfinite(ref.canvas).all() and np.isfinite(ref.tol).all()
    o32, _ = P.oracle32(case)
    P.assert_within(o32, ref, f"{case.name}: the float32 oracle")
    P.assert_within(P.permuted32(case), ref, f"{case.name}: float32 in a permuted k order")
    for fault in P.FAULTS:
        if applicable(case, ref, fault):
            _seen_faults.add(fault)
            err = np.abs(P.forward64(case, fault, want_tol=False).canvas - ref.canvas)
            assert (err > ref.tol).any(), f"{case.name}: {fault} stays inside the bound"
    if kind == "dense":
        assert len(P.reach(case)["overflowing"]) >= 1


def test_every_fault_applied_somewhere():
    for grid, D, kind in (("S34", 4, "dense"), ("W40", 11, "dense")):      # (enough on their own when this test runs alone)
        case = P.x_case(grid, D, kind)
        ref = P.forward64(case, want_tol=False)
        _seen_faults.update(f for f in P.FAULTS if applicable(case, ref, f))
    assert _seen_faults >= set(P.FAULTS), set(P.FAULTS) - _seen_faults
