"""Exactly representable clouds for the pillar pipeline (tests/test_pillar_exact_host.py, tests/test_gpu_pillar_exact.py).

csrc/pillar.hip keeps the per-cell coordinate sums in 64-bit fixed point, does the cell arithmetic in float32 without contraction and
runs the point net as an fp32 fma chain (VALU) or on v_mfma_f32_16x16x4_f32 (one rounding per k-step).  When every partial sum of
both layers is representable, the float64 result is the ONLY correct canvas - whatever the path, the job split, the group, the
clamp layer or the record stride - and the kernels must return it bit for bit.  This module restates PointPillarNet.forward in
float64 (`forward64`), makes such data (class X), checks that it is such data (`preconditions`), makes general float32 clouds with
the grid's edge rows and a DERIVED error bound (class G), and restates the reference with one defect at a time (`FAULTS`) for the
host test's sensitivity checks.

Conventions (csrc/pillar.hip, oracle/pillar.py): nx = cells of xi (from x), ny = cells of yi (from y); the canvas is (B, 64, ny, nx)
and pillar (b, xi, yi) lands on row clamp(ny - 1 - xi), column clamp(yi) - the reference's (swapped) scatter.  A UNIT is one canvas row x
32 columns; ownership class w of W owns units w, w + W, ...; a group is up to 8 of them.  Weights are laid out as the C ABI takes
them: w1 [D + 5][64], w2 [64][64] (input index first).

Class X: ppm in {2, 4}, integer min_x / min_y, coordinates multiples of 1/8, the other columns multiples of 1/8 in [0, 1], a
power-of-two number of points per cell (1 ... 8; 32 in the cells of the dense unit), w1 in [-2, 2], w2 in [-1, 1], biases in [-8, 8]."""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import pillar as opillar

C = 64
UW, NSUB, CAP_MAX, GMAX, MAX_LAYERS, SCAN_TILE = 32, 2, 256, 8, 64, 2048      # csrc/pillar.hip
OVERFLOW_POINTS = NSUB * CAP_MAX                                              # a unit with more points overflows at any `cap`
U = 2.0 ** -24
f32, f64 = np.float32, np.float64


class Grid(namedtuple("Grid", "name min_x max_x min_y max_y ppm")):
    @property
    def nx(self):
        return int((self.max_x - self.min_x) * self.ppm)

    @property
    def ny(self):
        return int((self.max_y - self.min_y) * self.ppm)

    @property
    def upr(self):
        return (self.nx + UW - 1) // UW

    @property
    def args(self):
        return self[1:]

    @property
    def clamp_layers(self):
        """lav_pillar_scatter's count: key rows ny-1 .. nx on canvas row 0, times key columns nx-1 .. ny on the last column."""
        return max(self.nx - (self.ny - 1) + 1, 1) * (max(self.ny - self.nx + 1, 0) + 1)


GRIDS = {g.name: g for g in (
    Grid("S32", 0, 16, -8, 8, 2),        # 32x32: one unit per row, W = 32, one slot per class, VEC4
    Grid("S31", -4, 11.5, -8, 7.5, 2),   # 31x31: odd W, non-VEC4, the unit 31 wide
    Grid("S34", -4, 13, -8, 9, 2),       # 34x34: non-VEC4, right unit 2 columns wide
    Grid("S36", -2, 7, -4, 5, 4),        # 36x36: VEC4, right unit one quad wide
    Grid("W40", -4, 16, -8, 8, 2),       # 40x32: key rows 31 .. 40 clamp to canvas row 0 (10 layers of ordinary cells)
    Grid("T40", 0, 16, -10, 10, 2),      # 32x40: key columns 31 .. 40 clamp to the last column (10 layers on the border unit)
    Grid("B33", 0, 16, -8, 8, 4),        # 64x64 at batch 33: 4224 units > 8 x 512
)}
REFUSED_GRID = Grid("R100", 0, 50, 0, 8, 2)   # 100x16: 86 clamp layers > MAX_LAYERS
BATCH = {"B33": 33}
B33_EMPTY, B33_TRUNCATED = (5, 20), 7
SMALL = ("S32", "S31", "S34", "S36", "W40", "T40")
RICH = ("S34", "S36", "W40", "T40")          # the grids that also run `sparse` and `dense`
WIDTHS = (4, 8, 11)


def rng_of(*key):
    return np.random.Generator(np.random.PCG64(zlib.crc32(repr(key).encode())))


class Case:
    """points (B, nmax, D) float32 with n[b] live rows per cloud (the rows past them hold in-range points that must not count)."""

    def __init__(self, name, cls, grid, D, points, n, weights, dense_unit=None):
        self.name, self.cls, self.grid, self.D = name, cls, grid, D
        self.points, self.n = np.ascontiguousarray(points, f32), [int(v) for v in n]
        self.w1, self.b1, self.w2, self.b2 = (np.ascontiguousarray(w, f32) for w in weights)
        self.dense_unit = dense_unit          # (b, xi, first yi) of the unit that overflows, or None
        assert self.points.shape[0] == len(self.n) and self.points.shape[2] == D and self.w1.shape == (D + 5, C)

    @property
    def batch(self):
        return len(self.n)

    def permuted(self, seed=1):
        """The same clouds with the live rows of every cloud in another order."""
        rng = rng_of("perm", self.name, seed)
        pts = self.points.copy()
        for b, n in enumerate(self.n):
            pts[b, :n] = pts[b, rng.permutation(n)]
        return Case(self.name + " permuted", self.cls, self.grid, self.D, pts, self.n, (self.w1, self.b1, self.w2, self.b2), self.dense_unit)


# ---------------------------------------------------------------------------------------------- float64 reference
FAULTS = ("drop_point", "unit_mean", "swap_w1_rows", "bias_neighbour", "swap_w2_tiles", "earlier_wins", "drop_overflow", "border_zero",
          "origins_unswapped")
Ref = namedtuple("Ref", "canvas unique_coords inverse kept dec tol")


def indices(case):
    """Keep-test and cell ids: float32 by definition of the operation (oracle.pillar).  Returns the kept points (float32), the unique
    pillar rows (b, xi, yi), the inverse map and the kept rows' indices into the flattened (B * nmax) input."""
    g, nmax = case.grid, case.points.shape[1]
    coords, pts, kept = [], [], []
    for b, n in enumerate(case.n):
        kp, c, k = opillar.grid_locations(case.points[b, :n], *g.args)
        coords.append(np.concatenate([np.full((len(c), 1), b, np.int64), c.reshape(-1, 2)], axis=1))
        pts.append(kp)
        kept.append(k + b * nmax)
    uniq, inv = opillar.pillar_generation(np.concatenate(coords, axis=0))
    return np.concatenate(pts, axis=0), uniq, inv, np.concatenate(kept)


def landing(g, uniq):
    """Canvas row, column and unit of every pillar (the reference's clamp)."""
    rows = np.clip(g.ny - 1 - uniq[:, 1], 0, g.ny - 1)
    cols = np.clip(uniq[:, 2], 0, g.nx - 1)
    return rows, cols, (uniq[:, 0] * g.ny + rows) * g.upr + cols // UW


def _rank_within(keys):
    """Position of every element among the elements of its own key, in order of appearance."""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    start = np.r_[0, np.flatnonzero(sk[1:] != sk[:-1]) + 1]
    first = np.repeat(start, np.diff(np.r_[start, len(sk)]))
    rank = np.empty(len(keys), np.int64)
    rank[order] = np.arange(len(keys)) - first
    return rank


def forward64(case, fault=None, want_tol=None):
    """PointPillarNet.forward with means, decoration (swapped, un-centred cell origins), both layers, ReLU and the per-pillar max in
    float64 on the float32 inputs; the canvas written by explicit ordered assignment (pillars in unique order, the later one replaces
    the earlier on a clamped cell).  fault: the same with one defect (FAULTS).  tol (class G, or want_tol): the derived bound of a
    float32 evaluation, per canvas element."""
    g, D, K1 = case.grid, case.D, case.D + 5
    B, nx, ny = case.batch, g.nx, g.ny
    pts, uniq, inv, kept = indices(case)
    P = len(uniq)
    rows, cols, units = landing(g, uniq)
    keep = np.ones(len(pts), bool)
    if fault == "drop_point":          # the first point of the first multi-point pillar that nothing replaces on the canvas
        cell = (uniq[:, 0] * ny + rows) * nx + cols
        last = np.zeros(P, bool)
        last[[np.flatnonzero(cell == c)[-1] for c in np.unique(cell)]] = True
        p = np.flatnonzero(last & (np.bincount(inv, minlength=P) >= 2))[0]
        keep[np.flatnonzero(inv == p)[0]] = False
    if fault == "drop_overflow":       # what arrives at a unit after its two buckets of 256 are full
        keep &= _rank_within(units[inv]) < OVERFLOW_POINTS
    v, iv = pts.astype(f64)[keep], inv[keep]
    seg = units[iv] if fault == "unit_mean" else iv
    nseg = int(seg.max()) + 1 if len(seg) else 0
    sums = np.zeros((nseg, 3))
    np.add.at(sums, seg, v[:, :3])
    mean = (sums / np.maximum(np.bincount(seg, minlength=nseg), 1)[:, None])[seg]
    a, b_ = (1, 2) if fault == "origins_unswapped" else (2, 1)          # the reference pairs yi with min_x and xi with min_y
    xo = uniq[iv, a].astype(f64) / g.ppm + g.min_x
    yo = uniq[iv, b_].astype(f64) / g.ppm + g.min_y
    f = np.concatenate([v, v[:, :3] - mean, (v[:, 0] - xo)[:, None], (v[:, 1] - yo)[:, None]], axis=1)
    w1, b1, w2, b2 = (w.astype(f64) for w in (case.w1, case.b1, case.w2, case.b2))
    if fault == "swap_w1_rows":
        w1[[K1 - 1, K1 - 2]] = w1[[K1 - 2, K1 - 1]]
    if fault == "swap_w2_tiles":
        w2[np.r_[0:16, 16:32]] = w2[np.r_[16:32, 0:16]]
    if fault == "bias_neighbour":      # the constant 1 and the last feature change places in front of [w1; b1]
        h1 = f[:, :K1 - 1] @ w1[:K1 - 1] + w1[K1 - 1] + f[:, K1 - 1:] * b1
    else:
        h1 = f @ w1 + b1
    h1 = np.maximum(h1, 0.0)
    h2 = np.maximum(h1 @ w2 + b2, 0.0)
    feat = np.zeros((P, C))
    np.maximum.at(feat, iv, h2)
    alive = np.bincount(iv, minlength=P) > 0
    winner = np.full((B, ny, nx), -1, np.int64)
    for p in range(P):                                                   # unique order: the later pillar replaces the earlier
        if alive[p] and not (fault == "earlier_wins" and winner[uniq[p, 0], rows[p], cols[p]] >= 0):
            winner[uniq[p, 0], rows[p], cols[p]] = p
    bb, rr, cc = np.nonzero(winner >= 0)                                 # (distinct cells: plain assignment)
    canvas = np.zeros((B, C, ny, nx))
    canvas[bb, :, rr, cc] = feat[winner[bb, rr, cc]]
    if fault == "border_zero" and nx % UW:
        canvas[..., 4 * ((nx - 1) // 4):] = 0.0
    tol = None
    if fault is None and (case.cls == "G" if want_tol is None else want_tol):
        e_f = np.zeros_like(f)
        e_f[:, D:D + 3] = 4 * U * (np.abs(v[:, :3]) + np.abs(mean)) + 2.0 ** -31     # fixed point, the mean's rounding, the subtraction
        e_f[:, D + 3] = 4 * U * (np.abs(v[:, 0]) + np.abs(xo))
        e_f[:, D + 4] = 4 * U * (np.abs(v[:, 1]) + np.abs(yo))
        A1 = np.abs(f) @ np.abs(w1) + np.abs(b1)
        E1 = e_f @ np.abs(w1) + (K1 + 2) * U * A1
        E2 = E1 @ np.abs(w2) + (C + 2) * U * (A1 @ np.abs(w2) + np.abs(b2))
        tolp = np.zeros((P, C))
        np.maximum.at(tolp, iv, E2)                                      # ReLU and max are 1-Lipschitz
        tol = np.zeros((B, C, ny, nx))
        tol[bb, :, rr, cc] = tolp[winner[bb, rr, cc]]
    return Ref(canvas, uniq, inv, kept, f, tol)


# ---------------------------------------------------------------------------------------------- float32 evaluations (host test)
def oracle32(case):
    """oracle.pillar in float32: its decorate (running float32 sums), numpy's float32 products, its scatter_max and scatter_points."""
    g = case.grid
    pts, uniq, inv, _ = indices(case)
    dec = opillar.decorate(pts, uniq, inv, g.min_x, g.min_y, g.ppm)
    h = np.maximum(dec @ case.w1 + case.b1, f32(0))
    h = np.maximum(h @ case.w2 + case.b2, f32(0))
    feat = opillar.scatter_max(h, inv, len(uniq)) if len(uniq) else np.zeros((0, C), f32)
    return opillar.scatter_points(feat, uniq, case.batch, g.nx, g.ny), dec


def permuted32(case, seed=3):
    """A second float32 evaluation: the decorated features of the oracle, every accumulator one float32 chain over k in a permuted
    order that starts from the bias (two roundings per term)."""
    g = case.grid
    pts, uniq, inv, _ = indices(case)
    rng = rng_of("korder", seed)
    h = opillar.decorate(pts, uniq, inv, g.min_x, g.min_y, g.ppm)
    for w, b in ((case.w1, case.b1), (case.w2, case.b2)):
        acc = np.broadcast_to(b, (len(h), C)).astype(f32)
        for k in rng.permutation(w.shape[0]):
            acc = (acc + (h[:, k, None] * w[k][None, :]).astype(f32)).astype(f32)
        h = np.maximum(acc, f32(0))
    feat = opillar.scatter_max(h, inv, len(uniq)) if len(uniq) else np.zeros((0, C), f32)
    rows, cols, _ = landing(g, uniq)
    canvas = np.zeros((case.batch, C, g.ny, g.nx), f32)
    for p in range(len(uniq)):                     # ordered assignment, as forward64
        canvas[uniq[p, 0], :, rows[p], cols[p]] = feat[p]
    return canvas


# ---------------------------------------------------------------------------------------------- preconditions
def quantum(*arrays):
    """The largest power of two that divides every element of the arrays (1.0 when all are zero)."""
    v = np.concatenate([np.abs(np.asarray(a, f64)).reshape(-1) for a in arrays])
    v = v[v != 0]
    if not len(v):
        return 1.0
    m, e = np.frexp(v)
    mi = (m * float(1 << 53)).astype(np.int64)
    le = np.frexp((mi & -mi).astype(f64))[1] - 1
    return float(np.exp2((e - 53 + le).min()))


def is_f32(a):
    a = np.asarray(a, f64)
    return bool(np.all(np.isfinite(a)) and np.array_equal(a.astype(f32).astype(f64), a))


def preconditions(case, ref=None):
    """Class X: every cell count a power of two; every mean, decorated feature and canvas value a float32 number; sum |terms| of both
    layers below 2^24 quanta of their terms (every partial sum in any order is then a float32 number); every channel that w2 feeds has
    zero and non-zero canvas elements.  Returns the float64 reference.  A case that fails here is a broken test."""
    assert case.cls == "X"
    ref = ref or forward64(case, want_tol=False)
    cnt = np.bincount(ref.inverse, minlength=len(ref.unique_coords))
    assert len(cnt) == 0 or (np.all(cnt >= 1) and np.all(cnt & (cnt - 1) == 0)), f"{case.name}: a cell count is no power of two"
    assert is_f32(ref.dec), f"{case.name}: a mean or a decorated feature is no float32 number"
    w1, b1, w2, b2 = (np.abs(w.astype(f64)) for w in (case.w1, case.b1, case.w2, case.b2))
    if len(ref.dec):
        q1 = min(quantum(ref.dec) * quantum(w1), quantum(b1))
        q2 = min(q1 * quantum(w2), quantum(b2))
        A1 = np.abs(ref.dec) @ w1 + b1
        A2 = A1 @ w2 + b2
        assert A1.max() / q1 < 2.0 ** 24, f"{case.name}: layer 1 needs {np.log2(A1.max() / q1):.1f} bits"
        assert A2.max() / q2 < 2.0 ** 24, f"{case.name}: layer 2 needs {np.log2(A2.max() / q2):.1f} bits"
        fed = w2.any(axis=0)
        flat = ref.canvas.transpose(1, 0, 2, 3).reshape(C, -1)
        assert np.all((flat != 0).any(axis=1)[fed]) and np.all((flat == 0).any(axis=1)[fed]), f"{case.name}: a channel is all zero or never zero"
    assert is_f32(ref.canvas), f"{case.name}: a canvas value is no float32 number"
    return ref


# ---------------------------------------------------------------------------------------------- what a case reaches
def reach(case, W=512):
    """From the geometry, for W persistent workgroups (min with the units, as fill_args): the points per unit, the units that
    overflow, the points per group of every ownership class, the other occupied units of an overflowing unit's group, the occupied layers per canvas cell."""
    g = case.grid
    _, uniq, inv, _ = indices(case)
    rows, cols, units = landing(g, uniq)
    nunits = case.batch * g.ny * g.upr
    W = min(W, nunits, 2048)
    load = np.bincount(units[inv], minlength=nunits)
    cell = (uniq[:, 0] * g.ny + rows) * g.nx + cols
    layers = np.bincount(cell).max() if len(cell) else 0
    group_of = (np.arange(nunits) // W) // GMAX * W + np.arange(nunits) % W          # (group, class) as one number
    group_load = np.bincount(group_of, weights=load).astype(np.int64)
    over = np.flatnonzero(load > OVERFLOW_POINTS)
    mates = [int(((group_of == group_of[u]) & (load > 0)).sum()) - 1 for u in over]   # other occupied units of the overflowing unit's group
    return dict(W=W, nunits=nunits, load=load, overflowing=over, group_mates=mates, group_load=group_load, layers=int(layers),
                collisions=bool(len(cell) != len(np.unique(cell))), occupied_units=int((load > 0).sum()))


# ---------------------------------------------------------------------------------------------- class X
def x_weights(rng, D):
    return (rng.integers(-2, 3, size=(D + 5, C)), rng.integers(-8, 9, size=C), rng.integers(-1, 2, size=(C, C)), rng.integers(-8, 9, size=C))


def _x_points(rng, g, D, xi, yi, count):
    """`count` points of cell (xi, yi): x, y, z multiples of 1/8, the other columns multiples of 1/8 in [0, 1]."""
    sub = 8 // g.ppm
    p = np.empty((count, D))
    p[:, 0] = g.min_x + xi / g.ppm + rng.integers(0, sub, size=count) / 8.0
    p[:, 1] = g.min_y + yi / g.ppm + rng.integers(0, sub, size=count) / 8.0
    p[:, 2] = rng.integers(-16, 17, size=count) / 8.0
    p[:, 3:] = rng.integers(0, 9, size=(count, D - 3)) / 8.0
    return p


def _forced_cells(g):
    """Cells every cloud with room for them holds: the clamp layers (all key rows that land on canvas row 0 at three columns, all key columns
    that land on the last canvas column at three rows), the canvas' corners and the columns of the right-border unit."""
    xs, ys = sorted({0, g.nx // 2, g.nx - 1}), sorted({0, min(17, g.ny - 1), min(g.ny, g.nx) - 1})
    cells = {(xi, yi) for xi in range(min(g.ny - 1, g.nx - 1), g.nx) for yi in ys}
    cells |= {(xi, yi) for yi in range(min(g.nx - 1, g.ny - 1), g.ny) for xi in xs}
    cells |= {(xi, yi) for xi in (0, g.nx - 1) for yi in (0, g.ny - 1)}
    first = UW * (g.upr - 1)
    cells |= {(xi, yi) for yi in range(first, min(g.nx, g.ny)) if yi - first < 3 or yi >= min(g.nx, g.ny) - 5 for xi in (3, g.nx - 4)}
    return cells


def _sparse_cells(g):
    """A unit with 20 points (two jobs: the two-way split over the waves) and a unit with 4 (one job: the four-way split)."""
    return {(g.nx // 2, 3): 8, (g.nx // 2, 4): 8, (g.nx // 2, 5): 4}, {(2, 10): 2, (2, 11): 1, (2, 20): 1}


def _points_of(rng, g, D, cells):
    """{(xi, yi): count} -> the points, in random order."""
    if not cells:
        return np.zeros((0, D))
    p = np.concatenate([_x_points(rng, g, D, xi, yi, k) for (xi, yi), k in cells.items()], axis=0)
    return p[rng.permutation(len(p))]


def _x_cloud(rng, g, D, ncells, dense=None, forced=True, extra=()):
    """A `spread` cloud: ncells random cells (and the forced and `extra` ones) with 1, 2, 4 or 8 points each.  dense: (xi, first yi) of
    the unit whose 32 cells hold 32 points each instead."""
    flat = rng.choice(g.nx * g.ny, size=min(ncells, g.nx * g.ny), replace=False)
    cells = {(int(c) // g.ny, int(c) % g.ny): 0 for c in flat}
    cells.update({c: 0 for c in (_forced_cells(g) if forced else ())})
    cells.update({c: 0 for c in extra})
    cells = {c: int(k) for c, k in zip(cells, rng.choice([1, 2, 4, 8], size=len(cells), p=[0.2, 0.3, 0.3, 0.2]))}
    if dense is not None:
        cells.update({(dense[0], dense[1] + j): 32 for j in range(UW)})
    return _points_of(rng, g, D, cells)


def _assemble(rng, g, D, clouds, live=None):
    """(B, nmax, D) with the rows past every cloud's points filled with in-range points (and the cloud `live` names cut short: the
    points past live[b] stay in the array and must not count)."""
    n = [len(c) for c in clouds]
    nmax = max(n)
    pts = np.empty((len(clouds), nmax, D))
    for b, c in enumerate(clouds):
        fill = _x_points(rng, g, D, 0, 0, nmax - len(c))
        fill[:, 0] = g.min_x + rng.integers(0, g.nx * 8 // g.ppm, size=len(fill)) / 8.0
        fill[:, 1] = g.min_y + rng.integers(0, g.ny * 8 // g.ppm, size=len(fill)) / 8.0
        pts[b] = np.concatenate([c, fill], axis=0)
    for b, k in (live or {}).items():
        n[b] = k
    return pts, n


DENSE_AT = {"S34": ((10, 0), (25, 0)), "S36": ((10, 0), (25, 0)), "W40": ((31, 0), (36, 0)), "T40": ((16, 0), (5, 0)), "B33": ((30, 32), (12, 0))}
B33_DENSE_CLOUD = 2      # the units W and 2 W / ... further on are the same row and columns of clouds 4, 6, ...: they hold points too


@functools.lru_cache(maxsize=None)
def x_case(grid, D, kind, variant=0):
    """Class X.  kind: sparse | spread | dense | empty; variant 1 of `dense` puts the dense unit elsewhere."""
    g = GRIDS[grid]
    rng = rng_of("X", grid, D, kind, variant)
    weights = x_weights(rng_of("Xw", D), D)
    B = BATCH.get(grid, 1)
    name = f"{grid} D {D} X {kind}" + (f" v{variant}" if variant else "")
    if kind == "empty":
        return Case(name, "X", g, D, np.zeros((B, 0, D)), [0] * B, weights)
    dense = DENSE_AT[grid][variant] if kind == "dense" else None
    sparse_a, sparse_b = _sparse_cells(g)
    live = {}
    if B == 1:
        dense_cloud = 0
        clouds = [_points_of(rng, g, D, {**sparse_a, **sparse_b}) if kind == "sparse" else _x_cloud(rng, g, D, 200, dense)]
    elif kind == "sparse":       # the unit of 20 points in cloud 1, the unit of 4 in cloud 30, nothing else anywhere
        clouds = [_points_of(rng, g, D, {1: sparse_a, 30: sparse_b}.get(b, {})) for b in range(B)]
    else:
        dense_cloud = B33_DENSE_CLOUD
        clouds = []
        for b in range(B):
            extra = [(dense[0], dense[1] + 8)] if (dense and b in (4, 6, 10)) else ()
            clouds.append(np.zeros((0, D)) if b in B33_EMPTY else
                          _x_cloud(rng, g, D, 28, dense if b == dense_cloud else None, forced=False, extra=extra))
        # the truncated cloud: four more cells of in-range points behind its n
        live[B33_TRUNCATED] = len(clouds[B33_TRUNCATED])
        clouds[B33_TRUNCATED] = np.concatenate([clouds[B33_TRUNCATED], _x_cloud(rng, g, D, 4, forced=False)], axis=0)
    pts, n = _assemble(rng, g, D, clouds, live)
    return _revived(Case(name, "X", g, D, pts, n, weights, (dense_cloud,) + dense if dense else None))


def _revived(case):
    # The coordinates dominate the features, so a column of w2 can come out negative for every point of a cloud: such an output channel
    # would be all zero and check nothing.  Those columns (and their bias) change sign: still integers in [-1, 1] and [-8, 8].
    f = forward64(case, want_tol=False).dec
    h2 = np.maximum(f @ case.w1.astype(f64) + case.b1, 0.0) @ case.w2.astype(f64) + case.b2
    dead = ~(h2 > 0).any(axis=0)
    case.w2[:, dead] = -case.w2[:, dead]
    case.b2[dead] = np.abs(case.b2[dead])
    return case


@functools.lru_cache(maxsize=None)
def x_scan_case(max_points, grid="S31", D=4):
    """Class X at batch 2 with exactly max_points rows per cloud: cloud 0 has fewer live rows (in-range points behind them), every row
    of cloud 1 is live (a spread cloud topped up with one-point cells).  On S31 the key space has 2 x 32 x 32 = SCAN_TILE cells."""
    g = GRIDS[grid]
    rng = rng_of("scan", grid, D, max_points)
    weights = x_weights(rng_of("Xw", D), D)
    name = f"{grid} D {D} X batch 2 max_points {max_points}"
    if max_points == 0:
        return Case(name, "X", g, D, np.zeros((2, 0, D)), [0, 0], weights)
    a, b = _x_cloud(rng, g, D, 150), _x_cloud(rng, g, D, 150, forced=False)
    used = set(map(tuple, np.floor((b[:, :2] - (g.min_x, g.min_y)) * g.ppm).astype(int)))
    free = [c for c in ((xi, yi) for xi in range(g.nx) for yi in range(g.ny)) if c not in used]
    more = [free[i] for i in rng.permutation(len(free))[:max_points - len(b)]]
    b = np.concatenate([b] + [_x_points(rng, g, D, xi, yi, 1) for xi, yi in more], axis=0)
    assert len(a) < max_points == len(b)
    pts, n = _assemble(rng, g, D, [a, b[rng.permutation(len(b))]])
    return _revived(Case(name, "X", g, D, pts, n, weights))


def x_cases():
    """(grid, D, kind) of every class X case of the issue's table."""
    out = [(grid, D, "spread") for grid in SMALL for D in WIDTHS]
    out += [(grid, D, kind) for grid in RICH for D in WIDTHS for kind in ("sparse", "dense")]
    out += [("B33", D, "spread") for D in (4, 11)]
    return out


KNOB_CASES = [(grid, D, kind) for grid in ("S34", "S36", "W40", "B33") for D in (4, 11) for kind in ("sparse", "spread", "dense")]
KNOB_EXTRA = [("S34", 8, "spread", "mfma"), ("S36", 8, "spread", "mfma"), ("S34", 11, "spread", "valu"), ("S36", 11, "spread", "valu")]
SEQUENCE = [("S36", 11, "dense", 0), ("S36", 11, "dense", 1), ("S36", 4, "sparse", 0), ("S36", 8, "empty", 0), ("S36", 4, "dense", 0),
            ("S36", 8, "spread", 0), ("S36", 11, "dense", 0)]


# ---------------------------------------------------------------------------------------------- class G
ODD_CELLS = ((2, 2), (9, 4), (4, 11))      # (xi, yi) of the cells that hold exactly 3, 5 and 7 points


def edge_rows(g, D, rng):
    """The grid's edge rows: x and y at min (kept), at max (dropped) and one ulp below max (kept; may round up to cell nx / ny), alone
    and together; NaN, +-inf; -0.0 where min is 0; interior cell borders and one ulp below; cells of 3, 5 and 7 points, exact duplicates;
    z of 1e6 and 1e-6."""
    F = lambda v: f32(v)
    below = lambda v: np.nextafter(F(v), F(-np.inf))
    xs = [F(g.min_x), F(g.max_x), below(g.max_x)]
    ys = [F(g.min_y), F(g.max_y), below(g.max_y)]
    xm, ym = F(g.min_x + 5.3), F(g.min_y + 6.1)
    xy = [(x, ym) for x in xs] + [(xm, y) for y in ys] + [(x, y) for x in xs for y in ys]
    for bad in (np.nan, np.inf, -np.inf):
        xy += [(F(bad), ym), (xm, F(bad)), (F(bad), F(bad))]
    if g.min_x == 0:
        xy += [(F(-0.0), ym), (F(-0.0), ys[2])]
    if g.min_y == 0:
        xy += [(xm, F(-0.0))]
    for k in (1, 7, g.nx - 1):
        xb = F(g.min_x + k / g.ppm)
        xy += [(xb, ym), (below(xb), ym), (xb, F(g.min_y + k / g.ppm)), (below(xb), below(g.min_y + k / g.ppm))]
    for k in (1, g.ny - 1):
        yb = F(g.min_y + k / g.ppm)
        xy += [(xm, yb), (xm, below(yb))]
    for m, (cx, cy) in zip((3, 5, 7), ODD_CELLS):                       # cells of 3, 5, 7 points
        xy += [(F(g.min_x + (cx + t) / g.ppm), F(g.min_y + (cy + s) / g.ppm)) for t, s in rng.uniform(0.05, 0.95, size=(m, 2))]
    rows = np.zeros((len(xy), D), f32)
    rows[:, :2] = np.array(xy, f32)
    rows[:, 2] = rng.standard_normal(len(xy))
    rows[:, 3:] = rng.uniform(0, 1, size=(len(xy), D - 3))
    dup = np.repeat(rows[3:4], 3, axis=0)                                # exact duplicates (of the point at y = min_y)
    zz = np.repeat(rows[:1], 4, axis=0)
    zz[:, 0], zz[:, 1] = F(g.min_x + 3.3), F(g.min_y + 1.2)
    zz[:, 2] = (1e6, 1e-6, 1e6, 1e-6)
    zz[2:, 0] = F(g.min_x + 6.3)                                         # one z pair shares a cell, the other one too: 1e6 beside 1e-6 twice
    return np.concatenate([rows, dup, zz], axis=0)


@functools.lru_cache(maxsize=None)
def g_case(grid, D, kind="spread"):
    """Class G: an arbitrary float32 cloud (some of it outside the grid), the edge rows, N(0, 1)-scaled weights.  dense: 1100 further
    points on the 32 cells of one unit."""
    g = GRIDS[grid]
    rng = rng_of("G", grid, D, kind)
    n = 600
    p = np.empty((n, D))
    p[:, 0] = rng.uniform(g.min_x - 1, g.max_x + 1, size=n)
    p[:, 1] = rng.uniform(g.min_y - 1, g.max_y + 1, size=n)
    p[:, 2] = rng.standard_normal(n)
    p[:, 3:] = rng.uniform(0, 1, size=(n, D - 3))
    cell = np.floor((p[:, :2] - (g.min_x, g.min_y)) * g.ppm)
    p = p[~np.any([(cell == c).all(axis=1) for c in ODD_CELLS], axis=0)]          # (the cells of 3, 5 and 7 points keep their counts)
    parts = [p.astype(f32), edge_rows(g, D, rng)]
    dense_unit = None
    if kind == "dense":
        xi, y0 = DENSE_AT[grid][0]
        d = np.empty((1100, D))
        d[:, 0] = g.min_x + (xi + rng.uniform(0.01, 0.99, size=1100)) / g.ppm
        d[:, 1] = g.min_y + (y0 + rng.uniform(0.01, 31.99, size=1100)) / g.ppm
        d[:, 2] = rng.standard_normal(1100)
        d[:, 3:] = rng.uniform(0, 1, size=(1100, D - 3))
        parts.append(d.astype(f32))
        dense_unit = (0, xi, y0)
    pts = np.concatenate(parts, axis=0)
    pts = pts[rng.permutation(len(pts))][None]
    K1 = D + 5
    weights = (rng.standard_normal((K1, C)) / np.sqrt(K1), rng.standard_normal(C), rng.standard_normal((C, C)) / 8.0, rng.standard_normal(C))
    return Case(f"{grid} D {D} G {kind}", "G", g, D, pts, [pts.shape[1]], weights, dense_unit)


def g_cases():
    return [(grid, D, "spread") for grid in SMALL for D in WIDTHS] + [(grid, D, "dense") for grid in ("S34", "W40", "T40") for D in (4, 11)]


# ---------------------------------------------------------------------------------------------- comparison
def mismatch(got, want, what):
    """None when got == want element for element (float64 on both sides), else the message."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"{what}: shape {got.shape} vs {want.shape}"
    if np.array_equal(got, want):
        return None
    bad = got != want
    first = tuple(int(v) for v in np.argwhere(bad)[0])
    return (f"{what}: {int(bad.sum())} of {bad.size} elements differ from float64; worst |difference| "
            f"{float(np.nanmax(np.abs(got[bad].astype(f64) - want[bad]))):.6g}; first at {first}: kernel {got[first]!r}, float64 {want[first]!r}")


def assert_exact(got, want, what):
    msg = mismatch(got, want, what)
    assert msg is None, msg


def assert_within(got, ref, what):
    """|got - float64| <= the derived bound, element for element (class G)."""
    got = np.asarray(got, f64)
    assert got.shape == ref.canvas.shape, f"{what}: shape {got.shape} vs {ref.canvas.shape}"
    err = np.abs(got - ref.canvas)
    bad = ~(err <= ref.tol)
    if bad.any():
        first = tuple(int(v) for v in np.argwhere(bad)[0])
        ratio = np.where(ref.tol > 0, err / np.where(ref.tol > 0, ref.tol, 1), np.where(err > 0, np.inf, 0))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the derived bound; worst error / bound "
                             f"{float(np.nanmax(ratio)):.3g}; first at {first}: {got[first]!r} vs {ref.canvas[first]!r} +- {ref.tol[first]:.3g}")
