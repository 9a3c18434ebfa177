"""Plain numpy references of the per-tick glue kernels (include/lav_amd.h, sections 6 and 6c: lav_extract_peaks, lav_det_decode,
lav_stack_sweeps, lav_merge_ticks), the seeded input builders and the case tables shared by tests/test_frame_ref_host.py (CPU)
and tests/test_gpu_frame_edges.py (MI355X).

The references restate the header's rules and nothing else: no project code is imported here.  Every value the builders
produce is exactly representable (integers / 1024, multiples of 1 / 64), so a kernel is held to them bit for bit."""
from __future__ import annotations

import functools

import numpy as np

TILE = 32                       # frame.hip: side of a peak tile in pixels
REG_CANDIDATES = 2048           # frame.hip: 128 lanes x PEAK_PER_LANE candidates of a class stay in registers; more are scanned
FILLER = np.float32(-1e5)       # score of a row beyond the number of non-suppressed pixels
NAN_BITS = 0x7FC00000           # the +NaN of the NaN cases


# ------------------------------------------------------------------------------------------------ peaks
def ordered_u32(v):
    """The kernel's total order on float32: the monotone unsigned map of the bit pattern (negative: all bits flipped; otherwise
    the sign bit set).  -0.0 sorts below +0.0, a +NaN above +Inf."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def window_max(plane, r, pad=-np.inf):
    """Maximum over the (2r+1)^2 window of every pixel, `pad` outside the map, NaN ignored (np.fmax)."""
    H, W = plane.shape
    p = np.full((H + 2 * r, W + 2 * r), pad, np.float32)
    p[r:r + H, r:r + W] = plane
    rowmax = p[:, 0:W].copy()
    for d in range(1, 2 * r + 1):
        rowmax = np.fmax(rowmax, p[:, d:d + W])
    m = rowmax[0:H].copy()
    for d in range(1, 2 * r + 1):
        m = np.fmax(m, rowmax[d:d + H])
    return m


def sigmoid_exact(logits):
    """float32 sigmoid of logits whose 1 / (1 + expf(-v)) is exact whatever the last bits of expf: v <= -120 gives 0 (expf
    overflows to +Inf), v == 0 gives 0.5, v >= 20 gives 1 (expf(-20) < 2^-25 vanishes in 1 + e).  Anything else raises."""
    v = np.asarray(logits, np.float32)
    lo, mid, hi = v <= -120, v == 0, v >= 20
    if not (lo | mid | hi).all():
        raise ValueError("sigmoid_exact: a logit whose float32 sigmoid depends on the rounding of expf")
    return np.where(lo, np.float32(0), np.where(mid, np.float32(0.5), np.float32(1))).astype(np.float32)


def peaks_ref(heat, size, ori, ks, max_det, apply_sigmoid=False):
    """lav_extract_peaks: heat (ncls,H,W), size (cs,H,W), ori (co,H,W) -> (rows (ncls, max_det, 3+cs+co), candidates_per_class).
    A pixel survives when not (window maximum > value); survivors by descending ordered_u32(value), ties by ascending y*W + x;
    the first max_det give (score, x, y, size.., ori..); the remaining rows are (-1e5, 0, 0, 0..).  candidates_per_class: the sum
    over 32 x 32 tiles of min(survivors in the tile, max_det) - what the kernel's last workgroup selects from."""
    heat = sigmoid_exact(heat) if apply_sigmoid else np.asarray(heat, np.float32)
    ncls, H, W = heat.shape
    gathered = np.concatenate([np.asarray(size, np.float32).reshape(-1, H * W), np.asarray(ori, np.float32).reshape(-1, H * W)])
    rows = np.zeros((ncls, max_det, 3 + gathered.shape[0]), np.float32)
    rows[:, :, 0] = FILLER
    cands = []
    with np.errstate(invalid="ignore"):
        for c in range(ncls):
            alive = ~(window_max(heat[c], ks // 2) > heat[c])
            idx = np.flatnonzero(alive.reshape(-1)).astype(np.uint64)
            key = (ordered_u32(heat[c].reshape(-1)[idx]).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)
            best = idx[np.argsort(key)[::-1][:max_det]].astype(np.int64)      # keys are unique: they carry the pixel index
            n = len(best)
            rows[c, :n, 0] = heat[c].reshape(-1)[best]
            rows[c, :n, 1] = best % W
            rows[c, :n, 2] = best // W
            rows[c, :n, 3:] = gathered[:, best].T
            tiles = np.zeros((-(-H // TILE) * TILE, -(-W // TILE) * TILE), np.int64)
            tiles[:H, :W] = alive
            per_tile = tiles.reshape(tiles.shape[0] // TILE, TILE, tiles.shape[1] // TILE, TILE).sum((1, 3))
            cands.append(int(np.minimum(per_tile, max_det).sum()))
    return rows, cands


def filler_rows(rows):
    """Number of rows per class that carry the filler (-1e5, 0, 0, 0..) exactly."""
    fill = (rows[:, :, 0] == FILLER) & ~rows[:, :, 1:].any(-1)
    return fill.sum(1)


# ------------------------------------------------------------------------------------------------ peak inputs
def gather_maps(H, W, seed):
    """Random size / ori maps (2,H,W) each: the gathered columns are compared bit for bit as well."""
    g = np.random.default_rng([seed, 77])
    return g.standard_normal((2, H, W)).astype(np.float32), g.standard_normal((2, H, W)).astype(np.float32)


def tie_map(shape, levels, seed):
    """Tie-rich map: integers / 1024 from `levels` levels, so equal scores are common.  Odd planes are shifted below zero
    (the order map's other branch, and the planes on which a zero padding would differ from -inf).  No -0.0."""
    ncls, H, W = shape
    k = np.random.default_rng([seed, 1]).integers(0, levels, shape)
    k = k - levels * (np.arange(ncls) % 2)[:, None, None]
    return k.astype(np.float32) / np.float32(1024)


def plateau_map(shape, seed, ks=7, n_equal=24, n_high=5, cluster=False, extra=()):
    """Plateau map: a 0.5 base (every base pixel outside a peak's window survives: a full tile yields max_det candidates),
    `n_equal` isolated 0.75 pixels, `n_high` isolated distinct values 49/64.., placed by a seeded generator, plus one probe
    triple per plane - 56/64 with 55/64 at distance r (suppressed) and 54/64 at distance r + 1 (survives) - which a window of
    another radius treats differently.  cluster: plane 0 also gets one full tile whose (r+1)-lattice holds 64 values above
    everything else (59 x 58/64, then 59/64 .. 63/64): the top 64 of the plane come from ONE tile.  Odd planes are shifted by -1
    (all values negative).  extra: (plane, y, x) of further 0.75 pixels."""
    ncls, H, W = shape
    r = ks // 2
    heat = np.full(shape, 0.5, np.float32)
    for c in range(ncls):
        g = np.random.default_rng([seed, 2, c])
        free = np.ones((H, W), bool)

        def claim(y, x, rad):
            free[max(0, y - rad):y + rad + 1, max(0, x - rad):x + rad + 1] = False

        for (pc, y, x) in extra:
            if pc == c:
                heat[c, y, x] = 0.75
                claim(y, x, 2 * r + 2)
        if cluster and c == 0:
            ty, tx = int(g.integers(0, H // TILE)) * TILE, int(g.integers(0, W // TILE)) * TILE
            ys, xs = np.meshgrid(np.arange(ty, ty + TILE, r + 1), np.arange(tx, tx + TILE, r + 1), indexing="ij")
            ys, xs = ys.reshape(-1), xs.reshape(-1)
            heat[c, ys, xs] = 58 / 64
            top = g.choice(len(ys), 5, replace=False)
            heat[c, ys[top], xs[top]] = (59 + np.arange(5)) / 64
            claim(ty + TILE // 2, tx + TILE // 2, TILE // 2 + 2 * r + 2)

        def place(value, lo_y=0, lo_x=0):
            for _ in range(10000):
                y, x = int(g.integers(0, H - lo_y)), int(g.integers(0, W - lo_x))
                if free[y, x]:
                    heat[c, y, x] = value
                    return y, x
            raise RuntimeError("plateau_map: no free pixel left")

        if H > 2 * r + 2 and W > 2 * r + 2:
            y, x = place(56 / 64, r + 1, r)
            heat[c, y, x + r] = 55 / 64
            heat[c, y + r + 1, x] = 54 / 64
            claim(y, x, 3 * r + 3)
        for k in range(n_high):
            claim(*place((49 + k) / 64), 2 * r + 2)
        for _ in range(n_equal):
            claim(*place(0.75), 2 * r + 2)
        if c % 2:
            heat[c] -= 1
    return heat


def sigmoid_logits(shape, block, seed, values=(-200, -120, 0, 20, 40)):
    """Logits from {-200, -120, 0, 20, 40} (or a subset) in block x block squares, block no divisor of the tile: plateaus of
    exact 0, 0.5 and 1 that cross tile borders."""
    ncls, H, W = shape
    g = np.random.default_rng([seed, 3])
    pick = g.integers(0, len(values), (ncls, -(-H // block), -(-W // block)))
    v = np.array(values, np.float32)[pick]
    return np.ascontiguousarray(np.repeat(np.repeat(v, block, 1), block, 2)[:, :H, :W])


def smooth_map(shape, seed):
    """Tie-free map with real NMS structure: box-smoothed noise (the existing GPU test's input without its plateau)."""
    ncls, H, W = shape
    z = np.random.default_rng([seed, 4]).standard_normal((ncls, H + 4, W + 4))
    s = sum(z[:, dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)) / 25
    return (1 / (1 + np.exp(-8 * s))).astype(np.float32)


def nan_map(shape=(3, 40, 56), seed=9, plane=1):
    """smooth_map with one +NaN (0x7fc00000) beside the largest pixel of `plane`: (with the NaN, without it, (y, x))."""
    clean = smooth_map(shape, seed)
    H, W = shape[1:]
    y, x = np.unravel_index(int(np.argmax(clean[plane])), (H, W))
    x = x + 1 if x + 1 < W else x - 1
    heat = clean.copy()
    heat[plane].reshape(-1).view(np.uint32)[y * W + x] = NAN_BITS
    return heat, clean, (int(y), int(x))


# name -> (kind, shape, ks, max_det, builder arguments).  Kinds of the ties-and-caps table: "tie" (every plane's expected rows hold
# two distinct scores and three equal ones), "top1" (max_det = 1: every plane's maximum is attained at three pixels or more, so the
# tie rule alone picks the row), "few" (fewer survivors than rows: filler rows), "single" (one pixel, one row).
TIE_CASES = {
    "t32": ("tie", (1, 32, 32), 7, 15, dict(levels=300, seed=1)),
    "t33x65": ("tie", (2, 33, 65), 3, 20, dict(levels=400, seed=2)),
    "t40c8": ("tie", (8, 40, 40), 15, 64, dict(levels=200, seed=3)),
    "t8x300": ("top1", (3, 8, 300), 1, 1, dict(levels=16, seed=4)),
    "t64x96": ("tie", (2, 64, 96), 7, 64, dict(levels=900, seed=5)),
    "t31x97": ("tie", (1, 31, 97), 5, 33, dict(levels=400, seed=6)),
    "t3": ("few", (1, 3, 3), 7, 15, dict(levels=3, seed=7)),
    "t1": ("single", (1, 1, 1), 1, 1, dict(levels=5, seed=8)),
}
# name -> (kind, shape, max_det, candidates per class, builder arguments); ks = 7.  "bound": exactly 2048 candidates, the last count
# that stays in registers; "scan": more, the list is rescanned per row; "regs": fewer.
PATH_CASES = {
    "p128x256": ("bound", (1, 128, 256), 64, 2048, dict(seed=11, cluster=True)),
    "p192": ("scan", (1, 192, 192), 64, 2304, dict(seed=12)),
    "p129x256": ("scan", (1, 129, 256), 64, 2290, dict(seed=16, n_equal=80, extra=((0, 126, 40), (0, 127, 200)))),
    "p320": ("scan", (2, 320, 320), 64, 6400, dict(seed=14, cluster=True)),
    "p320d20": ("regs", (2, 320, 320), 20, 2000, dict(seed=14, cluster=True)),
}
SIGMOID_CASES = {
    "s70x100": ((2, 70, 100), 7, 20, dict(block=12, seed=21)),
    "s96": ((1, 96, 96), 3, 64, dict(block=20, seed=22)),
    "s50x90": ((1, 50, 90), 7, 64, dict(block=3, seed=23, values=(-200, -120) * 40 + (0,))),   # a few 0.5, then the zeros
}


@functools.lru_cache(maxsize=None)
def peak_case(name):
    """(heat, size, ori, ks, max_det, apply_sigmoid, expected rows, candidates per class) of a case of the three tables; computed
    once per process and shared: treat the arrays as read-only."""
    if name in TIE_CASES:
        _, shape, ks, max_det, kw = TIE_CASES[name]
        heat, sig = tie_map(shape, **kw), False
    elif name in PATH_CASES:
        _, shape, max_det, _, kw = PATH_CASES[name]
        ks, heat, sig = 7, plateau_map(shape, ks=7, **kw), False
    else:
        shape, ks, max_det, kw = SIGMOID_CASES[name]
        heat, sig = sigmoid_logits(shape, **kw), True
    size, ori = gather_maps(shape[1], shape[2], kw["seed"])
    rows, cand = peaks_ref(heat, size, ori, ks, max_det, sig)
    for a in (heat, size, ori, rows):
        a.setflags(write=False)
    return heat, size, ori, ks, max_det, sig, rows, cand


# ------------------------------------------------------------------------------------------------ detection decode
def det_decode_ref(rows, cls, min_score, ego_xy, near_px, far_px, min_box, centre_xy, skip_px, ppm):
    """lav_det_decode on rows (ncls, max_det, 7) float32 -> (actors float32 [2*max_det] + [max_det], n).  float64 on widened
    float32, strict inequalities as the header lists them: keep a row when score > min_score, near_px < dist < far_px with dist
    between the TRUNCATED integer coordinates and the truncated ego pixel, not fmax(w, h) < min_box, and the distance of the
    (truncated) coordinates to the centre > skip_px.  Survivors in row order: ((X - cx) / ppm, (Y - cy) / ppm) rounded to
    float32, headings atan2(ori1, ori0); entries beyond n are zero."""
    r = np.asarray(rows, np.float32)[cls]
    max_det = r.shape[0]
    s, w, h = r[:, 0].astype(np.float64), r[:, 3].astype(np.float64), r[:, 4].astype(np.float64)
    xi, yi = np.trunc(r[:, 1]).astype(np.int64), np.trunc(r[:, 2]).astype(np.int64)
    ex, ey = int(ego_xy[0]), int(ego_xy[1])
    X, Y = xi.astype(np.float64), yi.astype(np.float64)
    cx, cy = float(centre_xy[0]), float(centre_xy[1])
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(((xi - ex) ** 2 + (yi - ey) ** 2).astype(np.float64))
        ok = (s > float(min_score)) & (dist > float(near_px)) & (dist < float(far_px)) & ~(np.fmax(w, h) < float(min_box))
        ok &= np.sqrt((X - cx) ** 2 + (Y - cy) ** 2) > float(skip_px)
    j = np.flatnonzero(ok)
    actors = np.zeros(3 * max_det, np.float32)
    actors[0:2 * len(j):2] = ((X[j] - cx) / float(ppm)).astype(np.float32)
    actors[1:2 * len(j):2] = ((Y[j] - cy) / float(ppm)).astype(np.float32)
    actors[2 * max_det:2 * max_det + len(j)] = np.arctan2(r[j, 6].astype(np.float64), r[j, 5].astype(np.float64)).astype(np.float32)
    return actors, len(j)


# The frame's constants (thresholds are Python floats: 0.2 and 0.1 * ppm = 0.4 are NOT float32 values), and the same with the two
# thresholds a float32 can sit on exactly: there a score / box equal to its threshold exists, and `>` against `>=` shows.
DECODE = dict(min_score=0.2, ego_xy=(160, 280), near_px=2.0, far_px=120.0, min_box=0.4, centre_xy=(160.0, 240.0), skip_px=4.0, ppm=4.0)
F32 = np.float32
DECODE_EXACT = dict(DECODE, min_score=float(F32(0.2)), min_box=float(F32(0.4)))


def _det_row(score=0.9, dx=20, dy=-30, w=1.5, h=0.9, co=0.6, si=-0.8):
    return [score, DECODE["ego_xy"][0] + dx, DECODE["ego_xy"][1] + dy, w, h, co, si]


# (label, row, kept with DECODE).  One filter per row; every other field passes with room to spare.
DECODE_THRESHOLD_ROWS = (
    ("score 0.2f: > 0.2 as a double", _det_row(score=F32(0.2)), True),
    ("score one float32 below 0.2f", _det_row(score=np.nextafter(F32(0.2), F32(0))), False),
    ("filler score -1e5", _det_row(score=FILLER), False),
    ("NaN score", _det_row(score=np.nan), False),
    ("distance == near_px: offset (2, 0)", _det_row(dx=2, dy=0), False),
    ("offset (2, 1)", _det_row(dx=2, dy=1), True),
    ("distance == far_px: offset (72, -96)", _det_row(dx=72, dy=-96), False),
    ("offset (72, -95)", _det_row(dx=72, dy=-95), True),
    ("max(w, h) == 0.4f: not below min_box", _det_row(w=F32(0.4), h=0.1), True),
    ("max(w, h) one float32 below 0.4f", _det_row(w=0.1, h=np.nextafter(F32(0.4), F32(0))), False),
    ("sizes NaN", _det_row(w=np.nan, h=np.nan), True),
    ("distance to the centre == skip_px: centre + (0, 4)", [0.9, 160, 244, 1.5, 0.9, 1.0, 0.0], False),
    ("centre + (1, 4)", [0.9, 161, 244, 1.5, 0.9, 0.0, 1.0], True),
    ("161.9 truncates to 161, 244.9 to 244", [0.9, 161.9, 244.9, 1.5, 0.9, -1.0, 0.0], True),
    ("160.9, 244.9 truncate onto the skip circle", [0.9, 160.9, 244.9, 1.5, 0.9, -1.0, 0.0], False),
)


def decode_rows(kind, ncls=2, cls=1):
    """Constructed peak rows (ncls, max_det, 7) for lav_det_decode; the other class's rows would all be kept, so reading the
    wrong class shows.  "threshold": DECODE_THRESHOLD_ROWS (max_det 15); "all64": max_det = 64 and every row kept, distinct
    positions and headings (lane 63's prefix is used); "none64": 64 rows, each dropped by one of the filters."""
    if kind == "threshold":
        own = np.array([r for _, r, _ in DECODE_THRESHOLD_ROWS], np.float32)
    elif kind == "all64":
        j = np.arange(64)
        own = np.array([_det_row(score=1 - j_ / 128, dx=-60 + 2 * j_, dy=-70 + (j_ % 7), co=np.cos(0.1 * j_ - 3), si=np.sin(0.1 * j_ - 3))
                        for j_ in j], np.float32)
    elif kind == "none64":
        drops = [r for _, r, kept in DECODE_THRESHOLD_ROWS if not kept]
        own = np.array([drops[j % len(drops)] for j in range(64)], np.float32)
    else:
        raise KeyError(kind)
    other = np.array([_det_row(score=0.5 + 0.001 * j, dx=10 + j, dy=-40) for j in range(len(own))], np.float32)
    rows = np.stack([own if c == cls else other for c in range(ncls)])
    return rows


# ------------------------------------------------------------------------------------------------ lidar glue
def stack_sweeps_ref(fused, ring, slot, sweeps, R, t):
    """lav_stack_sweeps: sweep 0 is `fused`, sweep s > 0 is ring[sweeps[s]] (before the history write); xyz' = ((v0*R[0,c] +
    v1*R[1,c]) + v2*R[2,c]) + t[c] in float32 operations, one rounding each, left to right; feature columns unchanged; one-hot
    sweep column appended.  Returns (out (S*rows, dim+S), ring after ring[slot] = fused)."""
    fused, ring = np.asarray(fused, np.float32), np.asarray(ring, np.float32)
    R, t = np.asarray(R, np.float32), np.asarray(t, np.float32).reshape(-1, 3)
    S, (rows, dim) = len(sweeps), fused.shape
    out = np.zeros((S, rows, dim + S), np.float32)
    with np.errstate(invalid="ignore"):
        for s in range(S):
            v = fused if s == 0 else ring[int(sweeps[s])]
            for c in range(3):
                out[s, :, c] = ((v[:, 0] * R[s, 0, c] + v[:, 1] * R[s, 1, c]) + v[:, 2] * R[s, 2, c]) + t[s, c]
            out[s, :, 3:dim] = v[:, 3:]
            out[s, :, dim + s] = 1
    after = ring.copy()
    after[int(slot)] = fused
    return out.reshape(S * rows, dim + S), after


def stack_inputs(rows, seed, slots=15, slot=12, sweeps=(12, 7, 2), nan_rows=()):
    """Seeded inputs of lav_stack_sweeps: (fused, ring, slot, sweeps, R (3,3,3), t (3,3)); nan_rows: points whose x is NaN in the
    new sweep and in the history, as lav_merge_ticks marks them.  The rotations are float32 roundings of real poses."""
    g = np.random.default_rng([seed, 5])
    ring = (g.standard_normal((slots, rows, 8)) * 20).astype(np.float32)
    fused = (g.standard_normal((rows, 8)) * 20).astype(np.float32)
    for i in nan_rows:
        fused[i, 0] = np.nan
        ring[sweeps[1], (i + 1) % rows, 0] = np.nan
    R = np.zeros((3, 3, 3), np.float32)
    t = np.zeros((3, 3), np.float32)
    for s in range(3):
        o = 0.105 * s + 0.013
        R[s] = [[np.cos(o), np.sin(o), 0], [-np.sin(o), np.cos(o), 0], [0, 0, 1]]
        t[s] = [1.55 * s, -0.35 * s, 0]
    return fused, ring, slot, list(sweeps), R, t


EGO_BOX = ((F32(-2.4), F32(0)), (F32(-0.8), F32(0.8)), (F32(-1.5), F32(-1)))   # open intervals of x, y, z (lav_agent_fast.py:450-452)


def merge_ticks_ref(tick, prev):
    """lav_merge_ticks: (cur = cat([tick, prev]) with x = NaN where the point lies strictly inside the ego box, prev after = tick)."""
    cur = np.concatenate([tick, prev]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        inside = np.ones(len(cur), bool)
        for k, (lo, hi) in enumerate(EGO_BOX):
            inside &= (cur[:, k] > lo) & (cur[:, k] < hi)
    cur[inside, 0] = np.nan
    return cur, np.array(tick, np.float32), inside


def merge_inputs(rows, seed):
    """(tick, prev) of `rows` points: random points around the box, then - as far as the rows reach - the twelve face probes:
    a point exactly on each of the six faces (kept) and the point one float32 inside it (marked), the other coordinates mid-box."""
    g = np.random.default_rng([seed, 6])
    lo, hi = (-3, -1.2, -2, 0), (1, 1.2, -0.5, 1)
    tick = g.uniform(lo, hi, (rows, 4)).astype(np.float32)
    prev = g.uniform(lo, hi, (rows, 4)).astype(np.float32)
    probes = []
    for k, (lo, hi) in enumerate(EGO_BOX):
        for face, toward in ((lo, hi), (hi, lo)):
            for v in (face, np.nextafter(face, toward)):
                p = np.array([-1.0, 0.1, -1.2, 0.5], np.float32)
                p[k] = v
                probes.append(p)
    for i, p in enumerate(probes):      # alternately into the two halves of cur
        if i // 2 < rows:
            (tick if i % 2 == 0 else prev)[i // 2] = p
    return tick, prev
