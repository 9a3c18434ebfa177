"""The trainers' visual logs (lav/utils/logger.py: log_bev_info, log_lidar_info, log_seg_info, log_bra_info) as one frame format, its
NumPy specification, the four frames' table builders and the writer that keeps a run's frames as PNG files.

A frame is three host-built tables.  PANELS: a rectangle of the frame and a source drawn into it pixel for pixel - an (h, w, 3) uint8
image, an (h, w) integer label map or (C, h, w) float32 logits through the CARLA palette (label i + 1 -> SEM_COLORS[labels[i]], the
rest black: visualize_semantic_processed; the logits' argmax by np.argmax's rule), (C, h, w) float32 planes as
imshow(mean(axis=0), cmap='gray'), or a colour.  PRIMITIVES: dots and thickness-2 segments by debug_view.covers's integer rules, and
filled convex polygons (every int64 edge function of the pixel centre >= 0, or every one <= 0, inside the polygon's box); drawn in
order, later over earlier, each clipped to the panel it names.  TEXT: rows of 7-bit ASCII in debug_view.FONT at their origins,
white, clipped to the frame.  log_view_numpy is the specification; lav_log_view (csrc/log_view.hip, ops.log_view) composes the same
frame on the device from the tensors a logged step left in HBM, bit for bit (tests/test_gpu_log_view.py).

Pinned against the reference: the palette (tests/golden/log_view.npz, written by the reference's visualize_semantic_processed) and
the corners of the detection boxes (matplotlib's Rectangle built by the reference's expression).  UNPINNED: (1) matplotlib's
anti-aliased rasterisation and its scaling of the axes into a figure - integer rules of this project at one frame pixel per source
pixel instead; (2) the text - debug_view.FONT, not matplotlib's title font; (3) imshow's normalisation, restated: grey =
floor((m - lo) * 255 / (hi - lo)) in float64, m the float64 channel mean (sum in channel order over the count), lo / hi the smallest /
largest finite mean; 0 where hi == lo or m is not finite.
"""
from __future__ import annotations

import os
import struct
import zlib
from collections import namedtuple

import numpy as np

from ..agent.debug_view import CMD_NAMES, COORD_LIMIT, DOT, FONT, GLYPH_H, GLYPH_STEP, GLYPH_W, JET_U8, SEGMENT, _to_pixel, covers, jet_index

IMAGE_U8, LABELS, LOGITS, PLANES, SOLID = range(5)
CONVEX = 2
MAX_PANELS, MAX_LABELS, MAX_PRIMS, MAX_ROWS, TEXT_LEN, MAX_SIDE = 8, 8, 1 << 16, 64, 64, 16384
PANEL_DTYPE = np.dtype([("kind", "<i4"), ("rect", "<i4", (4,)), ("source", "<i4"), ("colour", "u1", (4,)), ("nlabels", "<i4"),
                        ("labels", "<i4", (MAX_LABELS,))])                  # rect = (x, y, w, h); source = index into `sources`
PRIM_DTYPE = np.dtype([("kind", "<i4"), ("p0", "<i4", (2,)), ("p1", "<i4", (2,)), ("radius", "<i4"), ("colour", "u1", (4,)), ("panel", "<i4"),
                       ("p2", "<i4", (2,)), ("p3", "<i4", (2,)), ("n", "<i4"), ("pad", "<i4", (3,))])     # the device record, 16 int32
TEXT_DTYPE = np.dtype([("origin", "<i4", (2,)), ("chars", "u1", (TEXT_LEN,))])      # (x, y) of the row's baseline-left
# the panel record lav_log_view reads (16 int32): the host's with the palette and the source resolved
DEVICE_PANEL_DTYPE = np.dtype([("kind", "<i4"), ("rect", "<i4", (4,)), ("channels", "<i4"), ("colour", "u1", (4,)), ("pal_off", "<i4"),
                               ("pal_n", "<i4"), ("label_bytes", "<i4"), ("source", "<u8"), ("pad", "<i4", (4,))])
assert PRIM_DTYPE.itemsize == 64 and DEVICE_PANEL_DTYPE.itemsize == 64

# lav/utils/visualization.py: SEM_COLORS (pinned by tests/golden/log_view.npz)
SEM_COLORS = {4: (220, 20, 60), 5: (153, 153, 153), 6: (157, 234, 50), 7: (128, 64, 128), 8: (244, 35, 232), 10: (0, 0, 142), 18: (220, 220, 0)}
DEFAULT_LABELS = (4, 6, 7, 10, 18)
BRA_LABELS = (4, 10, 18)
# lav/utils/logger.py: Tango colours
ORANGE, RED, BLUE, GREEN, BLACK = (252, 175, 62), (204, 0, 0), (52, 101, 164), (115, 210, 22), (0, 0, 0)
ARROW_WIDTH = 10
TEXT_STRIP = 12                     # rows above the lidar frame's panels for the command name
BAR_PANEL_W, BAR_W, BAR_GROUND = 64, 16, (46, 52, 54)

Frame = namedtuple("Frame", "panels prims text sources size")


# ---------------------------------------------------------------------------------------------- tables
def palette_of(labels) -> np.ndarray:
    """(n, 3) uint8: entry i is the colour of label value i + 1."""
    try:
        return np.array([SEM_COLORS[int(l)] for l in labels], np.uint8).reshape(-1, 3)
    except KeyError as e:
        raise ValueError(f"log view: label {e} has no colour in SEM_COLORS") from None


def panel_table(rows) -> np.ndarray:
    """rows of dict(kind, x, y, w, h[, source][, colour][, labels]) -> PANEL_DTYPE."""
    out = np.zeros(len(rows), PANEL_DTYPE)
    for o, r in zip(out, rows):
        labels = list(r.get("labels", ()))
        if len(labels) > MAX_LABELS:
            raise ValueError(f"log view: {len(labels)} labels (at most {MAX_LABELS})")
        o["kind"], o["rect"], o["source"] = r["kind"], (r["x"], r["y"], r["w"], r["h"]), r.get("source", -1)
        o["colour"][:3] = r.get("colour", (0, 0, 0))
        o["nlabels"] = len(labels)
        o["labels"][:len(labels)] = labels
    return out


def text_table(rows) -> np.ndarray:
    """rows of (x, y, string) -> TEXT_DTYPE (7-bit ASCII, zero padded, cut at TEXT_LEN)."""
    out = np.zeros(len(rows), TEXT_DTYPE)
    for o, (x, y, s) in zip(out, rows):
        b = np.frombuffer(str(s).encode("ascii", "replace")[:TEXT_LEN], np.uint8)
        o["origin"] = (x, y)
        o["chars"][:len(b)] = b
    return out


def _shape(src):
    return tuple(int(v) for v in src.shape)


def _dtype_name(src) -> str:
    return str(src.dtype).replace("torch.", "")


def check_panels(panels, sources) -> np.ndarray:
    """The panel table against its sources' shapes and dtypes (NumPy arrays or torch tensors)."""
    panels = np.ascontiguousarray(panels)
    if panels.dtype != PANEL_DTYPE or panels.ndim != 1 or len(panels) > MAX_PANELS:
        raise ValueError(f"log view: panels must be at most {MAX_PANELS} rows of PANEL_DTYPE, got {panels.dtype} {panels.shape}")
    for i, p in enumerate(panels):
        kind, (x, y, w, h) = int(p["kind"]), (int(v) for v in p["rect"])
        if kind not in (IMAGE_U8, LABELS, LOGITS, PLANES, SOLID):
            raise ValueError(f"log view: panel {i} of unknown kind {kind}")
        if min(x, y, w, h) < 0 or max(x + w, y + h) > MAX_SIDE:
            raise ValueError(f"log view: panel {i} rectangle {(x, y, w, h)}")
        if not 0 <= int(p["nlabels"]) <= MAX_LABELS:
            raise ValueError(f"log view: panel {i} with {int(p['nlabels'])} labels")
        palette_of(p["labels"][:int(p["nlabels"])])
        if kind == SOLID:
            continue
        if not 0 <= int(p["source"]) < len(sources):
            raise ValueError(f"log view: panel {i} names source {int(p['source'])} of {len(sources)}")
        src = sources[int(p["source"])]
        shape, dt = _shape(src), _dtype_name(src)
        want = {IMAGE_U8: (shape == (h, w, 3) and dt == "uint8"), LABELS: (shape == (h, w) and dt in ("uint8", "int32", "int64")),
                LOGITS: (len(shape) == 3 and shape[1:] == (h, w) and 1 <= shape[0] <= 4096 and dt == "float32"),
                PLANES: (len(shape) == 3 and shape[1:] == (h, w) and 1 <= shape[0] <= 4096 and dt == "float32")}[kind]
        if not want:
            raise ValueError(f"log view: panel {i} (kind {kind}, {h} x {w}) cannot show a source of {dt} {shape}")
    return panels


def check_prims(prims, npanels: int) -> np.ndarray:
    prims = np.ascontiguousarray(prims)
    if prims.dtype != PRIM_DTYPE or prims.ndim != 1 or len(prims) > MAX_PRIMS:
        raise ValueError(f"log view: primitives must be at most {MAX_PRIMS} rows of PRIM_DTYPE, got {prims.dtype} {prims.shape}")
    if len(prims):
        if not np.isin(prims["kind"], (DOT, SEGMENT, CONVEX)).all():
            raise ValueError("log view: unknown primitive kind")
        if max(np.abs(prims[k]).max() for k in ("p0", "p1", "p2", "p3")) > COORD_LIMIT or prims["radius"].min() < 0 or prims["radius"].max() > 1024:
            raise ValueError("log view: primitive coordinates beyond +-2^20 or a radius outside [0, 1024]")
        if prims["panel"].min() < 0 or prims["panel"].max() >= npanels:
            raise ValueError(f"log view: a primitive names a panel outside the {npanels} of the frame")
        cv = prims[prims["kind"] == CONVEX]
        if not np.isin(cv["n"], (3, 4)).all() or (cv["p3"][cv["n"] == 3] != cv["p2"][cv["n"] == 3]).any():
            raise ValueError("log view: a polygon has 3 or 4 vertices, and a triangle repeats its last")
    return prims


def check_text(text) -> np.ndarray:
    text = np.ascontiguousarray(text)
    if text.dtype != TEXT_DTYPE or text.ndim != 1 or len(text) > MAX_ROWS or (len(text) and text["chars"].max() > 127):
        raise ValueError(f"log view: text must be at most {MAX_ROWS} rows of TEXT_DTYPE holding 7-bit characters")
    if len(text) and np.abs(text["origin"]).max() > COORD_LIMIT:
        raise ValueError("log view: a text origin beyond +-2^20")
    return text


def frame_size(panels, size=None):
    """(height, width): `size`, or the extent of the panels."""
    if size is None:
        size = (max((int(p["rect"][1] + p["rect"][3]) for p in panels), default=0), max((int(p["rect"][0] + p["rect"][2]) for p in panels), default=0))
    h, w = int(size[0]), int(size[1])
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"log view: frame of {h} x {w}")
    return h, w


def device_tables(panels, sources, pointers):
    """(DEVICE_PANEL_DTYPE table, (n, 3) uint8 palette) of checked panels; pointers[i] is the address of sources[i]."""
    out = np.zeros(len(panels), DEVICE_PANEL_DTYPE)
    pal = []
    for o, p in zip(out, panels):
        o["kind"], o["rect"], o["colour"] = p["kind"], p["rect"], p["colour"]
        o["pal_off"], o["pal_n"] = sum(len(a) for a in pal), p["nlabels"]
        pal.append(palette_of(p["labels"][:int(p["nlabels"])]))
        if int(p["kind"]) != SOLID:
            src = sources[int(p["source"])]
            o["source"] = pointers[int(p["source"])]
            o["channels"] = _shape(src)[0] if int(p["kind"]) in (LOGITS, PLANES) else 0
            o["label_bytes"] = {"uint8": 1, "int32": 4, "int64": 8}.get(_dtype_name(src), 0)
    return out, np.concatenate(pal + [np.zeros((0, 3), np.uint8)]).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- specification
def covers_convex(prim, xs, ys) -> np.ndarray:
    """Whether the filled convex polygon covers the pixel centres (xs, ys), in int64: inside the box of its vertices, every edge
    function (b - a) x (c - a) is >= 0 or every one is <= 0 - edges inclusive; a zero-area polygon covers only its edges."""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    v = np.array([prim["p0"], prim["p1"], prim["p2"], prim["p3"]], np.int64)
    pos = neg = (xs >= v[:, 0].min()) & (xs <= v[:, 0].max()) & (ys >= v[:, 1].min()) & (ys <= v[:, 1].max())
    for a, b in zip(v, np.roll(v, -1, axis=0)):
        e = (b[0] - a[0]) * (ys - a[1]) - (b[1] - a[1]) * (xs - a[0])
        pos, neg = pos & (e >= 0), neg & (e <= 0)
    return pos | neg


def prim_box(prim):
    """(x0, y0, x1, y1) of the primitive in its panel's coordinates, inclusive."""
    if int(prim["kind"]) == CONVEX:
        v = np.array([prim["p0"], prim["p1"], prim["p2"], prim["p3"]], np.int64)
        return int(v[:, 0].min()), int(v[:, 1].min()), int(v[:, 0].max()), int(v[:, 1].max())
    r = int(prim["radius"])
    xs, ys = (int(prim["p0"][0]), int(prim["p1"][0])), (int(prim["p0"][1]), int(prim["p1"][1]))
    return min(xs) - r, min(ys) - r, max(xs) + r, max(ys) + r


def prim_covers(prim, xs, ys) -> np.ndarray:
    return covers_convex(prim, xs, ys) if int(prim["kind"]) == CONVEX else covers(prim, xs, ys)


def planes_grey(src) -> np.ndarray:
    """(C, h, w) float32 -> (h, w) uint8: imshow(mean(axis=0), cmap='gray') as the module's docstring restates it."""
    src = np.asarray(src)
    acc = np.zeros(src.shape[1:], np.float64)
    for plane in src:
        acc = acc + plane.astype(np.float64)
    m = acc / np.float64(src.shape[0])
    fin = np.isfinite(m)
    out = np.zeros(m.shape, np.uint8)
    if fin.any():
        lo, hi = m[fin].min(), m[fin].max()
        if hi != lo:
            with np.errstate(invalid="ignore", over="ignore"):
                g = np.floor((m - lo) * 255.0 / (hi - lo))
            out = np.where(fin, np.clip(np.where(fin, g, 0.0), 0.0, 255.0), 0.0).astype(np.uint8)
    return out


def palette_image(labels, palette) -> np.ndarray:
    labels = np.asarray(labels).astype(np.int64)
    out = np.zeros(labels.shape + (3,), np.uint8)
    for i, colour in enumerate(palette):
        out[labels == i + 1] = colour
    return out


def _numpy(src) -> np.ndarray:
    return src.detach().cpu().numpy() if hasattr(src, "detach") else np.asarray(src)


def panel_image(panel, sources) -> np.ndarray:
    kind, (_, _, w, h) = int(panel["kind"]), (int(v) for v in panel["rect"])
    if kind == SOLID:
        return np.broadcast_to(panel["colour"][:3], (h, w, 3))
    src = _numpy(sources[int(panel["source"])])
    if kind == IMAGE_U8:
        return src
    if kind == PLANES:
        return np.repeat(planes_grey(src)[..., None], 3, axis=2)
    return palette_image(src if kind == LABELS else np.argmax(src, axis=0), palette_of(panel["labels"][:int(panel["nlabels"])]))


def log_view_numpy(panels, prims, text, sources, size=None) -> np.ndarray:
    """The frame (height, width, 3) uint8 of the three tables over `sources` (a list of arrays or tensors): what lav_log_view
    computes.  size: (height, width) of the frame; by default the extent of the panels."""
    panels = check_panels(panels, sources)
    prims, text = check_prims(prims, len(panels)), check_text(text)
    H, W = frame_size(panels, size)
    frame = np.zeros((H, W, 3), np.uint8)
    for p in panels:
        x, y, w, h = (int(v) for v in p["rect"])
        hh, ww = min(h, H - y), min(w, W - x)
        if hh > 0 and ww > 0:
            frame[y:y + hh, x:x + ww] = panel_image(p, sources)[:hh, :ww]
    for p in prims:
        x, y, w, h = (int(v) for v in panels[int(p["panel"])]["rect"])
        x0, y0, x1, y1 = prim_box(p)
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1, W - 1 - x), min(y1, h - 1, H - 1 - y)
        if x1 < x0 or y1 < y0:
            continue
        ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        frame[y + y0:y + y1 + 1, x + x0:x + x1 + 1][prim_covers(p, xs, ys)] = p["colour"][:3]
    for row in text:
        ox, oy = int(row["origin"][0]), int(row["origin"][1])
        for i, ch in enumerate(row["chars"]):
            for gy in range(GLYPH_H):
                for gx in range(GLYPH_W):
                    yy, xx = oy - (GLYPH_H - 1) + gy, ox + GLYPH_STEP * i + gx
                    if FONT[ch, gy] >> (GLYPH_W - 1 - gx) & 1 and 0 <= yy < H and 0 <= xx < W:
                        frame[yy, xx] = 255
    return frame


# ---------------------------------------------------------------------------------------------- builders
class _Prims:
    def __init__(self):
        self.rows = []

    def _row(self, kind, panel, pts, radius, colour, n=0):
        pts = [(int(p[0]), int(p[1])) for p in pts]
        pts += [pts[-1]] * (4 - len(pts))
        self.rows.append((kind, pts[0], pts[1], radius, tuple(int(c) for c in colour) + (0,), panel, pts[2], pts[3], n, (0, 0, 0)))

    def dot(self, panel, p, radius, colour):
        self._row(DOT, panel, [p, p], radius, colour)

    def segment(self, panel, a, b, colour):
        self._row(SEGMENT, panel, [a, b], 1, colour)

    def convex(self, panel, pts, colour):
        self._row(CONVEX, panel, pts, 0, colour, n=len(pts))

    def table(self) -> np.ndarray:
        if len(self.rows) > MAX_PRIMS:
            raise ValueError(f"log view: {len(self.rows)} primitives (at most {MAX_PRIMS})")
        return np.array(self.rows, dtype=PRIM_DTYPE)


def jet_colour(score):
    return BLACK if np.isnan(score) else tuple(int(c) for c in JET_U8[jet_index(score)])


def quad_corners(x, y, w, h, cos, sin) -> np.ndarray:
    """The four corners, (4, 2) float64 before truncation, of the reference's Rectangle((x, y) + [w, h] @ [[-sin, cos], [-cos, -sin]],
    2 w, 2 h, angle=rad2deg(arctan2(sin, cos) - pi / 2)): the anchor, then along the width, the far corner, along the height."""
    xy = (x, y) + np.array([w, h], np.float64) @ np.array([[-sin, cos], [-cos, -sin]], np.float64)
    a = np.deg2rad(np.rad2deg(np.arctan2(sin, cos) - np.pi / 2))
    rot = np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
    return xy + np.array([[0, 0], [2 * w, 0], [2 * w, 2 * h], [0, 2 * h]], np.float64) @ rot


def arrow_parts(x, y, dx, dy, width=ARROW_WIDTH):
    """matplotlib's Arrow(x, y, dx, dy, width) as a shaft ((2, 2): its thickness of 0.2 width is the segment's 2 pixels at width 10)
    and a head ((3, 2): from 0.8 of the length, 0.3 width to either side, to the tip); float64 before truncation."""
    p, d = np.array([x, y], np.float64), np.array([dx, dy], np.float64)
    length = np.hypot(d[0], d[1])
    n = np.array([-d[1], d[0]]) / length * (0.3 * width) if length > 0 and np.isfinite(length) else np.zeros(2)
    return np.array([p, p + 0.8 * d]), np.array([p + 0.8 * d - n, p + d, p + 0.8 * d + n])


def _boxes(prims, panel, dets):
    for colour, det in zip((ORANGE, RED), dets):
        for x, y, w, h, cos, sin in det:
            prims.convex(panel, _to_pixel(quad_corners(x, y, w, h, cos, sin)), colour)
            shaft, head = arrow_parts(x, y, ARROW_WIDTH * sin, -ARROW_WIDTH * cos)
            prims.segment(panel, *_to_pixel(shaft), BLACK)
            prims.convex(panel, _to_pixel(head), BLACK)


def _dots(prims, panel, locs, radius, colour):
    for loc in np.asarray(locs, np.float64).reshape(-1, 2):
        prims.dot(panel, _to_pixel(loc), radius, colour)


def bev_frame(info) -> Frame:
    """log_bev_info: the BEV of sample 0 with the route target, the ego casts of every command in jet by their scores, the plan."""
    _, h, w = _shape(info["bev"])
    prims = _Prims()
    prims.dot(0, _to_pixel(np.clip(np.asarray(info["nxp"], np.float64), 0, w)), 2, ORANGE)
    for score, traj in zip(np.asarray(info["ego_cast_cmds"]), np.asarray(info["ego_cast_locs"])):
        _dots(prims, 0, traj, 1, jet_colour(score))
    _dots(prims, 0, info["ego_plan_locs"], 1, ORANGE)
    return Frame(panel_table([dict(kind=PLANES, x=0, y=0, w=w, h=h, source=0)]), prims.table(),
                 text_table([(4, 10, CMD_NAMES.get(int(info["cmd"])))]), [info["bev"]], (h, w))


def lidar_frame(info) -> Frame:
    """log_lidar_info: under the command name, the ground truth (BEV, boxes with heading arrows, the ego's and the others' future
    locations, the target) beside the prediction (BEV, detected boxes, the plan, every command's cast of every detected vehicle in
    jet by its score - the reference's threshold is commented out)."""
    (_, h0, w0), (_, h1, w1) = _shape(info["bev"]), _shape(info["pred_bev"])
    prims = _Prims()
    _boxes(prims, 0, info["gt_det"])
    _dots(prims, 0, info["ego_next_locs"], 1, RED)
    prims.dot(0, _to_pixel(np.asarray(info["nxp"], np.float64)), 2, ORANGE)
    _dots(prims, 0, info["other_next_locs"], 1, RED)
    _boxes(prims, 1, info["det"])
    _dots(prims, 1, info["ego_plan_locs"], 1, GREEN)
    for scores, trajs in zip(np.asarray(info["other_cast_cmds"]), np.asarray(info["other_cast_locs"])):
        for score, traj in zip(scores, trajs):
            _dots(prims, 1, traj, 1, jet_colour(score))
    panels = panel_table([dict(kind=PLANES, x=0, y=TEXT_STRIP, w=w0, h=h0, source=0), dict(kind=PLANES, x=w0, y=TEXT_STRIP, w=w1, h=h1, source=1)])
    return Frame(panels, prims.table(), text_table([(4, 9, CMD_NAMES.get(int(info["cmd"])))]), [info["bev"], info["pred_bev"]],
                 (TEXT_STRIP + max(h0, h1), w0 + w1))


def seg_frame(info, labels) -> Frame:
    """log_seg_info: camera image | label map | predicted label map (the argmax of the logits)."""
    h, w, _ = _shape(info["rgb"])
    (hs, ws), (_, hp, wp) = _shape(info["sem"]), _shape(info["pred_sem"])
    panels = panel_table([dict(kind=IMAGE_U8, x=0, y=0, w=w, h=h, source=0), dict(kind=LABELS, x=w, y=0, w=ws, h=hs, source=1, labels=labels),
                          dict(kind=LOGITS, x=w + ws, y=0, w=wp, h=hp, source=2, labels=labels)])
    return Frame(panels, _Prims().table(), text_table([]), [info["rgb"], info["sem"], info["pred_sem"]], (max(h, hs, hp), w + ws + wp))


def bar_height(value, h: int) -> int:
    """floor(value * h) of a bar in a panel of h rows, the value cut to [0, 1] (NaN: 0)."""
    v = np.float64(value)
    return 0 if np.isnan(v) else int(np.floor(np.clip(v, 0.0, 1.0) * h))


def bra_frame(info, labels=BRA_LABELS) -> Frame:
    """log_bra_info: the two predicted label maps (at the resolution the model emits them) and the bars of predicted against true
    brake over the two images."""
    (_, h1, w1), (_, h2, w2) = _shape(info["pred_sem1"]), _shape(info["pred_sem2"])
    (H1, W1, _), (H2, W2, _) = _shape(info["rgb1"]), _shape(info["rgb2"])
    top = max(h1, h2, 3 * GLYPH_H)
    bx = w1 + w2
    rows = [dict(kind=LOGITS, x=0, y=0, w=w1, h=h1, source=0, labels=labels), dict(kind=LOGITS, x=w1, y=0, w=w2, h=h2, source=1, labels=labels),
            dict(kind=SOLID, x=bx, y=0, w=BAR_PANEL_W, h=top, colour=BAR_GROUND)]
    for k, key in enumerate(("pred_bra", "bra")):
        bh = bar_height(info[key], top)
        rows.append(dict(kind=SOLID, x=bx + 8 + k * (BAR_W + 16), y=top - bh, w=BAR_W, h=bh, colour=BLUE))
    rows += [dict(kind=IMAGE_U8, x=0, y=top, w=W1, h=H1, source=2), dict(kind=IMAGE_U8, x=W1, y=top, w=W2, h=H2, source=3)]
    text = text_table([(bx + 4, 8, "pred"), (bx + 4 + BAR_W + 16, 8, "gt")])
    return Frame(panel_table(rows), _Prims().table(), text, [info["pred_sem1"], info["pred_sem2"], info["rgb1"], info["rgb2"]],
                 (top + max(H1, H2), max(bx + BAR_PANEL_W, W1 + W2)))


def build_frame(what: str, info, cfg=None) -> Frame:
    """The frame of trainer `what` ("bev", "lidar", "seg", "bra") from the view its logged step returned."""
    if what == "bev":
        return bev_frame(info)
    if what == "lidar":
        return lidar_frame(info)
    if what == "seg":
        return seg_frame(info, list(cfg.seg_channels) if cfg is not None else DEFAULT_LABELS[:4])
    if what == "bra":
        return bra_frame(info)
    raise ValueError(f"log view: no frame for {what!r}")


def render(frame: Frame, out=None):
    """The frame's pixels: composed on the device (a uint8 tensor in HBM, lav_log_view) when its sources are there, else by the
    specification (a NumPy array)."""
    if any(getattr(s, "is_cuda", False) for s in frame.sources):
        from .. import ops
        return ops.log_view(frame.panels, frame.prims, frame.text, frame.sources, size=frame.size, out=out)
    return log_view_numpy(frame.panels, frame.prims, frame.text, frame.sources, size=frame.size)


# ---------------------------------------------------------------------------------------------- PNG
def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def encode_png(frame: np.ndarray) -> bytes:
    """(h, w, 3) uint8 RGB -> PNG bytes: 8-bit truecolour, filter 0 on every row, one IDAT."""
    frame = np.ascontiguousarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or frame.shape[0] < 1 or frame.shape[1] < 1:
        raise ValueError(f"log view: a PNG frame is (height, width, 3) uint8, got {frame.dtype} {frame.shape}")
    h, w = frame.shape[:2]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), frame.reshape(h, w * 3)], axis=1)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6))
            + _chunk(b"IEND", b""))


class FrameWriter:
    """The logged frames of a run as `directory`/{what}_{step:07d}.png.  A frame composed on the device is copied without blocking
    into a pinned ring of two slots; it is encoded and written when the next one arrives and by close(), so the step that logs
    never waits for its own picture.  A NumPy frame (the CPU path) is written the same way, one step late."""

    def __init__(self, directory: str, what: str, slots: int = 2):
        self.directory, self.what, self.slots = directory, what, max(int(slots), 2)
        self.ring = self.events = None
        self.pending = None              # (step, slot or the NumPy frame)
        self.at = 0
        self.written = []

    def add(self, frame, step: int):
        held = frame if isinstance(frame, np.ndarray) else None
        if held is None and not frame.is_cuda:
            held = frame.numpy().copy()
        if held is None:
            import torch
            if self.ring is None or tuple(self.ring.shape[1:]) != tuple(frame.shape):
                self.flush()
                self.ring = torch.empty((self.slots, *frame.shape), dtype=torch.uint8).pin_memory()
                self.events = [torch.cuda.Event() for _ in range(self.slots)]
            self.at = (self.at + 1) % self.slots          # never the slot the pending frame sits in
            self.ring[self.at].copy_(frame, non_blocking=True)
            self.events[self.at].record()
            held = self.at
        self.flush()
        self.pending = (int(step), held)

    def flush(self):
        if self.pending is None:
            return None
        step, held = self.pending
        self.pending = None
        if isinstance(held, int):
            self.events[held].synchronize()
            held = self.ring[held].numpy()
        os.makedirs(self.directory, exist_ok=True)
        path = os.path.join(self.directory, f"{self.what}_{step:07d}.png")
        with open(path, "wb") as f:
            f.write(encode_png(held))
        self.written.append(path)
        return path

    close = flush
