"""The agent's per-tick debug frame (team_code_v2/lav_agent_fast.py:459-518, 567-581) as a NumPy specification, and the recorder
that keeps the frames of a drive.

debug_view_numpy is the specification: the three cameras and the telephoto image resized to the LiDAR panel's height, the LiDAR
bird's-eye histogram (the reference's lidar_to_bev, exactly) with the ego plan, the other vehicles' forecasts coloured by command
score, the detected boxes and the route target drawn on it, the predicted BEV, all side by side, halved, with four lines of text.
lav_debug_view (csrc/debug_view.hip, ops.debug_view) renders the same frame on the device from what the frame pipeline left in
HBM, bit for bit (tests/test_gpu_debug_view.py); both draw from the same host-computed records: primitives() (integer pixel
coordinates by the reference's own expressions and dtypes), text_rows() and image.resize_linear_table().

Pinned against the reference: the LiDAR panel (tests/golden/debug_view.npz, written by the reference's lidar_to_bev) and the jet
colours (matplotlib).  UNPINNED, because OpenCV is not available here: (1) the rasterisers - a dot covers dx^2 + dy^2 <= r^2, a
thickness-2 segment the pixels whose centre lies within distance 1 of it; integer-exact rules of this project, not cv2.circle's
and cv2.drawContours' pixel sets; (2) the two resizes - image.resize_linear_u8, OpenCV's fixed-point path restated from memory;
(3) the text - FONT, a 5 x 7 bitmap font of this project, not cv2.putText's Hershey strokes.
"""
from __future__ import annotations

import os

import numpy as np

from ..data.image import resize_linear_table, resize_linear_u8

HIST_MAX = 10
# count -> grey, the reference's own expression (float64, truncated): the kernel's 11-entry table
HIST_LUT = np.array([np.float64(c) / HIST_MAX * 255. for c in range(HIST_MAX + 1)]).astype(np.uint8)
COORD_LIMIT = 1 << 20           # pixel coordinates of the records are clamped to +-2^20: a wild detection cannot overflow
DOT, SEGMENT = 0, 1
PRIM_DTYPE = np.dtype([("kind", "<i4"), ("p0", "<i4", (2,)), ("p1", "<i4", (2,)), ("radius", "<i4"), ("colour", "u1", (4,)), ("pad", "<i4")])
MAX_PRIMS = 1 << 16
TEXT_LEN = 64
TEXT_ORIGINS = ((4, 10), (4, 20), (4, 30), (4, 40))      # (x, y) of each line's baseline-left, as the reference's putText calls
GLYPH_W, GLYPH_H, GLYPH_STEP = 5, 7, 6
CMD_NAMES = {0: "left", 1: "right", 2: "straight", 3: "follow", 4: "change left", 5: "change right"}

# ---------------------------------------------------------------------------------------------- font
# 5 x 7 glyphs, one byte per row (bit 4 = leftmost pixel).  Letters have one shape for both cases.
_GLYPHS = {
    "a": "0E11111F111111", "b": "1E11111E11111E", "c": "0E11101010110E", "d": "1E11111111111E", "e": "1F10101E10101F",
    "f": "1F10101E101010", "g": "0E11101711110F", "h": "1111111F111111", "i": "0E04040404040E", "j": "0702020202120C",
    "k": "11121418141211", "l": "1010101010101F", "m": "111B1515111111", "n": "11111915131111", "o": "0E11111111110E",
    "p": "1E11111E101010", "q": "0E11111115120D", "r": "1E11111E141211", "s": "0F10100E01011E", "t": "1F040404040404",
    "u": "1111111111110E", "v": "11111111110A04", "w": "1111111515150A", "x": "11110A040A1111", "y": "1111110A040404",
    "z": "1F01020408101F", "0": "0E11131519110E", "1": "040C040404040E", "2": "0E11010204081F", "3": "1F02040201110E",
    "4": "02060A121F0202", "5": "1F101E0101110E", "6": "0608101E11110E", "7": "1F010204080808", "8": "0E11110E11110E",
    "9": "0E11110F01020C", ":": "000C0C000C0C00", ".": "00000000000C0C", "/": "00010204081000", "-": "0000001F000000",
    "+": "0004041F040400", "_": "0000000000001F", " ": "00000000000000",
}


def _font() -> np.ndarray:
    f = np.zeros((128, GLYPH_H), np.uint8)
    for ch, rows in _GLYPHS.items():
        f[ord(ch)] = np.frombuffer(bytes.fromhex(rows), np.uint8)
        if ch.isalpha():
            f[ord(ch.upper())] = f[ord(ch)]
    return f


FONT = _font()


# ---------------------------------------------------------------------------------------------- jet
_JET = dict(red=((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
            green=((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
            blue=((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)))


def _jet_u8(n: int = 256) -> np.ndarray:
    """int(c * 255) of matplotlib's n-entry jet table, from jet's piecewise-linear segments the way LinearSegmentedColormap
    builds its lookup table."""
    out = np.zeros((n, 3), np.uint8)
    for k, name in enumerate(("red", "green", "blue")):
        a = np.array(_JET[name], np.float64)
        x, y0, y1 = a[:, 0] * (n - 1), a[:, 1], a[:, 2]
        xind = (n - 1) * np.linspace(0, 1, n)
        ind = np.searchsorted(x, xind)[1:-1]
        dist = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut = np.concatenate([[y1[0]], dist * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
        out[:, k] = (np.clip(lut, 0.0, 1.0) * 255).astype(np.int64)
    return out


JET_U8 = _jet_u8()


def jet_index(score) -> int:
    """The table entry cmap(score) reads for a float32 scalar: the score times 256 in float32, truncated, cut to the table."""
    v = np.float32(score) * np.float32(256)
    if not np.isfinite(v):
        return 255 if v > 0 else 0
    return int(min(max(int(v), 0), 255))


# ---------------------------------------------------------------------------------------------- geometry
def grid_bins(grid):
    """(min_x, max_x, min_y, max_y, pixels_per_meter) -> ((x start, x stop, x bins), (y start, y stop, y bins)): the arguments
    of lidar_to_bev's two np.linspace calls (the `+ 1` on the upper edge is the reference's)."""
    min_x, max_x, min_y, max_y, ppm = grid
    nx, ny = (max_x - min_x) * ppm, (max_y - min_y) * ppm
    if nx != int(nx) or ny != int(ny) or nx < 1 or ny < 1:
        raise ValueError(f"debug view: grid {tuple(grid)} has no whole, positive number of bins")
    return (float(min_x), float(max_x + 1), int(nx)), (float(min_y), float(max_y + 1), int(ny))


def layout(rgb_shape, tel_shape, grid, bev_shape) -> dict:
    """Panel widths and offsets of the full-size canvas and the size of the frame."""
    (_, _, nxb), (_, _, nyb) = grid_bins(grid)
    H = nxb
    if len(bev_shape) != 3 or bev_shape[0] != 3 or bev_shape[1] != H:
        raise ValueError(f"debug view: pred_bev {tuple(bev_shape)} is not (3, {H}, width)")
    for name, s in (("rgb", rgb_shape), ("tel_rgb", tel_shape)):
        if len(s) != 3 or s[2] != 3 or s[0] < 1 or s[1] < 1:
            raise ValueError(f"debug view: {name} {tuple(s)} is not (height, width, 3)")
    w1 = int(rgb_shape[1] / rgb_shape[0] * H)
    w2 = int(tel_shape[1] / tel_shape[0] * H)
    if w1 < 1 or w2 < 1:
        raise ValueError("debug view: a camera panel would be empty")
    W = w1 + w2 + nyb + int(bev_shape[2])
    out = dict(H=H, w_rgb=w1, w_tel=w2, w_lidar=nyb, w_bev=int(bev_shape[2]), W=W, x_tel=w1, x_lidar=w1 + w2, x_bev=w1 + w2 + nyb,
               frame_h=int(H / 2), frame_w=int(W / 2))
    if out["frame_h"] < 1 or out["frame_w"] < 1:
        raise ValueError("debug view: empty frame")
    return out


def resize_tables(rgb_shape, tel_shape, lay) -> np.ndarray:
    """The six axis tables of the two resizes, concatenated as (n, 4) int32 in the order the kernel expects: camera columns,
    telephoto columns, camera rows, telephoto rows, frame columns, frame rows."""
    return np.ascontiguousarray(np.concatenate([
        resize_linear_table(rgb_shape[1], lay["w_rgb"]), resize_linear_table(tel_shape[1], lay["w_tel"]),
        resize_linear_table(rgb_shape[0], lay["H"]), resize_linear_table(tel_shape[0], lay["H"]),
        resize_linear_table(lay["W"], lay["frame_w"]), resize_linear_table(lay["H"], lay["frame_h"])]), dtype=np.int32)


# ---------------------------------------------------------------------------------------------- LiDAR panel
def lidar_counts(lidar, grid) -> np.ndarray:
    """np.histogramdd of the cloud's (x, y) over lidar_to_bev's edges, as integers: [x bin][y bin].  Rows with a non-finite x or
    y are skipped (the graphed pipeline marks absent points NaN; histogramdd would drop them as outliers too)."""
    (x0, x1, nxb), (y0, y1, nyb) = grid_bins(grid)
    xy = np.asarray(lidar)[..., :2].reshape(-1, 2)
    xy = xy[np.isfinite(xy).all(axis=1)]
    hist = np.histogramdd(xy, bins=(np.linspace(x0, x1, nxb + 1), np.linspace(y0, y1, nyb + 1)))[0]
    return hist.astype(np.int64)


def lidar_panel(lidar, grid) -> np.ndarray:
    """lidar_to_bev(...).astype(uint8) -> (x bins, y bins) grey."""
    hist = lidar_counts(lidar, grid).astype(np.float64)
    hist[hist > HIST_MAX] = HIST_MAX
    return (hist / HIST_MAX * 255.)[::-1, :].astype(np.uint8)


# ---------------------------------------------------------------------------------------------- primitives
def _to_pixel(v) -> np.ndarray:
    """.astype(int) of the reference, with the undefined conversions pinned: NaN -> 0, the rest cut to +-COORD_LIMIT."""
    v = np.nan_to_num(np.asarray(v, np.float64), nan=0.0, posinf=COORD_LIMIT, neginf=-COORD_LIMIT)
    return np.clip(v, -COORD_LIMIT, COORD_LIMIT).astype(np.int64)


def primitives(pred_loc, cast_locs, cast_cmds, det, tgt, *, ppm, cmd_thresh, ego=(160, 280)) -> np.ndarray:
    """The drawing list of the LiDAR panel in drawing order (later records overwrite earlier ones), PRIM_DTYPE: ego plan dots,
    forecast dots of every vehicle and every command scored >= cmd_thresh in jet colour, the vehicle boxes of det[1] as four
    thickness-2 segments each, the target dot.  Pixel coordinates by the reference's expressions and dtypes: float32 location
    times the int pixels_per_meter, plus the int64 ego, in float64, truncated toward zero."""
    ego = [int(ego[0]), int(ego[1])]
    rows = []

    def dot(p, r, colour):
        rows.append((DOT, (int(p[0]), int(p[1])), (int(p[0]), int(p[1])), r, tuple(colour) + (0,), 0))

    def at(loc):
        return _to_pixel(ego + loc * ppm)

    for loc in np.asarray(pred_loc):
        dot(at(loc), 1, (255, 0, 0))
    for trajs, cmds in zip(np.asarray(cast_locs), np.asarray(cast_cmds)):
        for traj, score in zip(trajs, cmds):
            if score < cmd_thresh:
                continue
            colour = (0, 0, 0) if np.isnan(score) else tuple(int(c) for c in JET_U8[jet_index(score)])
            for loc in traj:
                dot(at(loc), 1, colour)
    for x, y, ww, hh, cos, sin in det[1]:
        R = np.array([[-sin, cos], [-cos, -sin]])
        p = [_to_pixel([x, y] + [sx * ww, sy * hh] @ R) for sx, sy in ((-1, -1), (-1, 1), (1, 1), (1, -1))]
        for a, b in zip(p, p[1:] + p[:1]):
            rows.append((SEGMENT, (int(a[0]), int(a[1])), (int(b[0]), int(b[1])), 1, (255, 0, 0, 0), 0))
    dot(_to_pixel(np.clip(ego + np.array(tgt) * ppm, 0, 255)), 2, (0, 255, 0))
    if len(rows) > MAX_PRIMS:
        raise ValueError(f"debug view: {len(rows)} primitives (at most {MAX_PRIMS})")
    return np.array(rows, dtype=PRIM_DTYPE)


def check_primitives(prims) -> np.ndarray:
    prims = np.ascontiguousarray(prims)
    if prims.dtype != PRIM_DTYPE or prims.ndim != 1:
        raise ValueError(f"debug view: primitives must be a 1-d array of PRIM_DTYPE, got {prims.dtype} {prims.shape}")
    if len(prims) > MAX_PRIMS:
        raise ValueError(f"debug view: {len(prims)} primitives (at most {MAX_PRIMS})")
    if len(prims):
        if not np.isin(prims["kind"], (DOT, SEGMENT)).all():
            raise ValueError("debug view: unknown primitive kind")
        if np.abs(prims["p0"]).max() > COORD_LIMIT or np.abs(prims["p1"]).max() > COORD_LIMIT or prims["radius"].min() < 0 or prims["radius"].max() > 1024:
            raise ValueError("debug view: primitive coordinates beyond +-2^20 or a radius outside [0, 1024]")
    return prims


def covers(prim, xs, ys) -> np.ndarray:
    """Whether the primitive covers the pixels (xs, ys), in int64.  A dot: dx^2 + dy^2 <= r^2.  A segment p -> q of thickness 2:
    the squared distance from the pixel centre to the segment is <= 1 - with d = q - p, v = c - p, t = v . d the endpoint test
    where t <= 0 or t >= d . d, else (v x d)^2 <= d . d.  (|v x d| >= 2^22 cannot pass: d . d <= 2^43; the square is not taken
    then, it would leave int64.)"""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    px, py = int(prim["p0"][0]), int(prim["p0"][1])
    vx, vy = xs - px, ys - py
    if int(prim["kind"]) == DOT:
        r = int(prim["radius"])
        return vx * vx + vy * vy <= r * r
    qx, qy = int(prim["p1"][0]), int(prim["p1"][1])
    dx, dy = qx - px, qy - py
    dd = dx * dx + dy * dy
    t = vx * dx + vy * dy
    ux, uy = xs - qx, ys - qy
    cross = vx * dy - vy * dx
    small = np.abs(cross) < (1 << 22)
    inside = small & (np.where(small, cross, 0) ** 2 <= dd)
    return np.where(t <= 0, vx * vx + vy * vy <= 1, np.where(t >= dd, ux * ux + uy * uy <= 1, inside))


def draw(panel: np.ndarray, prims) -> np.ndarray:
    """Draw the records onto the (H, W, 3) panel in place, in order, clipped to it."""
    h, w = panel.shape[:2]
    for p in check_primitives(prims):
        r = int(p["radius"])
        x0 = max(min(int(p["p0"][0]), int(p["p1"][0])) - r, 0)
        x1 = min(max(int(p["p0"][0]), int(p["p1"][0])) + r, w - 1)
        y0 = max(min(int(p["p0"][1]), int(p["p1"][1])) - r, 0)
        y1 = min(max(int(p["p0"][1]), int(p["p1"][1])) + r, h - 1)
        if x1 < x0 or y1 < y0:
            continue
        ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        panel[y0:y1 + 1, x0:x1 + 1][covers(p, xs, ys)] = p["colour"][:3]
    return panel


# ---------------------------------------------------------------------------------------------- text
def text_rows(cmd, spd, steer, throt, brake, pred_bra) -> np.ndarray:
    """The four lines of the frame, formatted as the reference formats them, as (4, TEXT_LEN) uint8 rows (7-bit ASCII, zero
    padded, cut at TEXT_LEN)."""
    lines = (f"speed: {spd:.3f}m/s", f"steer: {steer:.3f} throttle: {throt:.3f} brake: {brake:.3f}",
             "cmd: {}".format(CMD_NAMES.get(cmd)), f"predicted brake: {pred_bra:.3f}")
    out = np.zeros((len(lines), TEXT_LEN), np.uint8)
    for row, s in zip(out, lines):
        b = np.frombuffer(s.encode("ascii", "replace")[:TEXT_LEN], np.uint8)
        row[:len(b)] = b
    return out


def check_text(text) -> np.ndarray:
    text = np.ascontiguousarray(text)
    if text.dtype != np.uint8 or text.shape != (len(TEXT_ORIGINS), TEXT_LEN) or text.max(initial=0) > 127:
        raise ValueError(f"debug view: text must be ({len(TEXT_ORIGINS)}, {TEXT_LEN}) uint8 of 7-bit characters")
    return text


def draw_text(frame: np.ndarray, text) -> np.ndarray:
    """White FONT glyphs, GLYPH_STEP pixels apart, the bottom row of a glyph on the line's baseline y, its left column at x."""
    h, w = frame.shape[:2]
    for (x0, y0), row in zip(TEXT_ORIGINS, check_text(text)):
        for i, ch in enumerate(row):
            for gy in range(GLYPH_H):
                for gx in range(GLYPH_W):
                    y, x = y0 - (GLYPH_H - 1) + gy, x0 + GLYPH_STEP * i + gx
                    if FONT[ch, gy] >> (GLYPH_W - 1 - gx) & 1 and 0 <= y < h and 0 <= x < w:
                        frame[y, x] = 255
    return frame


# ---------------------------------------------------------------------------------------------- the frame
def bev_panel(pred_bev) -> np.ndarray:
    pred_bev = np.asarray(pred_bev)
    if pred_bev.dtype != np.float32:
        raise ValueError(f"debug view: pred_bev must be float32, got {pred_bev.dtype}")
    return (255 * pred_bev.mean(axis=0)).astype(np.uint8)


def compose_numpy(rgb, tel_rgb, lidar, pred_bev, prims, text, *, grid) -> np.ndarray:
    """The frame from the host-computed records: what lav_debug_view computes."""
    rgb, tel_rgb, pred_bev = np.asarray(rgb), np.asarray(tel_rgb), np.asarray(pred_bev)
    lay = layout(rgb.shape, tel_rgb.shape, grid, pred_bev.shape)
    H = lay["H"]
    grey = lidar_panel(lidar, grid)
    lidar_viz = draw(np.ascontiguousarray(np.repeat(grey[..., None], 3, axis=2)), prims)
    canvas = np.concatenate([resize_linear_u8(rgb, (lay["w_rgb"], H)), resize_linear_u8(tel_rgb, (lay["w_tel"], H)), lidar_viz,
                             np.repeat(bev_panel(pred_bev)[..., None], 3, axis=2)], axis=1)
    frame = resize_linear_u8(canvas, (lay["frame_w"], lay["frame_h"]))
    return draw_text(frame, text)


def debug_view_numpy(rgb, tel_rgb, lidar, pred_bra, pred_bev, pred_loc, cast_locs, cast_cmds, det, tgt, cmd, spd, steer, throt, brake,
                     *, grid, cmd_thresh, ego=(160, 280)) -> np.ndarray:
    """LAVAgent.visualize of the reference (its argument list, its meanings): rgb (h, w, 3) the three views side by side and
    tel_rgb (h', w', 3), RGB uint8; lidar (n, >= 2) the stacked cloud; pred_bev (3, x bins, width) float32, already sigmoided;
    pred_loc (T, 2), cast_locs (N, C, T, 2), cast_cmds (N, C), det the per-class detection lists, tgt the route target in metres;
    grid = (min_x, max_x, min_y, max_y, pixels_per_meter).  Returns (H / 2, W / 2, 3) uint8."""
    prims = primitives(pred_loc, cast_locs, cast_cmds, det, tgt, ppm=grid[4], cmd_thresh=cmd_thresh, ego=ego)
    return compose_numpy(rgb, tel_rgb, lidar, pred_bev, prims, text_rows(cmd, spd, steer, throt, brake, pred_bra), grid=grid)


# ---------------------------------------------------------------------------------------------- recorder
class ViewRecorder:
    """The frames of a drive.  With capacity 0 (the view is off) it holds nothing and creates nothing.

    format "npy": a pinned host ring of `capacity` frames that device frames are copied into without blocking; flush() waits for the
    last copy, writes view_{first frame:06d}.npy of shape (n, H / 2, W / 2, 3) under `directory` and clears the ring.

    format "mjpeg": append() encodes the device frame on the current stream (ops.jpeg_encode, csrc/jpeg.hip) into one of STAGES
    worst-case slots in HBM and copies its length to the host; a later append() that finds that copy landed (the event is queried,
    never waited for) copies exactly that many bytes into the slot's pinned twin, and one after that moves them into ordinary host
    memory and frees the slot - so in steady state a frame is on the host two ticks after it was rendered, run_step waits for nothing
    and only the compressed bytes cross the bus.  Only when every slot is still in flight (the device more than STAGES - 1 frames behind)
    does append() wait, for the oldest: nothing is ever dropped or cut.  Pinned memory: STAGES x (scan capacity + 4) bytes, 7.2 MB at
    the agent's 160 x 1146 frame, whatever `capacity` is.  flush() and frames_jpeg() synchronise; flush() writes
    view_{first frame:06d}.avi (lav_amd.agent.mjpeg.AviWriter at `fps`), every frame jpeg_header + scan + EOI.  CPU tensors are
    encoded by the specification jpeg_encode_numpy: the same bytes.  frames() is the "npy" ring's and not available here."""

    STAGES = 4
    FORMATS = ("npy", "mjpeg")

    def __init__(self, directory: str = "debug_view", capacity: int = 0, format: str = "npy", quality: int = 90, fps: float = 20.0):
        if format not in self.FORMATS:
            raise ValueError(f"ViewRecorder: format {format!r} is not one of {self.FORMATS}")
        self.directory, self.capacity, self.format, self.quality, self.fps = directory, int(capacity), format, quality, float(fps)
        if format == "mjpeg":
            from . import mjpeg
            mjpeg._check(quality, mjpeg.DEFAULT_RESTART_MCUS)
            if not self.fps > 0:
                raise ValueError(f"ViewRecorder: {fps} frames per second")
        self.ring = self.event = None
        self.count = 0
        self.first_frame = 0
        self.written = []
        self.jpegs = []                # mjpeg: the scans that have reached ordinary host memory, in order
        self.shape = None              # mjpeg: (h, w) of the frames held
        self.stage = None              # mjpeg: the device slots and their pinned twins
        self.inflight = []             # mjpeg: [slot, state, event, length] in frame order; state 0: length on its way, 1: bytes on their way

    def __len__(self):
        return self.count

    def clear(self):
        if self.inflight:
            self._advance(wait=True)           # (frames still on their way must not turn up among the next ones)
        self.count = 0
        self.jpegs = []

    def full(self) -> bool:
        return self.capacity > 0 and self.count >= self.capacity

    def append(self, frame, frame_no: int):
        """Copy (npy) or encode (mjpeg) the device frame into the next slot (non-blocking, on the current stream)."""
        import torch
        if self.capacity < 1:
            raise RuntimeError("ViewRecorder: recording is off (capacity 0)")
        if self.full():
            self.flush()
        if self.format == "mjpeg":
            return self._append_jpeg(frame, frame_no)
        if self.ring is None or tuple(self.ring.shape[1:]) != tuple(frame.shape):
            if self.count:
                self.flush()
            self.ring = torch.empty((self.capacity, *frame.shape), dtype=torch.uint8).pin_memory()
            self.event = torch.cuda.Event()
        if self.count == 0:
            self.first_frame = int(frame_no)
        self.ring[self.count].copy_(frame, non_blocking=True)
        self.event.record()
        self.count += 1

    # ------------------------------------------------------------------------------------------ mjpeg
    def _append_jpeg(self, frame, frame_no: int):
        import torch

        from . import mjpeg
        if frame.dim() != 3 or frame.shape[2] != 3 or frame.dtype != torch.uint8:
            raise ValueError(f"ViewRecorder: frame must be (h, w, 3) uint8, got {frame.dtype} {tuple(frame.shape)}")
        hw = (int(frame.shape[0]), int(frame.shape[1]))
        if self.shape != hw:
            if self.count:
                self.flush()
            self.shape, self.stage = hw, None
        if self.count == 0:
            self.first_frame = int(frame_no)
        self.count += 1
        if not frame.is_cuda:
            self._advance(wait=True)           # (device frames before this one keep their place)
            self.jpegs.append(mjpeg.scan_numpy(frame.numpy(), self.quality))
            return
        from .. import ops
        if self.stage is None or self.stage[0].device != frame.device:
            self._advance(wait=True)
            cap = mjpeg.scan_capacity(*hw)
            self.stage = (torch.empty((self.STAGES, cap), dtype=torch.uint8, device=frame.device),
                          torch.empty((self.STAGES,), dtype=torch.int32, device=frame.device),
                          torch.empty((self.STAGES, cap), dtype=torch.uint8).pin_memory(), torch.empty((self.STAGES,), dtype=torch.int32).pin_memory())
            self.free = list(range(self.STAGES))
        self._advance(wait=False)
        if not self.free:
            self._advance(wait=True)           # every slot in flight: the device is STAGES frames behind
        slot = self.free.pop(0)
        dev_scans, dev_len, _, host_len = self.stage
        ops.jpeg_encode(frame, quality=self.quality, out=dev_scans[slot:slot + 1], lengths=dev_len[slot:slot + 1])
        host_len[slot:slot + 1].copy_(dev_len[slot:slot + 1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.inflight.append([slot, 0, ev, 0])

    def _advance(self, wait: bool):
        """Move the frames in flight on as far as their copies have landed (the events are queried) - or, with wait, all the way."""
        import torch
        if not self.inflight:
            return
        dev_scans, _, host_scans, host_len = self.stage
        for item in self.inflight:             # a length has landed: copy exactly that many bytes
            slot, state, ev, _ = item
            if state == 0 and (wait or ev.query()):
                ev.synchronize()
                n = int(host_len[slot])
                if not 0 < n <= host_scans.shape[1]:
                    raise RuntimeError(f"ViewRecorder: a scan of {n} bytes in a slot of {host_scans.shape[1]}")
                host_scans[slot, :n].copy_(dev_scans[slot, :n], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                item[1:] = [1, ev, n]
        while self.inflight and self.inflight[0][1] == 1 and (wait or self.inflight[0][2].query()):      # in frame order
            slot, _, ev, n = self.inflight.pop(0)
            ev.synchronize()
            self.jpegs.append(host_scans[slot, :n].numpy().tobytes())
            self.free.append(slot)

    def frames_jpeg(self) -> list:
        """The recorded frames as complete JPEG streams, once every copy has landed (mjpeg only)."""
        from . import mjpeg
        if self.format != "mjpeg":
            raise RuntimeError("ViewRecorder: frames_jpeg() is the mjpeg format's; frames() holds the npy ring")
        self._advance(wait=True)
        if self.count == 0:
            return []
        head = mjpeg.jpeg_header(*self.shape, self.quality)
        return [head + scan + mjpeg.EOI for scan in self.jpegs]

    def frames(self) -> np.ndarray:
        """The recorded frames (n, H / 2, W / 2, 3), once their copies have landed; a view of the ring, valid until the next append."""
        if self.format != "npy":
            raise RuntimeError("ViewRecorder: frames() is the npy format's; frames_jpeg() holds the mjpeg frames")
        if self.count == 0:
            return np.zeros((0, 0, 0, 3), np.uint8)
        self.event.synchronize()
        return self.ring[:self.count].numpy()

    def flush(self):
        if self.count == 0:
            return None
        if self.format == "mjpeg":
            from . import mjpeg
            jpegs = self.frames_jpeg()
            assert len(jpegs) == self.count
            os.makedirs(self.directory, exist_ok=True)
            path = os.path.join(self.directory, f"view_{self.first_frame:06d}.avi")
            with mjpeg.AviWriter(path, *self.shape, fps=self.fps) as avi:
                for j in jpegs:
                    avi.add(j)
        else:
            frames = self.frames()
            os.makedirs(self.directory, exist_ok=True)
            path = os.path.join(self.directory, f"view_{self.first_frame:06d}.npy")
            np.save(path, frames)
        self.written.append(path)
        self.clear()
        return path
