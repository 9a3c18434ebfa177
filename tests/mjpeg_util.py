"""Shared by tests/test_mjpeg_host.py and tests/test_gpu_mjpeg.py: the sizes, the content cases and a marker walker.

SIZES are the smallest shapes at which each part of the stream can go wrong: one MCU; both sides padded (17 x 33: 2 x 3 MCUs); nine
MCUs in intervals of four, so that intervals cross MCU rows and the last one is partial; ten intervals of one MCU, so that the RST
index wraps; and the agent's 160 x 1146 frame (72 intervals of 10 MCUs, the width padded by 6 columns)."""
import functools
import struct

import numpy as np

from lav_amd.agent import debug_view as V
from lav_amd.agent import mjpeg as M
from tests.debug_view_util import AGENT_GRID, CMD_THRESH, cloud, controls, images, pred_bev, scene

SIZES = [(16, 16, 10), (17, 33, 10), (48, 48, 4), (16, 160, 1), (160, 1146, M.DEFAULT_RESTART_MCUS)]
QUALITIES = [25, 50, 90, 100]
# content case -> (quality, restart_mcus); case_frame(name) makes the frame
CASES = {"noise": (100, 4), "dots": (50, 10), "flat": (90, 1), "mcus": (100, 4), "checker": (100, 10), "gradient": (90, 10),
         "debug": (90, M.DEFAULT_RESTART_MCUS)}


def gradient(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(255 * x) // max(w - 1, 1), (255 * y) // max(h - 1, 1), (255 * (x + y)) // max(w + h - 2, 1)], -1).astype(np.uint8)


def lowpass_noise(h, w, seed=0):
    """Uniform noise averaged over 5 x 5 windows and stretched back to the full range."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 1, (h + 4, w + 4, 3))
    s = sum(a[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5))
    s = (s - s.min()) / (s.max() - s.min())
    return np.round(s * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _debug_frame():
    rgb, tel = images((288, 768, 3), (192, 480, 3), seed=5)
    pts = cloud(AGENT_GRID, n=20000, seed=6)
    plan, locs, cmds, det, tgt = scene("full", AGENT_GRID, (160, 280), 8)
    # cameras with structure (the noise images of debug_view_util would make the frame incompressible): a smooth scene under mild noise
    rng = np.random.default_rng(9)
    rgb = np.clip(gradient(*rgb.shape[:2]).astype(np.int64) + rng.integers(-6, 7, rgb.shape), 0, 255).astype(np.uint8)
    tel = np.clip(gradient(*tel.shape[:2])[..., ::-1].astype(np.int64) + rng.integers(-6, 7, tel.shape), 0, 255).astype(np.uint8)
    frame = V.debug_view_numpy(rgb, tel, pts, 0.25, pred_bev(AGENT_GRID, seed=7), plan, locs, cmds, det, tgt, *controls(8)[:5], grid=AGENT_GRID,
                               cmd_thresh=CMD_THRESH)
    assert frame.shape == (160, 1146, 3)
    frame.setflags(write=False)
    return frame


def debug_frame():
    """A rendered debug frame at the agent's geometry (lav_amd.agent.debug_view.debug_view_numpy), made once."""
    return _debug_frame()


@functools.lru_cache(maxsize=None)
def case_frame(name):
    rng = np.random.default_rng(11)
    if name == "noise":                 # uniform noise at quality 100: 0xFF bytes in the entropy-coded data
        f = rng.integers(0, 256, (48, 48, 3), dtype=np.uint8)
    elif name == "dots":                # black with sparse single-pixel dots at quality 50: runs of 16 and more zeros before a coefficient
        f = np.zeros((17, 33, 3), np.uint8)
        for y, x in ((3, 5), (6, 14), (12, 2), (9, 27), (16, 32), (1, 20)):
            f[y, x] = 200          # (at 255 every run of zeros stays below 16 at these quantisers; at 200 two do not)
    elif name == "flat":                # one colour: EOB only, every DC difference but an interval's first is zero
        f = np.empty((16, 160, 3), np.uint8)
        f[:] = (200, 30, 90)
    elif name == "mcus":                # black and white MCUs in turn at quality 100: the largest DC difference
        f = np.zeros((48, 48, 3), np.uint8)
        for my in range(3):
            for mx in range(3):
                f[16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = 255 * ((my * 3 + mx) % 2)
    elif name == "checker":             # every other pixel black / white at quality 100: the largest AC magnitude
        y, x = np.mgrid[0:16, 0:16]
        f = np.repeat((255 * ((x + y) % 2))[..., None], 3, axis=2).astype(np.uint8)
    elif name == "gradient":
        f = gradient(17, 33)
    elif name == "debug":
        return debug_frame()
    else:
        raise KeyError(name)
    f.setflags(write=False)
    return f


def walk_markers(stream: bytes):
    """([(marker, payload), ...], scan): the segments of a JPEG stream in order (SOI and EOI with empty payloads) and the
    entropy-coded data between SOS and EOI, found with nothing but struct."""
    assert stream[:2] == b"\xff\xd8" and stream[-2:] == b"\xff\xd9"
    segs, pos = [(0xD8, b"")], 2
    while True:
        assert stream[pos] == 0xFF, pos
        marker = stream[pos + 1]
        n = struct.unpack_from(">H", stream, pos + 2)[0]
        segs.append((marker, stream[pos + 4:pos + 2 + n]))
        pos += 2 + n
        if marker == 0xDA:
            break
    scan = stream[pos:-2]
    segs.append((0xD9, b""))
    return segs, scan
