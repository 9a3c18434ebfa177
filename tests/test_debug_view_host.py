"""The debug view's specification on the CPU (lav_amd/agent/debug_view.py, lav_amd/data/image.py:resize_linear_u8): the LiDAR panel
against the reference's own lidar_to_bev (tests/golden/debug_view.npz, written by tests/golden/make_golden_view.py), the jet
colours against matplotlib, the properties of the restated resize, this project's rasterisation rules, the font, and the frame's
layout at the agent's geometry."""
import os

import numpy as np
import pytest

from lav_amd.agent import debug_view as V
from lav_amd.data.image import resize_linear_table, resize_linear_u8
from tests.debug_view_util import AGENT_GRID, CMD_THRESH, FRAMES, GEOMETRIES, SCENES, cloud, controls, images, pred_bev, scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "debug_view.npz")


# ---------------------------------------------------------------------------------------------- LiDAR panel
@pytest.mark.parametrize("name", ["a", "b"])
def test_lidar_panel_equals_the_reference_lidar_to_bev(name):
    g = np.load(GOLDEN)
    grid, pts, want = tuple(int(v) for v in g[f"{name}/grid"]), g[f"{name}/points"], g[f"{name}/panel"]
    assert len(pts) <= 4096 and want.shape[0] <= 64 and want.shape[1] <= 64 and os.path.getsize(GOLDEN) < 100 * 1024
    # the fixture holds what it is meant to: cells at 9 points, at and past the clamp, rows outside the grid and non-finite rows
    counts = V.lidar_counts(pts, grid)
    assert {9, 10, 11, 300} <= set(np.unique(counts).tolist()) and counts.sum() < np.isfinite(pts[:, :2]).all(1).sum() < len(pts)
    np.testing.assert_array_equal(V.lidar_panel(pts, grid), want)
    assert V.HIST_LUT.tolist() == [0, 25, 51, 76, 102, 127, 153, 178, 204, 229, 255]


def test_lidar_bins_follow_histogramdd_on_edges():
    grid = (-2, 8, -5, 5, 5)                                   # step 11 / 50: edges float32 does not hold
    ex, ey = np.linspace(-2, 9, 51), np.linspace(-5, 6, 51)
    c = lambda x, y: V.lidar_counts(np.array([[x, y]], np.float32), grid)          # noqa: E731
    assert c(-2.0, -5.0)[0, 0] == 1 and c(9.0, 6.0)[49, 49] == 1                    # first edge inside, last edge inclusive
    assert c(np.nextafter(np.float32(9), np.float32(10)), 0.0).sum() == 0 and c(np.nextafter(np.float32(-2), np.float32(-3)), 0.0).sum() == 0
    for i in range(1, 50):                                     # an interior edge belongs to the bin on its right - as float32 holds it
        x = np.float32(ex[i])
        assert c(x, 0.0)[i if np.float64(x) >= ex[i] else i - 1].sum() == 1
    assert c(np.nan, 0.0).sum() == 0 and c(0.0, np.inf).sum() == 0
    assert ey[-1] == 6.0


# ---------------------------------------------------------------------------------------------- jet
def test_jet_table_and_index_rule_equal_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps["jet"]
    np.testing.assert_array_equal(V.JET_U8, np.array([[int(c * 255) for c in cmap(i)[:3]] for i in range(256)], np.uint8))
    scores = np.concatenate([np.linspace(0, 1, 4097), np.arange(257) / 256, np.nextafter(np.arange(257, dtype=np.float32) / 256, np.float32(-1)),
                             [1.0, 1.5, 0.2, 0.19999]]).astype(np.float32)
    for s in scores:                                           # a float32 scalar, as the reference passes it
        r, g, b, _ = cmap(s)
        assert (int(r * 255), int(g * 255), int(b * 255)) == tuple(V.JET_U8[V.jet_index(s)]), s


# ---------------------------------------------------------------------------------------------- resize
def test_resize_properties():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    np.testing.assert_array_equal(resize_linear_u8(img, (17, 13)), img)                                   # identity at equal size
    np.testing.assert_array_equal(resize_linear_u8(img[..., 0], (17, 13)), img[..., 0])
    for v in (0, 1, 127, 254, 255):                                                                       # a constant image stays constant
        for dsize in ((5, 7), (40, 31), (17, 6), (8, 13)):
            out = resize_linear_u8(np.full((13, 17, 3), v, np.uint8), dsize)
            assert out.shape == (dsize[1], dsize[0], 3) and (out == v).all()
    blocks = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)                                               # exact 2 : 1 of 2 x 2 blocks
    np.testing.assert_array_equal(resize_linear_u8(np.repeat(np.repeat(blocks, 2, 0), 2, 1), (9, 6)), blocks)
    # enlarging: the first and the last output pixels lie outside the source's pixel centres and take the edge pixel itself
    big = resize_linear_u8(img, (51, 39))
    np.testing.assert_array_equal(big[0, 0], img[0, 0]); np.testing.assert_array_equal(big[-1, -1], img[-1, -1])
    np.testing.assert_array_equal(big[0, -1], img[0, -1]); np.testing.assert_array_equal(big[-1, 0], img[-1, 0])
    t = resize_linear_table(17, 51)
    assert t[0].tolist() == [0, 1, 2048, 0] and t[-1].tolist() == [16, 16, 2048, 0] and (t[:, 2] + t[:, 3] == 2048).all()
    assert (np.diff(t[:, 0]) >= 0).all() and t[:, :2].min() == 0 and t[:, :2].max() == 16
    # the frame's second resize is a general one: 2293 -> 1146 columns
    t = resize_linear_table(2293, 1146)
    assert (t[:, 3] != 0).any() and len(np.unique(t[:, 3])) > 100
    with pytest.raises(TypeError):
        resize_linear_u8(img.astype(np.float32), (4, 4))


# ---------------------------------------------------------------------------------------------- rasteriser
def _prims(rows):
    return np.array(rows, dtype=V.PRIM_DTYPE)


def _dot(x, y, r, colour):
    return (V.DOT, (x, y), (x, y), r, (*colour, 0), 0)


def _seg(p, q, colour):
    return (V.SEGMENT, p, q, 1, (*colour, 0), 0)


def test_dots_cover_5_and_13_pixels_and_a_segment_three_rows():
    panel = V.draw(np.zeros((20, 30, 3), np.uint8), _prims([_dot(5, 6, 1, (255, 0, 0)), _dot(20, 10, 2, (0, 255, 0))]))
    assert (panel[..., 0] == 255).sum() == 5 and (panel[..., 1] == 255).sum() == 13
    assert panel[6, 4:7, 0].tolist() == [255] * 3 and panel[5:8, 5, 0].tolist() == [255] * 3 and panel[5, 4, 0] == 0
    assert panel[10, 18:23, 1].tolist() == [255] * 5 and panel[9, 19:22, 1].tolist() == [255] * 3 and panel[9, 18, 1] == 0
    seg = V.draw(np.zeros((20, 30, 3), np.uint8), _prims([_seg((4, 10), (24, 10), (9, 9, 9))]))[..., 0] == 9
    assert seg[9, 4:25].all() and seg[10, 3:26].all() and seg[11, 4:25].all() and seg.sum() == 21 * 3 + 2      # three rows and the two caps
    diag = V.draw(np.zeros((20, 30, 3), np.uint8), _prims([_seg((2, 2), (12, 12), (9, 9, 9))]))[..., 0] == 9
    assert all(diag[i, i] and diag[i, i + 1] and diag[i + 1, i] for i in range(2, 12)) and not diag[2, 4] and not diag[1, 1]


def test_draw_order_clipping_and_degenerate_box():
    a, b = _dot(5, 5, 2, (1, 1, 1)), _seg((0, 5), (10, 5), (2, 2, 2))
    first = V.draw(np.zeros((12, 12, 3), np.uint8), _prims([a, b]))[..., 0]
    second = V.draw(np.zeros((12, 12, 3), np.uint8), _prims([b, a]))[..., 0]
    assert first[5, 5] == 2 and second[5, 5] == 1 and first[3, 5] == 1 and second[5, 0] == 2       # the later record wins where both cover
    # clipped to the panel: a dot on the corner, a segment through the edge, records wholly outside
    out = V.draw(np.zeros((12, 12, 3), np.uint8), _prims([_dot(0, 0, 2, (7, 7, 7)), _seg((8, 3), (40, 3), (8, 8, 8)), _dot(-3, 5, 2, (9, 9, 9)),
                                                         _dot(12, 12, 1, (9, 9, 9)), _seg((-30, -30), (-5, -5), (9, 9, 9)), _dot(1 << 20, -(1 << 20), 2, (9, 9, 9))]))[..., 0]
    assert (out == 7).sum() == 6 and (out == 8).sum() == 3 * 4 + 1 and (out == 9).sum() == 0
    # a box of no size is four segments of no length: the five pixels of a radius-1 dot
    prims = V.primitives(np.zeros((0, 2), np.float32), np.zeros((0, 6, 20, 2), np.float32), np.zeros((0, 6), np.float32),
                         [[], [(6.0, 7.0, 0.0, 0.0, 1.0, 0.0)]], [100.0, 100.0], ppm=4, cmd_thresh=CMD_THRESH, ego=(3, 3))
    assert len(prims) == 5 and prims["kind"].tolist() == [V.SEGMENT] * 4 + [V.DOT]
    box = V.draw(np.zeros((12, 12, 3), np.uint8), prims[:4])[..., 0]
    assert (box == 255).sum() == 5 and box[7, 6] == 255 and box[6, 6] == 255 and box[7, 5] == 255


def test_primitives_follow_the_reference_expressions():
    plan = np.array([[0.3, -1.2], [np.nan, 0.0], [1e30, -1e30]], np.float32)
    locs = np.zeros((2, 6, 20, 2), np.float32)
    cmds = np.array([[0.1, 0.2, 0.5, 0.19, 0.9, 0.0], [0.0] * 6], np.float32)
    det = [[(1.0, 1.0, 1.0, 1.0, 1.0, 0.0)], [(100.4, 200.6, 3.3, 7.7, 0.6, 0.8)]]
    prims = V.primitives(plan, locs, cmds, det, [2.5, -300.0], ppm=4, cmd_thresh=CMD_THRESH)
    assert len(prims) == 3 + 3 * 20 + 4 + 1
    ego = [160, 280]
    assert prims["p0"][0].tolist() == list((ego + plan[0] * 4).astype(int)) and prims["p0"][1].tolist() == [0, 280]
    assert prims["p0"][2].tolist() == [V.COORD_LIMIT, -V.COORD_LIMIT]
    assert prims["colour"][3, :3].tolist() == V.JET_U8[V.jet_index(np.float32(0.2))].tolist() and prims["colour"][23, :3].tolist() == V.JET_U8[128].tolist()
    R = np.array([[-0.8, 0.6], [-0.6, -0.8]])
    corners = [tuple(([100.4, 200.6] + [sx * 3.3, sy * 7.7] @ R).astype(int)) for sx, sy in ((-1, -1), (-1, 1), (1, 1), (1, -1))]
    assert [tuple(p) for p in prims["p0"][63:67]] == corners and [tuple(p) for p in prims["p1"][63:67]] == corners[1:] + corners[:1]
    assert prims[-1]["p0"].tolist() == [170, 0] and prims[-1]["radius"] == 2 and prims[-1]["colour"][:3].tolist() == [0, 255, 0]
    assert prims.dtype.itemsize == 32


# ---------------------------------------------------------------------------------------------- text
def test_every_glyph_of_the_four_lines_is_drawn_and_distinct():
    chars = set("0123456789.-") | set("naif")                       # what {:.3f} can produce (nan, inf)
    for line in ("speed: m/s", "steer:  throttle:  brake: ", "cmd: ", "predicted brake: ", "None", *V.CMD_NAMES.values()):
        chars |= set(line.lower())
    glyphs = {c: V.FONT[ord(c)] for c in chars}
    for c, g in glyphs.items():
        assert (g < 32).all() and (g.any() or c == " "), c                # five columns; only the space is empty
    assert len({g.tobytes() for g in glyphs.values()}) == len(glyphs)
    np.testing.assert_array_equal(V.FONT[ord("N")], V.FONT[ord("n")])
    rows = V.text_rows(5, 1.23456, -0.5, 0.25, 1.0, 0.0)
    assert bytes(rows[0]).rstrip(b"\0") == b"speed: 1.235m/s" and bytes(rows[1]).rstrip(b"\0") == b"steer: -0.500 throttle: 0.250 brake: 1.000"
    assert bytes(rows[2]).rstrip(b"\0") == b"cmd: change right" and bytes(rows[3]).rstrip(b"\0") == b"predicted brake: 0.000"
    assert bytes(V.text_rows(9, float("nan"), 0, 0, 0, 0)[2]).rstrip(b"\0") == b"cmd: None"
    frame = V.draw_text(np.zeros((50, 300, 3), np.uint8), rows)
    # a line's glyphs stand on its baseline, 6 pixels apart from x = 4: 's' of "speed" in rows 4 .. 10, columns 4 .. 8
    assert frame[4:11, 4:9, 0].astype(bool).tolist() == [[bool(V.FONT[ord("s"), r] >> (4 - c) & 1) for c in range(5)] for r in range(7)]
    assert not frame[:4].any() and not frame[11:14].any() and not frame[:, :4].any() and frame[14:21].any() and frame[34:41].any() and not frame[41:].any()
    small = V.draw_text(np.zeros((8, 20, 3), np.uint8), rows)        # clipped to the frame
    assert small.shape == (8, 20, 3) and small.any()


# ---------------------------------------------------------------------------------------------- the frame
def test_frame_shape_and_panel_offsets_at_the_agent_geometry():
    lay = V.layout((288, 768, 3), (192, 480, 3), AGENT_GRID, (3, 320, 320))
    assert (lay["H"], lay["w_rgb"], lay["w_tel"], lay["w_lidar"], lay["w_bev"], lay["W"]) == (320, 853, 800, 320, 320, 2293)
    assert (lay["x_tel"], lay["x_lidar"], lay["x_bev"]) == (853, 1653, 1973) and (lay["frame_h"], lay["frame_w"]) == (160, 1146)
    assert 160 * 1146 * 3 == 550080
    rgb, tel = images((288, 768, 3), (192, 480, 3))
    plan, locs, cmds, det, tgt = scene("full", AGENT_GRID, (160, 280))
    cmd, spd, steer, throt, brake, bra = controls()
    pts = cloud(AGENT_GRID, n=20000)
    frame = V.debug_view_numpy(rgb, tel, pts, bra, pred_bev(AGENT_GRID), plan, locs, cmds, det, tgt, cmd, spd, steer, throt, brake,
                               grid=AGENT_GRID, cmd_thresh=CMD_THRESH)
    assert frame.shape == (160, 1146, 3) and frame.dtype == np.uint8
    # primitives never bleed out of the LiDAR panel: a frame without them differs only there (one frame pixel = two canvas pixels)
    bare = V.compose_numpy(rgb, tel, pts, pred_bev(AGENT_GRID), V.primitives(plan[:0], locs[:0], cmds[:0], [[], []], tgt, ppm=4, cmd_thresh=CMD_THRESH)[:0],
                           V.text_rows(cmd, spd, steer, throt, brake, bra), grid=AGENT_GRID)
    diff = np.flatnonzero((frame != bare).any(axis=(0, 2)))
    assert len(diff) > 20 and diff.min() >= 1653 // 2 and diff.max() <= 1973 // 2


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_small_geometries_have_the_frames_the_gpu_tests_expect(name):
    grid, rs, ts, ego = GEOMETRIES[name]
    lay = V.layout(rs, ts, grid, pred_bev(grid).shape)
    assert (lay["frame_h"], lay["frame_w"], lay["W"]) == FRAMES[name]
    assert lay["frame_h"] > 16 and lay["frame_h"] % 16 and lay["frame_w"] > 32 and lay["frame_w"] % 32      # two tiles each way, the last partial
    for kind in SCENES:
        plan, locs, cmds, det, tgt = scene(kind, grid, ego)
        prims = V.primitives(plan, locs, cmds, det, tgt, ppm=grid[4], cmd_thresh=CMD_THRESH, ego=ego)
        assert np.abs(prims["p0"]).max() <= V.COORD_LIMIT
        if kind in ("full", "pile"):
            assert (prims["kind"] == V.DOT).sum() == 20 + 1800 + 1 and (prims["kind"] == V.SEGMENT).sum() == 60


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        V.layout((288, 768, 3), (192, 480, 3), AGENT_GRID, (3, 160, 320))
    with pytest.raises(ValueError):
        V.layout((288, 768), (192, 480, 3), AGENT_GRID, (3, 320, 320))
    with pytest.raises(ValueError):
        V.check_primitives(np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        V.check_text(np.zeros((3, V.TEXT_LEN), np.uint8))
    with pytest.raises(ValueError):
        V.bev_panel(np.zeros((3, 4, 4), np.float64))
    rec = V.ViewRecorder("nowhere", 0)
    assert len(rec) == 0 and rec.flush() is None and rec.frames().shape[0] == 0 and not os.path.exists("nowhere")
