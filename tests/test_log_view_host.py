"""The trainers' visual log on the CPU (lav_amd/train/log_view.py): the palette against the reference's own
visualize_semantic_processed and the detection boxes' corners against matplotlib's Rectangle (tests/golden/log_view.npz, written by
tests/golden/make_golden_log.py), the polygon rule against Python integers, drawing order and clipping, the PLANES and LOGITS rules
at their edges, the PNG writer, and train_bev_v2.py --log-dir from the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lav_amd.train import log_view as V
from tests.log_view_util import FRAME_HW, SCENES, decode_png, mixed_panels, mixed_scene, mixed_sources, seeded_view

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "log_view.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", ["seg", "bra", "default"])
def test_palette_is_the_references(golden, name):
    labels = [int(v) for v in golden[f"palette/{name}_labels"]]
    assert labels == {"seg": [4, 6, 7, 10], "bra": list(V.BRA_LABELS), "default": list(V.DEFAULT_LABELS)}[name]
    sem = golden["palette/sem"]
    np.testing.assert_array_equal(V.palette_image(sem, V.palette_of(labels)), golden[f"palette/{name}"])
    # and through a LABELS panel of the specification
    panels = V.panel_table([dict(kind=V.LABELS, x=0, y=0, w=sem.shape[1], h=sem.shape[0], source=0, labels=labels)])
    frame = V.log_view_numpy(panels, V._Prims().table(), V.text_table([]), [sem])
    np.testing.assert_array_equal(frame, golden[f"palette/{name}"])
    assert {int(r[0]): tuple(int(c) for c in r[1:]) for r in golden["palette/sem_colors"]} == V.SEM_COLORS


def test_quad_corners_are_matplotlibs(golden):
    for det, want in zip(golden["boxes/det"], golden["boxes/corners"]):
        x, y, w, h, cos, sin = det
        np.testing.assert_allclose(V.quad_corners(int(x), int(y), w, h, cos, sin), want, rtol=0, atol=1e-9)
    # what the lidar builder draws: those corners truncated, as a 4-vertex polygon followed by the arrow's shaft and head
    p = V._Prims()
    V._boxes(p, 0, [[tuple(golden["boxes/det"][0])], []])
    t = p.table()
    assert [int(k) for k in t["kind"]] == [V.CONVEX, V.SEGMENT, V.CONVEX] and [int(n) for n in t["n"]] == [4, 0, 3]
    np.testing.assert_array_equal(np.stack([t[0][k] for k in ("p0", "p1", "p2", "p3")]), V._to_pixel(golden["boxes/corners"][0]))
    assert tuple(t[0]["colour"][:3]) == V.ORANGE and tuple(t[1]["colour"][:3]) == V.BLACK


def brute_convex(pts, x, y):
    """Python integers: inside the vertices' box, and every edge function >= 0 or every one <= 0."""
    pts = [(int(a), int(b)) for a, b in pts]
    if not (min(p[0] for p in pts) <= x <= max(p[0] for p in pts) and min(p[1] for p in pts) <= y <= max(p[1] for p in pts)):
        return False
    e = [(b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0]) for a, b in zip(pts, pts[1:] + pts[:1])]
    return all(v >= 0 for v in e) or all(v <= 0 for v in e)


def test_convex_coverage_equals_python_integers():
    rng = np.random.default_rng(7)
    big = 1 << 20
    cases = [[(2, 3), (17, 5), (9, 16)], [(9, 16), (17, 5), (2, 3)],                                  # both orientations
             [(1, 1), (18, 2), (16, 17), (3, 14)], [(3, 14), (16, 17), (18, 2), (1, 1)],
             [(4, 4), (15, 15), (15, 15), (4, 4)],                                                    # a zero-area quad: its edge only
             [(5, 9), (5, 9), (5, 9), (5, 9)],
             [(6, 6), (12, 6), (12, 12), (6, 12)],                                                    # vertices and edges on pixel centres
             [(-big, -big), (big, -big), (big, big), (-big, big)],                                    # +-2^20
             [(-big, 3), (big, 9), (big, 11)], [(0, -big), (19, big), (10, big)]]
    for _ in range(40):
        n = int(rng.integers(3, 5))
        a = np.sort(rng.uniform(0, 2 * np.pi, n))
        cases.append([(int(10 + r * np.cos(t)), int(10 + r * np.sin(t))) for t, r in zip(a, rng.uniform(2, 14, n))])      # convex or not
    ys, xs = np.mgrid[-2:22, -2:22]
    for pts in cases:
        p = V._Prims()
        p.convex(0, pts, (1, 2, 3))
        got = V.prim_covers(p.table()[0], xs, ys)
        want = np.array([[brute_convex(pts, int(x), int(y)) for x in xs[0]] for y in ys[:, 0]])
        np.testing.assert_array_equal(got, want, err_msg=str(pts))
    zero = V._Prims()
    zero.convex(0, cases[4], (1, 2, 3))
    assert V.prim_covers(zero.table()[0], xs, ys).sum() == 12          # the diagonal from (4, 4) to (15, 15)


def test_order_of_drawing_and_clipping_to_the_named_panel():
    panels = V.panel_table([dict(kind=V.SOLID, x=0, y=0, w=20, h=16, colour=(10, 10, 10)), dict(kind=V.SOLID, x=20, y=0, w=20, h=16, colour=(20, 20, 20))])
    p = V._Prims()
    p.dot(0, (18, 8), 4, (255, 0, 0))                                   # runs over panel 0's right border: cut there
    p.convex(0, [(16, 6), (19, 6), (19, 10), (16, 10)], (0, 255, 0))    # later: over the dot
    p.dot(1, (-1, 8), 1, (0, 0, 255))                                   # centred left of panel 1: only its part inside
    p.dot(0, (17, 8), 0, (9, 9, 9))                                     # the last one wins its pixel
    frame = V.log_view_numpy(panels, p.table(), V.text_table([]), [])
    assert frame.shape == (16, 40, 3)
    assert tuple(frame[8, 14]) == (255, 0, 0) and tuple(frame[8, 16]) == (0, 255, 0) and tuple(frame[8, 17]) == (9, 9, 9)
    assert tuple(frame[8, 20]) == (0, 0, 255) and tuple(frame[8, 21]) == (20, 20, 20) and tuple(frame[8, 19]) == (0, 255, 0)
    assert not (frame[:, 20:] == (255, 0, 0)).all(axis=2).any() and not (frame[:, :20] == (0, 0, 255)).all(axis=2).any()
    with pytest.raises(ValueError):
        bad = p.table()
        bad["panel"][0] = 2
        V.log_view_numpy(panels, bad, V.text_table([]), [])


def test_planes_rule_at_its_edges():
    const = np.zeros((3, 6, 7), np.float32)
    assert not V.planes_grey(const).any()
    withnan = np.zeros((2, 4, 5), np.float32)
    withnan[0, 1, 1], withnan[1, 2, 2], withnan[:, 3, 3], withnan[0, 0, 4] = np.nan, 2.0, 1.0, np.inf
    g = V.planes_grey(withnan)
    assert g[1, 1] == 0 and g[0, 4] == 0 and g[2, 2] == 255 and g[3, 3] == 255 and g[0, 0] == 0      # means 0 .. 1; NaN and Inf -> 0
    withnan[1, 2, 2] = 1.5
    assert V.planes_grey(withnan)[2, 2] == int(np.floor(0.75 * 255.0 / 1.0))
    lo = np.float32(0.3)
    ulp = np.stack([np.full((2, 3), lo), np.full((2, 3), lo)])
    ulp[1, 0, 0] = np.nextafter(lo, np.float32(1))
    m = ulp.astype(np.float64).sum(0) / 2
    assert len(np.unique(m)) == 2
    g = V.planes_grey(ulp)
    assert g[0, 0] == 255 and g.sum() == 255
    one = np.array([[[1.0, np.nextafter(1.0, 2.0)]]])                   # hi - lo is one float64 ulp of the mean itself
    np.testing.assert_array_equal(V.planes_grey(one.astype(np.float64)), [[0, 255]])
    assert not V.planes_grey(np.full((1, 2, 2), np.nan, np.float32)).any()


def first_maximum(v):
    best = 0
    for c in range(1, len(v)):
        if v[best] != v[best]:
            break
        if v[c] > v[best] or v[c] != v[c]:
            best = c
    return best


def test_logits_ties_and_nan_agree_with_argmax():
    logits = mixed_sources()[1]
    labels = [4, 6, 7, 10]
    panels = V.panel_table([dict(kind=V.LOGITS, x=0, y=0, w=47, h=41, source=0, labels=labels)])
    frame = V.log_view_numpy(panels, V._Prims().table(), V.text_table([]), [logits])
    am = np.argmax(logits, axis=0)
    np.testing.assert_array_equal(frame, V.palette_image(am, V.palette_of(labels)))
    assert (am[5] == 0).all() and (am[9, 1::2] != 2).sum() == (am[9, 3::4] == 0).sum() > 0 and (am[13] == 0).all()
    for y in (5, 7, 9, 11, 13, 20):          # np.argmax's rule, spelt out: what the kernel's loop does
        assert [first_maximum(logits[:, y, x]) for x in range(47)] == am[y].tolist()


@pytest.mark.parametrize("scene", SCENES)
def test_mixed_frame_scenes_render(scene):
    prims, text = mixed_scene(scene)
    frame = V.log_view_numpy(mixed_panels(), prims, text, mixed_sources(), size=FRAME_HW)
    assert frame.shape == FRAME_HW + (3,) and frame.dtype == np.uint8
    empty = V.log_view_numpy(mixed_panels(), *mixed_scene("empty"), mixed_sources(), size=FRAME_HW)
    assert (frame != empty).any() == (scene != "empty")
    assert (empty[:, 100:] == (40, 80, 120)).all() and (empty[37, :53] == 0).all()          # the solid panel; the gap between two panels


@pytest.mark.parametrize("what,ndet,size", [("bev", 0, (320, 320)), ("lidar", 0, (332, 640)), ("lidar", 7, (332, 640)), ("seg", 0, (288, 768)),
                                            ("bra", 0, (360, 1248))])
def test_builders_lay_the_frames_out_from_the_shapes(what, ndet, size):
    view = seeded_view(what, ndet)
    frame = V.build_frame(what, view)
    assert frame.size == size
    img = V.render(frame)
    assert img.shape == size + (3,) and len(np.unique(img.reshape(-1, 3), axis=0)) > 3
    if what == "lidar":
        per_box = 3
        dots = 21 + 1 + 6 * 21 + 20 + ndet * 6 * 20
        assert len(frame.prims) == 2 * ndet * per_box + dots
    if what == "bra":
        top = 72
        assert [int(p["rect"][3]) for p in frame.panels[3:5]] == [V.bar_height(view["pred_bra"], top), top]


def test_png_writer_round_trips(tmp_path):
    rng = np.random.default_rng(3)
    for shape in ((1, 1, 3), (7, 13, 3), (75, 131, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        data = V.encode_png(img)
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and data.count(b"IDAT") == 1
        np.testing.assert_array_equal(decode_png(data), img)
    w = V.FrameWriter(str(tmp_path / "d"), "seg")
    a, b = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8), rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    w.add(a, 0)
    assert not os.path.exists(tmp_path / "d")                  # written when the next one arrives
    w.add(b, 5)
    assert sorted(os.listdir(tmp_path / "d")) == ["seg_0000000.png"]
    w.close()
    assert sorted(os.listdir(tmp_path / "d")) == ["seg_0000000.png", "seg_0000005.png"]
    np.testing.assert_array_equal(decode_png(open(tmp_path / "d" / "seg_0000005.png", "rb").read()), b)
    with pytest.raises(ValueError):
        V.encode_png(np.zeros((4, 4), np.uint8))


def _drive(tmp_path, *extra):
    import yaml
    cfgp = tmp_path / "config_v2.yaml"
    cfgp.write_text(yaml.safe_dump(dict(num_plan=20, num_cmds=6, cmd_weight=0.1, branch_weights=[5, 5, 5, 1, 1, 1], camera_x=1.5)))
    cmd = [sys.executable, os.path.join(REPO, "train_bev_v2.py"), "--synthetic", "--device", "cpu", "--config-path", str(cfgp), "--batch-size", "1",
           "--num-epoch", "1", "--steps-per-epoch", "3", "--num-per-log", "2", "--save-dir", str(tmp_path / "ck"), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, WORLD_SIZE="1", RANK="0"), cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.strip().splitlines()


def test_train_bev_log_dir_writes_the_logged_steps(tmp_path):
    d = tmp_path / "viz"
    lines = _drive(tmp_path, "--log-dir", str(d))
    assert json.loads(lines[-1])["steps"] == 3
    assert sorted(os.listdir(d)) == ["bev_0000000.png", "bev_0000002.png"]
    for name in os.listdir(d):
        img = decode_png(open(d / name, "rb").read())
        assert img.shape == (320, 320, 3) and len(np.unique(img)) > 2


def test_without_log_dir_nothing_is_written_and_the_keys_are_todays(tmp_path):
    before = set(os.listdir(tmp_path))
    lines = _drive(tmp_path)
    assert set(os.listdir(tmp_path)) - before == {"ck", "config_v2.yaml"} and os.listdir(tmp_path / "ck") == ["bev_1.th"]
    logged = [ln for ln in lines if ln[:1].isdigit()]
    assert len(logged) == 2 and "view" not in "".join(logged)
    from lav_amd.train import LAV, TrainConfig, synthetic_bev_batch
    torch.manual_seed(0)
    lav = LAV(TrainConfig(), torch.device("cpu"), what="bev")
    today = {"loss", "plan_loss", "ego_cast_loss", "other_cast_loss", "cmd_loss"}
    assert lav.log_view is False
    assert set(lav.train_bev(*synthetic_bev_batch(1, seed=3))) == today
    lav.log_view = True
    info = lav.train_bev(*synthetic_bev_batch(1, seed=4))
    assert set(info) == today | {"view"}
    assert set(info["view"]) == {"bev", "cmd", "nxp", "ego_plan_locs", "ego_cast_locs", "ego_cast_cmds"}
    assert tuple(info["view"]["bev"].shape) == (9, 320, 320) and info["view"]["ego_cast_locs"].shape == (6, 20, 2) and info["view"]["ego_cast_locs"].dtype == np.float64
