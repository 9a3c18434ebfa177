"""Shared by tests/test_log_view_host.py and tests/test_gpu_log_view.py: the small mixed frame, its scenes, and seeded views of the
four trainers at their real geometries."""
import numpy as np

from lav_amd.train import log_view as V

LIST = 512          # csrc/log_view.hip: the records a tile's LDS list holds
TW, TH = 32, 8      # its tile

# The mixed frame: 75 rows x 131 columns (neither a multiple of the 32 x 8 tile: 5 x 10 tiles, the last of both partial), five
# panels of the five kinds at 37 x 53 and 41 x 47 (rows x columns).  The second 41-row panel runs past the frame's bottom edge.
FRAME_HW = (75, 131)
SCENES = ("empty", "straddle", "overflow", "degenerate", "text")


def mixed_sources(seed=0, constant_planes=False):
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    logits = rng.normal(size=(5, 41, 47)).astype(np.float32)
    logits[3, ::3] = logits[1, ::3]                       # forced ties: the first maximum wins
    logits[:, 5, :] = 0.25                                # every class equal
    logits[4, 7, ::2] = logits.max() + 1.0
    logits[2, 7, ::4] = logits[4, 7, ::4]
    logits[2, 9, 1::2], logits[0, 9, 3::4] = np.nan, np.nan      # a NaN counts as a maximum, the first NaN wins
    logits[1, 11, :] = np.inf
    logits[3, 11, ::2] = np.inf
    logits[:, 13, :] = -np.inf
    planes = rng.uniform(0, 1, (3, 37, 53)).astype(np.float32)
    planes[:, 0, :3] = [[1.0, 0.0, 1 / 3], [1.0, 0.0, 1 / 3], [1.0, 0.0, 1 / 3]]
    planes[1, 2, 4], planes[0, 3, 5], planes[2, 4, 6] = np.nan, np.inf, -np.inf
    if constant_planes:
        planes = np.full((3, 37, 53), 0.7, np.float32)
    labels = rng.integers(-1, 7, (41, 47)).astype(np.int64)      # below, inside and past the palette
    return [image, logits, planes, labels]


def mixed_panels():
    return V.panel_table([dict(kind=V.IMAGE_U8, x=0, y=0, w=53, h=37, source=0), dict(kind=V.LOGITS, x=53, y=0, w=47, h=41, source=1, labels=[4, 6, 7, 10]),
                          dict(kind=V.PLANES, x=0, y=38, w=53, h=37, source=2), dict(kind=V.LABELS, x=53, y=41, w=47, h=41, source=3, labels=[4, 10, 18]),
                          dict(kind=V.SOLID, x=100, y=0, w=31, h=75, colour=(40, 80, 120))])


def colour_of(i):
    return (1 + i % 255, 1 + (i // 255) % 255, 7 + 3 * (i % 80))


def mixed_scene(kind, seed=1):
    """(prims, text) of a scene on the mixed frame."""
    rng = np.random.default_rng(seed)
    p = V._Prims()
    text = []
    if kind == "straddle":
        # across panel borders (clipped to the named panel), tile borders (x = 32, 64, 96; y = 8, 16 ...) and the frame's edges
        for panel, (w, h) in enumerate(((53, 37), (47, 41), (53, 37), (47, 41), (31, 75))):
            for k, (x, y) in enumerate(((0, 0), (w - 1, h - 1), (w, h // 2), (-1, 3), (w // 2, -2), (w // 2, h + 1), (w + 40, h + 40))):
                p.dot(panel, (x, y), 1 + k % 4, colour_of(10 * panel + k))
            p.segment(panel, (-9, h // 3), (w + 9, 2 * h // 3), colour_of(100 + panel))
            p.segment(panel, (w // 3, -20), (w // 2, h + 20), colour_of(110 + panel))
            p.convex(panel, [(w - 12, h - 9), (w + 6, h - 6), (w + 3, h + 8), (w - 9, h + 2)], colour_of(120 + panel))
            p.convex(panel, [(-5, -4), (11, 2), (3, 13)], colour_of(130 + panel))
        p.convex(0, [(20, 3), (50, 6), (47, 30), (25, 20)], colour_of(140))            # spans tiles (32 | 64, several rows of tiles)
        p.convex(4, [(-(1 << 20), -(1 << 20)), (1 << 20, -(1 << 20)), (1 << 20, 30), (-(1 << 20), 20)], colour_of(141))
        p.segment(3, (-(1 << 20), 10), (1 << 20, 25), colour_of(142))
        p.dot(2, (1 << 20, 1 << 20), 1024, colour_of(143))
    elif kind == "overflow":
        # one tile (columns 64 .. 95, rows 16 .. 23 of the frame = panel 1's columns 11 .. 42) touched by more records than its list
        # holds: LIST + 37 dots of distinct colours over a few pixels - an order error shows
        for i in range(LIST + 37):
            p.dot(1, (int(rng.integers(14, 40)), int(rng.integers(17, 23))), int(rng.integers(0, 3)), colour_of(i))
        p.segment(1, (0, 20), (46, 20), colour_of(LIST + 40))          # through the pile, after it
        for i in range(300):                                            # and records elsewhere, interleaved in the scans that follow
            p.dot(int(rng.integers(0, 5)), (int(rng.integers(0, 60)), int(rng.integers(0, 60))), 1, colour_of(600 + i))
    elif kind == "degenerate":
        p.convex(0, [(5, 5), (30, 20), (30, 20), (5, 5)], colour_of(1))              # zero area: only its edges
        p.convex(0, [(10, 30), (20, 30), (40, 30), (30, 30)], colour_of(2))          # collinear, out of order
        p.convex(1, [(7, 7), (7, 7), (7, 7), (7, 7)], colour_of(3))                  # a point
        p.convex(1, [(3, 30), (43, 30), (43, 30)], colour_of(4))                     # a degenerate triangle
        p.convex(2, [(10, 10), (30, 10), (10, 30), (30, 30)], colour_of(5))          # not convex (a bow tie): the rule's own answer
        p.convex(3, [(30, 5), (5, 5), (5, 25), (30, 25)], colour_of(6))              # the other orientation
    elif kind == "text":
        text = [(4, 10, "left"), (100, 20, "runs off the right edge of the frame"), (-8, 40, "starts left of it"), (60, 3, "cut at the top"),
                (3, 78, "bottom"), (40, 60, "0123456789:./-+_")]
    elif kind != "empty":
        raise KeyError(kind)
    return p.table(), V.text_table(text)


# ---------------------------------------------------------------------------------------------- the trainers' views
def seeded_dets(rng, n, hw=320):
    return [[(int(rng.integers(0, hw)), int(rng.integers(0, hw)), float(rng.uniform(0.5, 12)), float(rng.uniform(1, 25)), float(rng.normal()),
              float(rng.normal())) for _ in range(k)] for k in (n // 3, n - n // 3)]


def seeded_view(what, ndet=0, seed=5, hw=320):
    """A seeded opt_info "view" of trainer `what` at its real geometry, sources as NumPy arrays."""
    rng = np.random.default_rng(seed + ndet)
    f32 = np.float32
    px = lambda *shape: rng.uniform(-20, hw + 20, shape + (2,))          # noqa: E731  (pixels, some outside the panel)
    if what == "bev":
        return dict(bev=(rng.random((9, hw, hw)) < 0.1).astype(f32), cmd=int(rng.integers(0, 6)), nxp=px()[()] * 2, ego_plan_locs=px(20),
                    ego_cast_locs=px(6, 20), ego_cast_cmds=rng.uniform(0, 1, 6).astype(f32))
    if what == "lidar":
        cmds = rng.uniform(0, 1, (ndet, 6)).astype(f32)
        if ndet:
            cmds[0, 0] = np.nan
        return dict(bev=(rng.random((9, hw, hw)) < 0.1).astype(f32), pred_bev=rng.uniform(0, 1, (3, hw, hw)).astype(f32), cmd=int(rng.integers(0, 6)),
                    nxp=px()[()], det=seeded_dets(rng, ndet, hw), gt_det=seeded_dets(rng, ndet, hw), ego_plan_locs=px(20), ego_next_locs=px(21),
                    other_next_locs=px(6, 21), other_cast_locs=px(ndet, 6, 20), other_cast_cmds=cmds)
    if what == "seg":
        return dict(rgb=rng.integers(0, 256, (288, 256, 3), dtype=np.uint8), sem=rng.integers(0, 5, (288, 256)).astype(np.int64),
                    pred_sem=rng.normal(size=(5, 288, 256)).astype(f32))
    if what == "bra":
        return dict(rgb1=rng.integers(0, 256, (288, 768, 3), dtype=np.uint8), rgb2=rng.integers(0, 256, (192, 480, 3), dtype=np.uint8),
                    pred_sem1=rng.normal(size=(4, 72, 192)).astype(f32), pred_sem2=rng.normal(size=(4, 48, 120)).astype(f32), bra=1.0,
                    pred_bra=float(rng.uniform(0, 1)))
    raise KeyError(what)


def decode_png(data: bytes) -> np.ndarray:
    """PNG bytes -> (h, w, 3) uint8 RGB, through lav_amd.data.image's decoder."""
    from lav_amd.data.image import IMREAD_COLOR, imdecode
    return np.ascontiguousarray(imdecode(data, IMREAD_COLOR)[..., ::-1])
