"""CPU checks of the box-metric specification (lav_amd.train.evaluate_det): hand-derived IoUs, exact rational clipping, the corners against
log_view.quad_corners, arm 0 against eval_frame_numpy, thresholds, ties, greedy order, invalid boxes, bin edges, and the ground-truth
boxes against the loader's own targets on the fixture routes.  The kernel is compared with this specification in
tests/test_gpu_eval_det.py."""
from fractions import Fraction

import numpy as np
import pytest

from lav_amd.train import evaluate as E
from lav_amd.train import evaluate_det as ED
from tests import eval_det_util as U

Q = 1 << 20


def run(f, acc=None, **kw):
    k = dict(f["kw"])
    k.update(kw)
    acc = ED.DetLayout(k.get("nbins", 256)).zeros() if acc is None else acc
    ED.eval_det_numpy(acc, *U.positional(f), **k)
    return acc


def fields(acc):
    lay = ED.DetLayout.of(acc)
    return {name: lay.view(acc, name) for name in lay.fields}


def boxes(pred, gt):
    return ED.box_of(*pred), ED.box_of(*gt)


# ------------------------------------------------------------------------------------------------------------ geometry by hand
@pytest.mark.parametrize("name", [k for k, v in U.HAND.items() if v[2] is not None])
def test_hand_derived_ious(name):
    pred, gt, want = U.HAND[name]
    p, g = boxes(pred, gt)
    got = ED.iou(p, g)
    assert abs(got - want) <= 1e-12, (name, got, want)
    if want in (0.0, 0.5, 1.0):
        assert ED.iou_quanta(p, g) == int(want * Q)
    assert abs(ED.iou(g, p) - got) <= 1e-12          # symmetric


def test_octagon_has_eight_vertices_and_its_area():
    pred, gt, _ = U.HAND["octagon"]
    p, g = boxes(pred, gt)
    poly = ED.clip(p[0], g[0])
    assert len(poly) == 8
    assert abs(ED.area(poly) - 2.0 * (np.sqrt(2.0) - 1.0)) <= 1e-12


def test_iou_is_symmetric_on_random_boxes():
    rng = np.random.default_rng(4)
    for _ in range(300):
        a = (rng.uniform(10, 20), rng.uniform(10, 20), rng.uniform(0.5, 5), rng.uniform(0.5, 5), *rng.normal(size=2))
        b = (rng.uniform(10, 20), rng.uniform(10, 20), rng.uniform(0.5, 5), rng.uniform(0.5, 5), *rng.normal(size=2))
        p, g = boxes(a, b)
        assert abs(ED.iou(p, g) - ED.iou(g, p)) <= 1e-12
        assert len(ED.clip(p[0], g[0])) <= 8


def test_corners_are_log_view_quad_corners():
    from lav_amd.train.log_view import quad_corners
    rng = np.random.default_rng(2)
    for _ in range(200):
        a = rng.uniform(-np.pi, np.pi)
        x, y, w, h = rng.uniform(0, 300), rng.uniform(0, 300), rng.uniform(0.5, 10), rng.uniform(0.5, 20)
        got = np.asarray(ED.box_of(x, y, w, h, np.cos(a), np.sin(a))[0])
        np.testing.assert_allclose(got, quad_corners(x, y, w, h, np.cos(a), np.sin(a)), rtol=0, atol=1e-9)
        # counter-clockwise in (x, y): the cross product of consecutive edges is positive
        e = np.roll(got, -1, axis=0) - got
        assert (e[:, 0] * np.roll(e, -1, axis=0)[:, 1] - e[:, 1] * np.roll(e, -1, axis=0)[:, 0] > 0).all()
    # a direction that is no unit vector gives the same box
    np.testing.assert_allclose(np.asarray(ED.box_of(5, 6, 2, 3, 3.0, 4.0)[0]), quad_corners(5, 6, 2, 3, 0.6, 0.8), rtol=0, atol=1e-9)


# ------------------------------------------------------------------------------------------------------------ exact clipping
def _exact_iou(pred, gt):
    """The specification's clipping restated in fractions.Fraction; boxes (cx, cy, w, h, (a, b, hyp)) with direction (a / hyp, b / hyp)."""
    def corners(cx, cy, w, h, tri):
        c, s = Fraction(tri[0], tri[2]), Fraction(tri[1], tri[2])
        ux, uy, vx, vy = s, -c, c, s
        return [(cx - w * ux - h * vx, cy - w * uy - h * vy), (cx + w * ux - h * vx, cy + w * uy - h * vy),
                (cx + w * ux + h * vx, cy + w * uy + h * vy), (cx - w * ux + h * vx, cy - w * uy + h * vy)]
    poly, G = corners(*pred), corners(*gt)
    for k in range(4):
        gx, gy = G[k]
        ex, ey = G[(k + 1) % 4][0] - gx, G[(k + 1) % 4][1] - gy
        out = []
        for i in range(len(poly)):
            (sx, sy), (tx, ty) = poly[i], poly[(i + 1) % len(poly)]
            dS, dE = ex * (sy - gy) - ey * (sx - gx), ex * (ty - gy) - ey * (tx - gx)
            if dS >= 0:
                out.append((sx, sy))
            if (dS >= 0) != (dE >= 0):
                t = dS / (dS - dE)
                out.append((sx + t * (tx - sx), sy + t * (ty - sy)))
        poly = out
    total = Fraction(0)
    for i in range(1, len(poly) - 1):
        ax, ay, bx, by = poly[i][0] - poly[0][0], poly[i][1] - poly[0][1], poly[i + 1][0] - poly[0][0], poly[i + 1][1] - poly[0][1]
        total += ax * by - ay * bx
    a = abs(total) / 2
    union = 4 * pred[2] * pred[3] + 4 * gt[2] * gt[3] - a
    return a / union if a > 0 else Fraction(0)


EXACT_SEED = 11


def test_float64_iou_against_exact_rational_clipping():
    rng = np.random.default_rng(EXACT_SEED)
    triples = []
    for a, b, h in ((3, 4, 5), (5, 12, 13), (8, 15, 17)):
        for x, y in ((a, b), (b, a)):
            triples += [(sx * x, sy * y, h) for sx in (1, -1) for sy in (1, -1)]
    grid = lambda lo, hi: Fraction(int(rng.integers(lo * 64, hi * 64 + 1)), 64)
    skipped = positive = 0
    for _ in range(200):
        cx, cy = grid(10, 20), grid(10, 20)
        pred = (cx + grid(-3, 3), cy + grid(-3, 3), grid(1, 4), grid(1, 6), triples[int(rng.integers(len(triples)))])
        gt = (cx, cy, grid(1, 4), grid(1, 6), triples[int(rng.integers(len(triples)))])
        exact = _exact_iou(pred, gt)
        as_float = lambda b: ED.box_of(float(b[0]), float(b[1]), float(b[2]), float(b[3]), float(b[4][0]), float(b[4][1]))
        p, g = as_float(pred), as_float(gt)
        got = ED.iou(p, g)
        assert abs(got - float(exact)) <= 1e-9, (pred, gt, got, float(exact))
        positive += exact > 0
        scaled = exact * Q
        if abs(scaled - (int(scaled) + Fraction(1, 2))) <= Fraction(1, 10 ** 6):
            skipped += 1
            continue
        assert ED.iou_quanta(p, g) == min(Q, int(scaled + Fraction(1, 2))), (pred, gt)
    assert skipped <= 2 and positive >= 150, (skipped, positive)


# ------------------------------------------------------------------------------------------------------------ the specification's behaviour
def test_arm_0_is_eval_frame_numpy():
    from tests import eval_util as EU
    for seed in range(50):
        f = U.random_scene(100 + seed, D=20, G=12, used=14, heavy=seed % 2 == 1, bad=seed % 5 == 0)
        got = fields(run(f))
        e = EU.blank(h=U.H, w=U.W, G=12)
        e.update(rows=f["rows"], typs=f["typs"], n=f["n"])
        e["locs"] = np.zeros((12, EU.T + 1, 2), np.float32)
        e["locs"][:, 0] = f["locs"][:, 0]
        acc = E.ACC.zeros()
        E.eval_frame_numpy(acc, *EU.positional(e), ppm=U.PPM, centre=U.CENTRE, radius_px=U.RADIUS)
        assert (got["n_gt"].sum(axis=1) == E.ACC.view(acc, "n_gt")).all()
        assert (got["det"][0].sum(axis=1) == E.ACC.view(acc, "det")).all()
        assert (got["hist"][0] == E.ACC.view(acc, "hist")).all()
        assert got["det"][0].sum() > 0


def _overlap_scene(target_q):
    """A row whose iou_q with its actor is exactly target_q: axis-aligned boxes on one centre, the prediction narrower."""
    # IoU = (2 w_p)(2 h) / ((2 w_g)(2 h)) = w_p / w_g, dyadic: exact
    return U.pair_scene((20.0, 12.0, 4.0 * target_q / Q, 3.0, 1.0, 0.0), (20.0, 12.0, 4.0, 3.0, 1.0, 0.0), iou_thresholds=U.DYADIC)


def test_threshold_edge_is_kept_and_one_quantum_below_is_not():
    for k, t in enumerate(U.DYADIC):
        L = int(t * Q)
        at, below = fields(run(_overlap_scene(L))), fields(run(_overlap_scene(L - 1)))
        assert at["sum_iou"].sum() == L and below["sum_iou"].sum() == L - 1
        assert at["det"][1 + k, 1].sum(axis=0).tolist() == [1, 0]
        assert below["det"][1 + k, 1].sum(axis=0).tolist() == [0, 1]
        for j in range(k):                                # the lower thresholds keep both
            assert at["det"][1 + j, 1].sum(axis=0).tolist() == [1, 0] and below["det"][1 + j, 1].sum(axis=0).tolist() == [1, 0]


def test_ties_go_to_the_lowest_index():
    f = U.blank(D=2, G=4)
    U.put_actor(f, 1, 1, 18.0, 12.0, 2.0, 2.0)           # the same overlap with the row from either side
    U.put_actor(f, 3, 1, 22.0, 12.0, 2.0, 2.0)
    U.put_actor(f, 0, 0, 18.0, 12.0 + 10, 2.0, 2.0)
    U.put_row(f, 1, 0, 0.9, 20.0, 12.0, 2.0, 2.0)
    U.put_row(f, 1, 1, 0.8, 22.0, 12.0, 2.0, 2.0)
    got = fields(run(f, iou_thresholds=(0.25,)))
    # row 0 takes actor 1 in both arms (IoU 1/3 with each), so row 1 finds actor 3 free: IoU 1, distance 0
    assert got["det"][0, 1].sum(axis=0).tolist() == [2, 0] and got["det"][1, 1].sum(axis=0).tolist() == [2, 0]
    assert got["sum_iou"].sum() == int(np.rint(Q / 3)) + Q
    assert got["sum_centre"].sum() == int(0.5 * Q)       # 2 px = 0.5 m, then 0


def test_greedy_order_decides_between_two_rows():
    f = U.blank(D=2, G=1)
    U.put_actor(f, 0, 1, 20.0, 12.0, 2.0, 2.0)
    U.put_row(f, 1, 0, 0.9, 21.0, 12.0, 2.0, 2.0)        # the worse fit comes first and takes the actor
    U.put_row(f, 1, 1, 0.8, 20.0, 12.0, 2.0, 2.0)
    got = fields(run(f, iou_thresholds=(0.5,)))
    assert got["det"][0, 1].sum(axis=0).tolist() == [1, 1] and got["det"][1, 1].sum(axis=0).tolist() == [1, 1]
    assert got["sum_iou"].sum() == int(np.rint(Q * 3 / 5))
    hist = got["hist"]
    b9, b8 = int(np.float32(0.9) * np.float32(256)), int(np.float32(0.8) * np.float32(256))
    assert hist[0, 1, 0, b9] == 1 and hist[0, 1, 1, b8] == 1 and hist[1, 1, 0, b9] == 1 and hist[1, 1, 1, b8] == 1


BROKEN = [(0.0, 3.0, 1.0, 0.0), (2.0, -1.0, 1.0, 0.0), (2.0, 3.0, 0.0, 0.0), (np.nan, 3.0, 1.0, 0.0), (2.0, np.inf, 1.0, 0.0), (2.0, 3.0, np.nan, 0.0)]


@pytest.mark.parametrize("broken", BROKEN)
def test_invalid_boxes_land_in_their_counters_only(broken):
    good = (2.0, 3.0, 1.0, 0.0)
    for side in ("pred", "gt", "both"):
        p = broken if side in ("pred", "both") else good
        g = broken if side in ("gt", "both") else good
        got = fields(run(U.pair_scene((20.0, 12.0, *p), (20.0, 12.0, *g))))
        assert got["pred_invalid"].tolist() == [0, int(side != "gt")] and got["gt_invalid"].tolist() == [0, int(side != "pred")]
        assert got["pair_invalid"].tolist() == [0, 1] and got["pairs"].sum() == 1 and got["n_gt"].sum() == 1
        assert got["det"][0, 1].sum(axis=0).tolist() == [1, 0]              # the centre arm does not look at the box
        assert got["det"][1:, 1].sum(axis=(0, 1)).tolist() == [0, 3]        # IoU 0 with everything
        for name in ("sum_centre", "sum_dw", "sum_dh", "sum_iou", "heading"):
            assert got[name].sum() == 0, name


def test_range_bins_at_their_exact_edges():
    # edges 1, 2, 3 m = 4, 8, 12 px from the ego pixel (26, 30)
    f = U.blank(D=4, G=4)
    for g, dx in enumerate((3.75, 4.0, 8.0, 12.0)):
        U.put_actor(f, g, 1, 26.0 + dx, 30.0, 2.0, 2.0)
        U.put_row(f, 1, g, 0.9 - 0.1 * g, 26.0 + dx, 30.0, 2.0, 2.0)
    f["rows"][1, 2, 2] = 0.0                              # row 2 is 30 px off its actor: a false positive in its own bin (d = sqrt(64 + 900))
    got = fields(run(f, range_edges_m=(1, 2, 3)))
    assert got["n_gt"][1].tolist() == [1, 1, 1, 1]
    assert got["det"][0, 1].tolist() == [[1, 0], [1, 0], [0, 0], [1, 1]]
    assert got["pairs"][1].tolist() == [1, 1, 0, 1]


def test_heading_bins_at_0_90_and_180_degrees():
    for (c, s), want in (((1.0, 0.0), 0), ((0.0, 1.0), 5), ((-1.0, 0.0), 7), ((0.0, -1.0), 5)):
        got = fields(run(U.pair_scene((20.0, 12.0, 2.0, 2.0, c, s), (20.0, 12.0, 2.0, 2.0, 1.0, 0.0))))
        assert got["heading"][1].tolist() == [int(b == want) for b in range(8)], (c, s)
    s = ED.summarise(run(U.pair_scene((20.0, 12.0, 2.0, 4.0, -1.0, 0.0), (20.0, 12.0, 2.0, 4.0, 1.0, 0.0))))
    assert s["classes"][1]["heading_flipped"] == 1.0 and s["classes"][1]["heading_within_10deg"] == 0.0 and s["classes"][1]["mean_iou"] == 1.0


def test_accumulation_does_not_depend_on_frame_order():
    frames = [U.random_scene(s, heavy=s % 2 == 0, bad=s % 3 == 0) for s in range(8)]
    a, b = ED.DetLayout().zeros(), ED.DetLayout().zeros()
    for f in frames:
        run(f, a)
    for f in reversed(frames):
        run(f, b)
    assert (a == b).all() and fields(a)["frames"].sum() == 8
    assert fields(a)["sum_iou"].sum() > 0 and fields(a)["pair_invalid"].sum() > 0 and fields(a)["heading"].sum() > 0


def test_summarise_of_an_empty_accumulator_has_no_nan():
    import json
    s = ED.summarise(ED.DetLayout().zeros())
    assert "NaN" not in json.dumps(s) and s["classes"][0]["mean_iou"] is None and s["classes"][1]["arms"]["centre"]["ap"] is None
    assert s["arms"] == ["centre", "iou0.3", "iou0.5", "iou0.7"]


def test_layout_has_the_length_the_library_says():
    from lav_amd import _lib
    lib = _lib.load()
    assert len(ED.DetLayout()) == lib.lav_eval_det_words(256) == 135 + 16 * 256
    assert len(ED.DetLayout(1)) == lib.lav_eval_det_words(1) and len(ED.DetLayout(1024)) == lib.lav_eval_det_words(1024)
    assert lib.lav_eval_det_words(0) == 0 and lib.lav_eval_det_words(1025) == 0
    assert ED.DetLayout.of(ED.DetLayout(7).zeros()).nbins == 7
    both = ED.det_layout(ED.HEADS)
    assert len(both) == 2 * len(ED.DetLayout()) and list(both.sections) == ["peaks", "dense"]


def test_thresholds_are_refused_where_they_make_no_sense():
    for kw in (dict(iou_thresholds=(0.1, 0.2, 0.3, 0.4)), dict(iou_thresholds=(0.0,)), dict(range_edges_m=(30, 15)), dict(heading_edges_deg=(0,)),
               dict(range_edges_m=(1, 2, 3, 4))):
        with pytest.raises(ValueError):
            ED.thresholds(4.0, **kw)
    L, r2, hc = ED.thresholds(4.0)
    assert L.tolist() == [int(np.rint(t * Q)) for t in (0.3, 0.5, 0.7)] and r2.tolist() == [3600.0, 14400.0, 40000.0] and len(hc) == 7


# ------------------------------------------------------------------------------------------------------------ the loader's targets
def test_ground_truth_boxes_are_the_loaders_own_and_a_perfect_detector_scores_one(tmp_path):
    """On the fixture routes every in-map actor whose nearest other actor is more than 2 px away reads exactly its own bbox * ppm and
    float32 cos / sin(ori) at the evaluator's pixel; a detector that outputs those boxes scores AP 1 in every arm."""
    from lav_amd.data.datasets import to_ego_frame
    from lav_amd.train.lav import TrainConfig
    from tests.util import dataset_fixture_config
    frames = E.held_out_frames(dataset_fixture_config(str(tmp_path), routes=2, frames=26), seed=0)
    ds = frames.dataset
    cfg = TrainConfig()
    ppm, centre, Hm, Wm = float(cfg.pixels_per_meter), (160.0, 280.0), 320, 320
    acc = ED.DetLayout().zeros()
    qualified = in_map = 0
    for idx in range(len(frames)):
        item = frames[idx]
        size, ori, locs, oris, typs, n = item[3].numpy(), item[4].numpy(), item[10], item[11], item[12], int(item[13])
        txn, index = ds.txn_map[idx], ds.idx_map[idx]
        _, ego_locs, ego_oris, _, _, t_locs, t_oris, t_bbox, t_typs = ds._tracks(txn, index)
        bbox = to_ego_frame(ego_locs, t_locs, t_oris, t_bbox, t_typs, ego_oris[0], ds.num_plan + 1)[3][:, 0]
        px = locs[:n, 0, 0].astype(np.float64) * ppm + centre[0]
        py = locs[:n, 0, 1].astype(np.float64) * ppm + centre[1]
        rows = np.zeros((2, 32, 7), np.float32)
        rows[..., 0] = -1e5
        count, clean = [0, 0], True
        for g in range(n):
            if not (0.0 <= px[g] < Wm and 0.0 <= py[g] < Hm):
                continue
            in_map += 1
            others = [np.hypot(px[k] - px[g], py[k] - py[g]) for k in range(n) if k != g]
            ix, iy = min(Wm - 1, int(px[g] + 0.5)), min(Hm - 1, int(py[g] + 0.5))
            if others and min(others) <= 2.0:
                clean = False
                continue
            qualified += 1
            want_size = (bbox[g].astype(np.float32) * np.float32(ppm))
            want_ori = np.array([np.cos(np.float32(oris[g])), np.sin(np.float32(oris[g]))], np.float32)
            assert (size[:, iy, ix] == want_size).all(), (idx, g, size[:, iy, ix], want_size)
            assert (ori[:, iy, ix] == want_ori).all(), (idx, g, ori[:, iy, ix], want_ori)
            c = int(typs[g])
            rows[c, count[c]] = (0.9, px[g], py[g], *want_size, *want_ori)
            count[c] += 1
        if clean:                                          # the perfect detector: every actor's own box, where all of them are known
            ED.eval_det_numpy(acc, rows, locs, typs, n, size, ori, ppm=ppm, centre=centre, radius_px=2.0 * ppm)
    assert qualified >= 50, (qualified, in_map)
    s = ED.summarise(acc)
    f = fields(acc)
    assert f["pairs"].sum() >= 50 and f["pair_invalid"].sum() == 0 and f["gt_invalid"].sum() == 0
    for c in range(2):
        k = s["classes"][c]
        if k["n_gt"] == 0:
            continue
        for arm in s["arms"]:
            assert k["arms"][arm]["ap"] == 1.0, (c, arm, k["arms"][arm])
        # a row carries float32(px): at most 2^-17 px off below 256 px, which costs a box of half extents w, h at most 2^-17 (1 / w + 1 / h)
        # of its IoU - below 1e-4 for any box of more than 0.2 px
        assert abs(k["mean_iou"] - 1.0) <= 1e-4 and k["heading_hist"][0] == k["pairs"] and k["heading_within_10deg"] == 1.0
        assert k["mean_dw"] == 0.0 and k["mean_dh"] == 0.0 and k["mean_centre_error"] <= 2.0 ** -17
