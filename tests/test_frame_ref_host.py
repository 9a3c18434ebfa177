"""The numpy references of the peak, decode and lidar-glue kernels (tests/frame_ref_util.py) checked on the CPU, before any kernel
is held to them: they equal the oracle where the oracle is defined (tie-free maps, the host decode, the BLAS stacking); every
table of tests/test_gpu_frame_edges.py satisfies the premise it was built for (ties present, candidate counts on the intended
side of the 2048 bound, filler rows); and every single-rule mistake a kernel could make changes the expected rows on those very
tables (selectivity).  The wrong variants below are copies of the reference, never the project's code."""
import math
import types

import numpy as np
import pytest
import torch

from oracle import bev as obev
from oracle import frame as oframe
from tests import frame_ref_util as U


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("shape,seed", [((2, 96, 96), 0), ((1, 37, 53), 2), ((3, 8, 300), 3)])
def test_peaks_ref_equals_the_oracle_on_tie_free_maps(shape, seed):
    heat = U.smooth_map(shape, seed)
    size, ori = U.gather_maps(shape[1], shape[2], seed)
    rows, _ = U.peaks_ref(heat, size, ori, 7, 15)
    W = shape[2]
    for c in range(shape[0]):
        more = U.peaks_ref(heat[c:c + 1], size, ori, 7, 16)[0][0, :, 0]      # no tie among the rows, nor with the first one left out
        more = more[more != U.FILLER]
        assert len(np.unique(more)) == len(more), "the map has ties: topk's order is unspecified there"
        score, loc = obev.extract_peak(torch.from_numpy(heat[c]))
        live = score.numpy() > -1e4
        assert live.sum() >= 3
        np.testing.assert_array_equal(rows[c, live, 0], score.numpy()[live])
        np.testing.assert_array_equal((rows[c, live, 2] * W + rows[c, live, 1]).astype(np.int64), loc.numpy()[live])
        np.testing.assert_array_equal(rows[c, ~live, 0], np.full((~live).sum(), U.FILLER))
        ys, xs = rows[c, live, 2].astype(int), rows[c, live, 1].astype(int)
        np.testing.assert_array_equal(rows[c, live, 3:5], size[:, ys, xs].T)
        np.testing.assert_array_equal(rows[c, live, 5:7], ori[:, ys, xs].T)


def test_det_decode_ref_equals_the_host_decode():
    """InferModel.det_decode_fast on the random rows of tests/test_gpu_frame.py, with the frame's constants."""
    from lav_amd.model_inference import InferModel
    up = types.SimpleNamespace(pixels_per_meter=4, offsets=lambda: (0.0, 0.75))
    im = types.SimpleNamespace(pixels_per_meter=4, uniplanner=up, _bev_hw=(320, 320))
    centre = (160.0, 280.0)
    rng = np.random.default_rng(3)
    seen = set()
    for trial in range(40):
        rows = np.zeros((2, 15, 7), np.float32)
        rows[..., 0] = np.sort(rng.uniform(0.0, 1.0, (2, 15)).astype(np.float32) ** (1 + trial % 3), axis=1)[:, ::-1]
        rows[..., 1] = rng.integers(0, 320, (2, 15)); rows[..., 2] = rng.integers(0, 320, (2, 15))
        rows[1, :4, 1] = 160 + rng.integers(-5, 6, 4); rows[1, :4, 2] = 280 + rng.integers(-5, 6, 4)
        rows[..., 3:5] = rng.uniform(0.0, 3.0, (2, 15, 2)); rows[1, 5, 3:5] = 0.39
        rows[..., 5:7] = rng.normal(0, 1, (2, 15, 2))
        actors, n = U.det_decode_ref(rows, 1, 0.2, (160, 280), 2.0, 30 * 4, 0.1 * 4, centre, 4.0, 4)
        _, locs, oris = InferModel.det_decode_fast(im, rows)
        assert n == len(locs)
        np.testing.assert_array_equal(actors[:2 * n].reshape(-1, 2), locs.astype(np.float32))
        np.testing.assert_array_equal(actors[30:30 + n], oris.astype(np.float32))
        assert not actors[2 * n:30].any() and not actors[30 + n:].any()
        seen.add(n)
    assert len(seen) >= 5


def test_sigmoid_exact_is_the_float32_formula_and_refuses_the_rest():
    v = np.array([-1e30, -200, -120, 0, 20, 40, 1e30, -np.inf, np.inf], np.float32)
    with np.errstate(over="ignore"):
        for off in (0.0, 1e-6, -1e-6):       # an expf that is off by many ulps (except at 0: exp(0) = 1) gives the same
            e = np.exp(-v.astype(np.float64)) * np.where(v == 0, 1.0, 1 + off)
            formula = np.float32(1) / (np.float32(1) + e.astype(np.float32))
            np.testing.assert_array_equal(U.sigmoid_exact(v), formula)
    for bad in (-119.0, -1.0, 1e-3, 19.5, np.nan):
        with pytest.raises(ValueError):
            U.sigmoid_exact(np.array([0.0, bad], np.float32))


def test_stack_sweeps_ref_is_the_oracle_up_to_the_matmul_and_not_its_fused_form():
    """Against oracle.frame.stack (BLAS matmul: summation order unspecified) within the existing GPU test's 2e-5; and the same
    product-sums with each multiply-add fused (one rounding instead of two: what a lost contraction pragma would compute) differ
    from the reference on the GPU test's inputs, so the bit-exact comparison there notices."""
    rows, slots = 300, 15
    rng = np.random.default_rng(5)
    ring = rng.standard_normal((slots, rows, 8)).astype(np.float32) * 20
    fused = rng.standard_normal((rows, 8)).astype(np.float32) * 20
    locs = {t: np.array([0.31 * t, -0.07 * t]) for t in range(slots)}
    oris = {t: 0.021 * t for t in range(slots)}
    sweeps, (loc0, ori0) = [12, 7, 2], (locs[12], oris[12])
    Rs, ts = [], []
    for t in sweeps:
        dloc = (locs[t] - loc0) @ np.array([[math.cos(ori0), -math.sin(ori0)], [math.sin(ori0), math.cos(ori0)]])
        o = oris[t] - ori0
        Rs.append([[math.cos(o), math.sin(o), 0.], [-math.sin(o), math.cos(o), 0.], [0., 0., 1.]])
        ts.append([dloc[0], dloc[1], 0.])
    got, after = U.stack_sweeps_ref(fused, ring, 12, sweeps, np.array(Rs, np.float32), np.array(ts, np.float32))
    hist = {t: ring[t] for t in range(slots)}
    hist[12] = fused
    want = oframe.stack([hist[t] for t in range(13)], [locs[t] for t in range(13)], [oris[t] for t in range(13)])
    np.testing.assert_allclose(got[:, :3], want[:, :3], rtol=0, atol=2e-5)
    np.testing.assert_array_equal(got[:, 3:], want[:, 3:])
    np.testing.assert_array_equal(after[12], fused)

    def fused_form(fz, rg, slot, sw, R, t):
        f64, out = np.float64, np.zeros((3, len(fz), 3), np.float32)
        for s in range(3):
            v = (fz if s == 0 else rg[sw[s]]).astype(f64)
            for c in range(3):
                a = (v[:, 0] * f64(R[s, 0, c])).astype(np.float32).astype(f64)
                a = (v[:, 1] * f64(R[s, 1, c]) + a).astype(np.float32).astype(f64)       # fma: the product is not rounded
                a = (v[:, 2] * f64(R[s, 2, c]) + a).astype(np.float32)
                out[s, :, c] = a + t[s, c]
        return out.reshape(-1, 3)
    for n in STACK_ROWS:
        d = U.stack_inputs(n, seed=n)
        ref = U.stack_sweeps_ref(*d)[0]
        if n >= 256:
            assert (fused_form(*d) != ref[:, :3]).sum() >= 10, "fused and unfused product-sums agree: the inputs do not discriminate"


STACK_ROWS = (1, 256, 257, 3000)


# ------------------------------------------------------------------------------------------------ premises of the GPU tables
@pytest.mark.parametrize("name", list(U.TIE_CASES))
def test_tie_table_premises(name):
    kind, shape, ks, max_det, _ = U.TIE_CASES[name]
    heat, _, _, _, _, _, rows, cand = U.peak_case(name)
    assert not np.signbit(heat[heat == 0]).any(), "-0.0 sorts below +0.0 by bit pattern: the builders avoid it"
    fill = U.filler_rows(rows)
    for c in range(shape[0]):
        real = rows[c, :max_det - fill[c], 0]
        values, counts = np.unique(real, return_counts=True)
        if kind == "tie":
            assert len(values) >= 2 and counts.max() >= 3, f"plane {c}: {len(values)} distinct scores, largest group {counts.max()}"
        elif kind == "top1":
            assert max_det == 1 and (heat[c] == heat[c].max()).sum() >= 3
        elif kind == "few":
            assert fill[c] >= 1 and len(real) >= 2 and heat[c].size < max_det
        else:
            assert rows.shape[:2] == (1, 1) and rows[0, 0, 0] == heat[0, 0, 0]
    assert max(cand) <= U.REG_CANDIDATES
    if shape[0] > 1:
        assert (heat[1] < 0).all() and (heat[0] >= 0).all()        # both branches of the order map


@pytest.mark.parametrize("name", list(U.PATH_CASES))
def test_path_table_premises(name):
    kind, shape, max_det, want, _ = U.PATH_CASES[name]
    heat, _, _, _, _, _, rows, cand = U.peak_case(name)
    assert cand == [want] * shape[0]
    assert {"bound": want == U.REG_CANDIDATES, "scan": want > U.REG_CANDIDATES, "regs": want < U.REG_CANDIDATES}[kind]
    for c in range(shape[0]):
        values, counts = np.unique(rows[c, :, 0], return_counts=True)
        assert len(values) >= 2 and counts.max() >= 3 and not U.filler_rows(rows)[c]


@pytest.mark.parametrize("name", list(U.SIGMOID_CASES))
def test_sigmoid_table_premises(name):
    shape, _, max_det, _ = U.SIGMOID_CASES[name]
    logits, _, _, _, _, sig, rows, _ = U.peak_case(name)
    assert sig and set(np.unique(rows[:, :, 0])) <= {0.0, 0.5, 1.0}
    heat = U.sigmoid_exact(logits)
    for c in range(shape[0]):
        assert np.unique(rows[c, :, 0], return_counts=True)[1].max() >= 3
        # a plateau of the last row's score crosses a tile border: its pixels reach the selection through different workgroups
        top = heat[c] == rows[c, -1, 0]
        assert (top[:, U.TILE - 1] & top[:, U.TILE]).any() or (top[U.TILE - 1] & top[U.TILE]).any()
    assert name != "s50x90" or len(np.unique(rows[0, :, 0])) == 2


def test_few_cases_have_filler_rows():
    few = [n for n, c in U.TIE_CASES.items() if U.filler_rows(U.peak_case(n)[6]).any()]
    assert "t3" in few and "t40c8" in few


# ------------------------------------------------------------------------------------------------ selectivity
def peaks_variant(heat, ks, max_det, tie_desc=False, ge=False, pad=-np.inf, dr=0, cap_less=0):
    """A copy of peaks_ref (score, x, y columns) with one rule changed per argument; with none it is the reference, built the
    kernel's way: the per-tile cut of max_det - cap_less candidates comes first."""
    ncls, H, W = heat.shape
    rows = np.zeros((ncls, max_det, 3), np.float32)
    rows[:, :, 0] = U.FILLER
    r = max(ks // 2 + dr, 0)
    for c in range(ncls):
        m = U.window_max(heat[c], r, pad)
        alive = ~(m >= heat[c]) if ge else ~(m > heat[c])
        idx = np.flatnonzero(alive.reshape(-1)).astype(np.uint64)
        low = idx if tie_desc else np.uint64(0xFFFFFFFF) - idx
        key = (U.ordered_u32(heat[c].reshape(-1)[idx]).astype(np.uint64) << np.uint64(32)) | low
        tile = (idx // np.uint64(W)) // np.uint64(U.TILE) * np.uint64(1 << 20) + (idx % np.uint64(W)) // np.uint64(U.TILE)
        keep = []
        for t in np.unique(tile):
            of_tile = np.flatnonzero(tile == t)
            keep.append(of_tile[np.argsort(key[of_tile])[::-1][:max_det - cap_less]])
        keep = np.concatenate(keep) if keep else np.zeros(0, np.int64)
        best = idx[keep[np.argsort(key[keep])[::-1][:max_det]]].astype(np.int64)
        rows[c, :len(best), 0] = heat[c].reshape(-1)[best]
        rows[c, :len(best), 1] = best % W
        rows[c, :len(best), 2] = best // W
    return rows


WRONG_PEAKS = {"ties by descending index": dict(tie_desc=True), "suppression with >=": dict(ge=True), "zero padding": dict(pad=0.0),
               "window radius r + 1": dict(dr=1), "window radius r - 1": dict(dr=-1), "per-tile cap max_det - 1": dict(cap_less=1)}


def _case_heat(name):
    heat, _, _, ks, max_det, sig, rows, _ = U.peak_case(name)
    return (U.sigmoid_exact(heat) if sig else heat), ks, max_det, rows[:, :, :3]


@pytest.mark.parametrize("name", list(U.TIE_CASES) + list(U.PATH_CASES) + list(U.SIGMOID_CASES))
def test_the_unchanged_copy_is_the_reference(name):
    """... so a difference below comes from the changed rule alone; and the per-tile cut of max_det never changes the rows."""
    heat, ks, max_det, want = _case_heat(name)
    np.testing.assert_array_equal(peaks_variant(heat, ks, max_det), want)


@pytest.mark.parametrize("wrong", list(WRONG_PEAKS))
def test_every_wrong_peak_rule_shows_on_every_peak_table(wrong):
    """The ties-and-caps table and the selection-path table each hold a case whose expected rows change.  (On the saturated
    sigmoid table every score is 0, 0.5 or 1: a zero padding cannot show there, the other rules are checked as well.)"""
    tables = {"ties": U.TIE_CASES, "paths": U.PATH_CASES}
    if wrong != "zero padding":
        tables["sigmoid"] = U.SIGMOID_CASES
    for table, cases in tables.items():
        differing = []
        for name in cases:
            heat, ks, max_det, want = _case_heat(name)
            if not np.array_equal(peaks_variant(heat, ks, max_det, **WRONG_PEAKS[wrong]), want):
                differing.append(name)
        assert differing, f"'{wrong}' gives the reference's rows on every case of the {table} table"


def decode_variant(rows, cls, min_score, ego_xy, near_px, far_px, min_box, centre_xy, skip_px, ppm, wrong):
    """A copy of det_decode_ref with one rule changed."""
    r = np.asarray(rows, np.float32)[cls]
    max_det = r.shape[0]
    s, w, h = r[:, 0].astype(np.float64), r[:, 3].astype(np.float64), r[:, 4].astype(np.float64)
    to_int = np.rint if wrong == "round" else np.trunc
    xi, yi = to_int(r[:, 1]).astype(np.int64), to_int(r[:, 2]).astype(np.int64)
    X, Y = xi.astype(np.float64), yi.astype(np.float64)
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(((xi - int(ego_xy[0])) ** 2 + (yi - int(ego_xy[1])) ** 2).astype(np.float64))
        far = np.sqrt((X - centre_xy[0]) ** 2 + (Y - centre_xy[1]) ** 2)
        ok = (s >= min_score) if wrong == "score >=" else (s > min_score)
        ok &= (dist >= near_px) if wrong == "near >=" else (dist > near_px)
        ok &= (dist <= far_px) if wrong == "far <=" else (dist < far_px)
        ok &= ~(np.fmax(w, h) <= min_box) if wrong == "box <=" else ~(np.fmax(w, h) < min_box)
        ok &= (far >= skip_px) if wrong == "skip >=" else (far > skip_px)
    j = np.flatnonzero(ok)
    actors = np.zeros(3 * max_det, np.float32)
    actors[0:2 * len(j):2] = ((X[j] - centre_xy[0]) / ppm).astype(np.float32)
    actors[1:2 * len(j):2] = ((Y[j] - centre_xy[1]) / ppm).astype(np.float32)
    actors[2 * max_det:2 * max_det + len(j)] = np.arctan2(r[j, 6].astype(np.float64), r[j, 5].astype(np.float64)).astype(np.float32)
    return actors, len(j)


def test_threshold_rows_are_kept_and_dropped_as_labelled():
    rows = U.decode_rows("threshold")
    kept = [k for _, _, k in U.DECODE_THRESHOLD_ROWS]
    actors, n = U.det_decode_ref(rows, 1, **U.DECODE)
    assert n == sum(kept)
    for j, (label, _, k) in enumerate(U.DECODE_THRESHOLD_ROWS):       # one row at a time: the label is that row's verdict
        one = np.repeat(rows[:, j:j + 1], 2, axis=1)
        assert U.det_decode_ref(one, 1, **U.DECODE)[1] == (2 if k else 0), label
    # with the thresholds ON float32 values the 0.2f score equals its threshold and goes; the 0.4f box equals its threshold and stays
    exact = [k and not label.startswith("score 0.2f") for label, _, k in U.DECODE_THRESHOLD_ROWS]
    assert U.det_decode_ref(rows, 1, **U.DECODE_EXACT)[1] == sum(exact) == sum(kept) - 1
    # the other tables
    assert U.det_decode_ref(U.decode_rows("all64"), 1, **U.DECODE)[1] == 64
    assert U.det_decode_ref(U.decode_rows("none64"), 1, **U.DECODE)[1] == 0
    assert U.det_decode_ref(U.decode_rows("none64"), 0, **U.DECODE)[1] == 64          # the other class would all be kept
    a64 = U.det_decode_ref(U.decode_rows("all64"), 1, **U.DECODE)[0]
    assert len(np.unique(a64[:128].reshape(64, 2), axis=0)) == 64 and len(np.unique(a64[128:])) == 64
    assert U.det_decode_ref(U.decode_rows("threshold", ncls=1, cls=0), 0, **U.DECODE)[1] == sum(kept)


@pytest.mark.parametrize("wrong", ["score >=", "near >=", "far <=", "box <=", "skip >=", "round"])
def test_every_wrong_decode_rule_shows_on_the_threshold_table(wrong):
    rows = U.decode_rows("threshold")
    assert decode_variant(rows, 1, **U.DECODE, wrong=None)[1] == U.det_decode_ref(rows, 1, **U.DECODE)[1]
    differs = False
    for consts in (U.DECODE, U.DECODE_EXACT):
        got, want = decode_variant(rows, 1, **consts, wrong=wrong), U.det_decode_ref(rows, 1, **consts)
        np.testing.assert_array_equal(decode_variant(rows, 1, **consts, wrong=None)[0], want[0])
        differs |= got[1] != want[1] or not np.array_equal(got[0], want[0])
    assert differs


# ------------------------------------------------------------------------------------------------ NaN
def test_a_nan_parts_the_reference_from_the_oracle_in_its_plane_only():
    """The kernel's rule (and the reference's): a NaN is ignored inside every window and the NaN pixel itself survives and sorts
    by its bit pattern - a +NaN first.  torch's max-pool propagates it instead: the whole 7 x 7 neighbourhood survives."""
    heat, clean, (y, x) = U.nan_map()
    ncls, H, W = heat.shape
    z = np.zeros((2, H, W), np.float32)
    rows, _ = U.peaks_ref(heat, z, z, 7, 15)
    rows_clean, _ = U.peaks_ref(clean, z, z, 7, 15)
    parted = []
    for c in range(ncls):
        score, loc = obev.extract_peak(torch.from_numpy(heat[c]))
        live = (score.numpy() > -1e4) | np.isnan(score.numpy())
        mine = (rows[c, :, 2] * W + rows[c, :, 1]).astype(np.int64)
        same = np.array_equal(mine[live], loc.numpy()[live]) and np.array_equal(rows[c, live, 0], score.numpy()[live], equal_nan=True) \
            and (rows[c, ~live, 0] == U.FILLER).all()
        if not same:
            parted.append(c)
        if c != 1:
            np.testing.assert_array_equal(rows[c], rows_clean[c])
    assert parted == [1]
    assert rows[1, 0, 0].view(np.uint32) == U.NAN_BITS and (rows[1, 0, 1], rows[1, 0, 2]) == (x, y)
    # the reference: the NaN's neighbours are suppressed by the plane's maximum beside it as if the NaN were not there ...
    assert rows[1, 1, 0] == clean[1].max() and not np.isnan(rows[1, 1:, 0]).any()
    # ... the oracle keeps them: pixels of the NaN's window that the maximum beside them would have suppressed
    score, loc = obev.extract_peak(torch.from_numpy(heat[1]))
    oracle_only = set(loc.tolist()) - set((rows[1, :, 2] * W + rows[1, :, 1]).astype(int).tolist())
    assert oracle_only and all(abs(l // W - y) <= 3 and abs(l % W - x) <= 3 for l in oracle_only)


# ------------------------------------------------------------------------------------------------ lidar glue
def test_merge_inputs_put_a_point_on_every_face_and_one_inside_it():
    tick, prev = U.merge_inputs(257, seed=1)
    cur, after, inside = U.merge_ticks_ref(tick, prev)
    for i in range(12):
        row = i // 2 + (0 if i % 2 == 0 else 257)
        k, on_face = i // 4, i % 2 == 0
        assert inside[row] == (not on_face), f"probe {i}: coordinate {k}"
        assert np.isnan(cur[row, 0]) == (not on_face)
    assert 12 < inside.sum() < len(cur) - 12
    np.testing.assert_array_equal(after, tick)
    t1, p1 = U.merge_inputs(1, seed=1)
    assert U.merge_ticks_ref(t1, p1)[2].tolist() == [False, True]
