"""lav_eval_resample on the MI355X against its specification (lav_amd.train.eval_common.eval_resample_numpy), every word compared; the seven
evaluation tools with and without --bootstrap; the paired differences; the row table in HBM against the one on the host.  The
specification, the row rule and the interval rule themselves are checked in tests/test_eval_resample_host.py."""
import json

import numpy as np
import pytest
import torch

from lav_amd import ops, synth
from lav_amd.train import eval_common as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CHUNK = 4096          # lav_eval_resample_chunk(): asserted below, so that the shapes here are the ones around it
WIDTHS = (1, 63, 64, 65, 257, 1025)
SEED = 0x9E3779B97F4A7C15


def kernel(rows, B, seed=SEED):
    return ops.eval_resample(torch.from_numpy(rows).to(DEV), B, seed).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ 5. the kernel
@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 65537])
def test_kernel_equals_specification_in_every_word(R):
    """Random int64 rows in +-2^40; every width with 1, 2 and 7 replicates (the largest R with W = 1 only).  Replicate b does not depend
    on B, so the specification is computed once per table, with 7."""
    assert ops.eval_resample_chunk() == CHUNK
    rng = np.random.default_rng(R)
    for W in WIDTHS if R < 65537 else (1,):
        rows = rng.integers(-(1 << 40), 1 << 40, (R, W), dtype=np.int64)
        want = C.eval_resample_numpy(rows, 7, SEED)
        np.testing.assert_array_equal(want[0], rows.sum(axis=0))
        on_device = torch.from_numpy(rows).to(DEV)
        for B in (1, 2, 7):
            got = ops.eval_resample(on_device, B, SEED)
            assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (B + 1, W)
            np.testing.assert_array_equal(got.cpu().numpy(), want[:B + 1], err_msg=f"R {R} W {W} B {B}")
        np.testing.assert_array_equal(on_device.cpu().numpy(), rows)                         # the table is only read


@pytest.mark.parametrize("R,W", [(1000, 65), (CHUNK + 1, 3)])
def test_kernel_carries_between_the_halves_and_sums_zeros(R, W):
    """Values up to 2^62 / R: the sums reach 2^62, so a carry dropped between the 32-bit halves of an add shows.  And a table of zeros."""
    rng = np.random.default_rng(R + W)
    top = (1 << 62) // R
    rows = rng.integers(-top, top, (R, W), dtype=np.int64)
    rows[0] = top - 1
    want = C.eval_resample_numpy(rows, 7, SEED)
    assert np.abs(want).max() > 1 << 45
    got = kernel(rows, 7)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[0], rows.sum(axis=0))
    np.testing.assert_array_equal(kernel(np.full((R, W), -1, np.int64), 3), np.full((4, W), -R, np.int64))
    np.testing.assert_array_equal(kernel(np.zeros((R, W), np.int64), 7), np.zeros((8, W), np.int64))


def test_seed_words_and_no_replicates():
    rows = np.random.default_rng(0).integers(-(1 << 40), 1 << 40, (37, 5), dtype=np.int64)
    for seed in (0, 1, 1 << 32, (1 << 64) - 1, -1):
        np.testing.assert_array_equal(kernel(rows, 3, seed), C.eval_resample_numpy(rows, 3, seed))
    np.testing.assert_array_equal(kernel(rows, 0), rows.sum(axis=0)[None])
    assert not np.array_equal(kernel(rows, 3, 1)[1:], kernel(rows, 3, 1 << 32)[1:])


def test_wrapper_refuses_bad_arguments_before_any_launch():
    rows = torch.zeros((4, 6), dtype=torch.int64, device=DEV)
    for bad in (rows.cpu(), rows.to(torch.int32), rows[0], rows[:, ::2], rows[:0], None):
        with pytest.raises(ValueError):
            ops.eval_resample(bad, 2, 0)
    with pytest.raises(ValueError):
        ops.eval_resample(rows, -1, 0)
    assert tuple(ops.eval_resample(rows, 2, 0).shape) == (3, 6)


# ------------------------------------------------------------------------------------------------------------ 6. and 7. the tools
def _cfg():
    from lav_amd.train.run import load_config
    return load_config(None, seed=2021)


def _tools():
    """name -> (main(argv), extra argv, unit, row_units of 16 units in blocks of 4, summary(acc) as the tool's line makes it, contrasts)"""
    from lav_amd.train import evaluate, evaluate_bev, evaluate_camera, evaluate_det, evaluate_distill, evaluate_drive
    from lav_amd.train.brake import BRA_LABELS
    cfg = _cfg()
    T, small = cfg.num_plan, ["--max-points", "20000"]
    cam, k_seg, k_bra = evaluate_camera, len(cfg.seg_channels) + 1, len(BRA_LABELS) + 1
    det_lay = evaluate_det.det_layout(evaluate_det.HEADS)
    return dict(
        eval_full_v2=(evaluate.main, small, "frames", [4, 4, 4, 4], lambda acc: evaluate.summarise(acc, T), ()),
        eval_seg=(lambda argv: cam.main("seg", argv), [], "images", [6, 6, 4],             # (a call is three images: 0 3 | 6 9 | 12 15)
                  lambda acc: cam.summarise_seg(cam.SEG.view(acc, "seg"), k_seg), ()),
        eval_bra_v2=(lambda argv: cam.main("bra", argv), [], "frames", [4, 4, 4, 4],
                     lambda acc: dict(threshold=0.1, brake=cam.summarise_scores(cam.BRA.view(acc, cam.SCORES)),
                                      wide=cam.summarise_seg(cam.BRA.view(acc, "wide"), k_bra), tele=cam.summarise_seg(cam.BRA.view(acc, "tele"), k_bra)), ()),
        eval_bev_v2=(evaluate_bev.main, [], "frames", [8, 8], lambda acc: evaluate_bev.summarise(acc, T), ()),
        eval_drive_v2=(evaluate_drive.main, small, "frames", [4, 4, 4, 4], lambda acc: evaluate_drive.summarise(acc, T), ()),
        eval_distill_v2=(evaluate_distill.main, small, "frames", [8, 8], lambda acc: evaluate_distill.summarise(acc, T), (("student", "teacher"),)),
        eval_det_v2=(evaluate_det.main, small + ["--heads", "both"], "frames", [4, 4, 4, 4],
                     lambda acc: {h: evaluate_det.summarise(acc[det_lay.sections[h]]) for h in evaluate_det.HEADS}, (("dense", "peaks"),)))


def _leaves(tree, path=()):
    """{path: leaf} of a summary, the path's steps as strings."""
    if isinstance(tree, dict):
        return {p: v for k, sub in tree.items() for p, v in _leaves(sub, path + (str(k),)).items()}
    if isinstance(tree, list):
        return {p: v for i, sub in enumerate(tree) for p, v in _leaves(sub, path + (str(i),)).items()}
    return {path: tree}


def _entries(tree, path=()):
    """{path: entry} of an interval tree; an entry is None or [lo, hi(, n)]."""
    if tree is None or (isinstance(tree, list) and tree and isinstance(tree[0], (int, float))):
        return {path: tree}
    items = tree.items() if isinstance(tree, dict) else enumerate(tree)
    return {p: e for k, sub in items for p, e in _entries(sub, path + (str(k),)).items()}


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _expected(point, reps, B, level, minus=None):
    """The interval rule applied leaf by leaf: {path: entry} for the float-or-None leaves of `point` (those `minus` has too)."""
    js = lambda t: json.loads(json.dumps(t))
    point, reps = _leaves(js(point)), [_leaves(js(r)) for r in reps]
    paths = [p for p, v in point.items() if v is None or isinstance(v, float)]
    if minus is not None:
        other, others = _leaves(js(minus[0])), [_leaves(js(r)) for r in minus[1]]
        paths = [p for p in paths if p in other and (other[p] is None or isinstance(other[p], float))]
    out = {}
    for p in paths:
        vals = []
        for b in range(len(reps)):
            v = reps[b].get(p)
            w = others[b].get(p) if minus is not None else 0.0
            if _number(v) and _number(w):
                vals.append(v - w if minus is not None else v)
        out[p] = C.interval(vals, B, level)
    return out


@pytest.mark.parametrize("name", ["eval_full_v2", "eval_seg", "eval_bra_v2", "eval_bev_v2", "eval_drive_v2", "eval_distill_v2", "eval_det_v2"])
def test_tool_with_bootstrap_keeps_its_line_and_adds_intervals(name, tmp_path, capsys):
    """main(argv) on 16 synthetic units, plain and with --bootstrap 16 --block 4 --rows-out: every old key but the rate is equal; the
    table's column sums are the counters; row_units follows the row rule; resample.ci (and the tool's contrasts) are what the interval rule
    gives on eval_resample_numpy's replicates of the table through the tool's summarise."""
    main, extra, unit, row_units, summary_of, contrasts = _tools()[name]
    base = ["--synthetic", "--frames", "16", "--precision", "f16x3"] + extra
    B, rows_out = 16, tmp_path / "rows.npz"
    plain = main(base)
    boot = main(base + ["--bootstrap", str(B), "--block", "4", "--rows-out", str(rows_out)])
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(plain) == len(boot) == 1 and len(printed) == 2
    plain, boot = plain[0], boot[0]
    assert printed[1] == json.loads(json.dumps(boot)) and "resample" not in printed[0]
    assert list(boot) == list(plain) + ["resample"]
    for key in plain:
        if key != f"{unit}_per_s":
            assert boot[key] == plain[key], key
    saved = np.load(rows_out)
    table, words = saved["table"], int(saved["words"])
    assert sorted(saved.files) == ["block", "row_units", "table", "words"] and int(saved["block"]) == 4
    assert saved["row_units"].tolist() == row_units and table.shape == (len(row_units), words) and table.dtype == np.int64
    assert (table != 0).any(axis=1).all()                                                    # no row is empty
    # (the named counters, flattened, are the accumulator: sections and fields in the layout's order, each row-major)
    np.testing.assert_array_equal(np.array(list(_leaves(boot["counters"]).values()), np.int64), table.sum(axis=0))
    r = boot["resample"]
    assert {k: r[k] for k in ("replicates", "block", "blocks", "units_per_block", "seed", "level")} == dict(
        replicates=B, block=4, blocks=len(row_units), units_per_block=[min(row_units), max(row_units)], seed=2021, level=0.95)
    reps = C.eval_resample_numpy(table, B, 2021)
    assert json.loads(json.dumps(summary_of(reps[0]))) == json.loads(json.dumps(boot["summary"]))
    summaries = [summary_of(reps[b]) for b in range(1, B + 1)]
    want = _expected(boot["summary"], summaries, B, 0.95)
    got = _entries(json.loads(json.dumps(r["ci"])))
    assert want and got == want
    assert any(e is not None and e[0] < e[1] for e in got.values()), "no interval has a width: the replicates are all the same"
    assert set(r) - {"replicates", "block", "blocks", "units_per_block", "seed", "level", "ci"} == ({"contrasts"} if contrasts else set())
    for a, b in contrasts:
        want = _expected(boot["summary"][a], [s[a] for s in summaries], B, 0.95, minus=(boot["summary"][b], [s[b] for s in summaries]))
        assert want and _entries(json.loads(json.dumps(r["contrasts"][f"{a} − {b}"]))) == want


def test_precision_all_pairs_every_later_line_with_the_first(tmp_path):
    """eval_bev_v2 --precision all --bootstrap: the first line has no `vs`, every later one the paired difference to it, recomputed here
    from the two tables of --rows-out."""
    from lav_amd.train import evaluate_bev
    rows_out, B = tmp_path / "rows.npz", 8
    lines = evaluate_bev.main(["--synthetic", "--frames", "16", "--precision", "all", "--bootstrap", str(B), "--block", "4", "--rows-out", str(rows_out)])
    assert len(lines) >= 2 and "vs" not in lines[0]["resample"]
    saved = np.load(rows_out)
    assert saved["row_units"].tolist() == [8, 8]
    T = _cfg().num_plan
    summaries = lambda table: [evaluate_bev.summarise(rep, T) for rep in C.eval_resample_numpy(table, B, 2021)[1:]]
    first = summaries(saved["table"])
    for line in lines[1:]:
        vs = line["resample"]["vs"]
        assert vs["precision"] == lines[0]["precision"] != line["precision"]
        np.testing.assert_array_equal(saved["row_units_" + line["precision"]], saved["row_units"])
        want = _expected(line["summary"], summaries(saved["table_" + line["precision"]]), B, 0.95, minus=(lines[0]["summary"], first))
        assert want and _entries(json.loads(json.dumps(vs["diff"]))) == want


# ------------------------------------------------------------------------------------------------------------ 8. device table == host table
def test_row_table_in_hbm_equals_the_one_on_the_host():
    """One BevEvaluator with its table in HBM (the kernels add into its rows) and one with it on the host (the specification does), in
    resample mode over the same 8 synthetic frames, two per forward, blocks of 4: identical tables, and identical replicates."""
    import lav_amd
    from lav_amd.train import evaluate_bev as E
    from lav_amd.train.synthetic import synthetic_bev_batch
    from tests.util import Y_OFF
    bp = lav_amd.BEVPlanner(pixels_per_meter=4, crop_size=96, feature_x_jitter=1.5, feature_angle_jitter=20, x_offset=0, y_offset=Y_OFF,
                            num_cmds=6, num_plan=20, num_plan_iter=5, num_frame_stack=2)
    bp.load_state_dict(synth.seeded_state_dict(bp, prefix="uni.bev_planner."))
    bp = bp.eval().to(DEV)
    batches = [synthetic_bev_batch(5, seed=5), synthetic_bev_batch(3, seed=6)]
    on_gpu, on_host, plain = E.BevEvaluator(bp, frames_per_forward=2), E.BevEvaluator(bp, device="cpu", frames_per_forward=2), E.BevEvaluator(bp, frames_per_forward=2)
    for ev in (on_gpu, on_host):
        ev.resample(4, 8)
    assert on_gpu.run(batches) == on_host.run(batches) == plain.run(batches) == 8
    (gpu_table, gpu_units), (host_table, host_units) = on_gpu.row_table(), on_host.row_table()
    assert gpu_table.is_cuda and not host_table.is_cuda and on_gpu.acc.is_cuda
    assert gpu_units.tolist() == host_units.tolist() == [4, 4]
    np.testing.assert_array_equal(gpu_table.cpu().numpy(), host_table.numpy())
    assert (host_table.numpy() != 0).any(axis=1).all()
    np.testing.assert_array_equal(on_gpu.counters(), plain.counters())
    np.testing.assert_array_equal(on_gpu.replicates(5, 3), on_host.replicates(5, 3))
    np.testing.assert_array_equal(on_gpu.replicates(5, 3)[0], plain.counters())
