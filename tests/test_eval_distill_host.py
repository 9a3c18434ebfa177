"""CPU checks of the student-beside-teacher evaluation (lav_amd.train.evaluate_distill): the specification against counters derived by
hand on built scenes, the accumulator's length through the C ABI, the layouts' round trip, the summary and the command line's parser.
The kernel is held to this specification in tests/test_gpu_eval_distill.py."""
import ctypes as C
import json

import numpy as np
import pytest

from lav_amd.train import evaluate_bev as EB
from lav_amd.train import evaluate_distill as E
from tests import eval_distill_util as U

Q = 1 << 20
T, S = U.T, U.I + 1
LAY = E.PairLayout(U.I)
STUDENT, TEACHER, TIE = 0, 1, 2


def run(s, acc=None):
    acc = E.PairLayout(s["s_ego_plan"].shape[1]).zeros() if acc is None else acc
    return E.eval_distill_numpy(acc, *U.positional(s))


def expect(lay=LAY, **fields):
    """An accumulator with the named slices set ({index tuple within the slice: value}, or a value for all of it), everything else 0."""
    acc = lay.zeros()
    for name, items in fields.items():
        view = lay.view(acc, name)
        if isinstance(items, dict):
            for at, v in items.items():
                view[at] = v
        else:
            view[...] = items
    return acc


def every(value, but=None, stages=S):
    """{(stage, mode): value} for every stage and mode, then the exceptions."""
    out = {(s, m): value for s in range(stages) for m in range(6)}
    out.update(but or {})
    return out


def test_layouts_are_114_plus_38_stages_and_the_library_agrees():
    from lav_amd import ops
    for iters in (1, 5, 8):
        pair, whole = E.PairLayout(iters), E.DistillLayout(iters)
        assert len(pair) == 114 + 38 * (iters + 1) == ops.eval_distill_words(iters)
        assert len(whole) == 2 * ops.eval_plans_words(iters) + ops.eval_distill_words(iters)
        assert E.PairLayout.of(pair.zeros()).iters == iters == E.DistillLayout.of(whole.zeros()).iters
        assert list(whole.sections) == ["teacher", "student", "pair"] and whole.sections["pair"] == slice(len(whole) - len(pair), len(whole))
        assert [whole.kind(k) for k in whole.sections] == ["plan", "plan", "pair"]
        assert list(whole.fields(whole.zeros(), "student")) == list(EB.PlanLayout(iters).fields)
        assert list(whole.fields(whole.zeros(), "pair")) == list(pair.fields) and pair.fields["oth_cmd_gap"][0].stop == len(pair)
        assert pair.view(pair.zeros(), "ego_closer").shape == (iters + 1, 6, 3)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            E.PairLayout(bad)
        with pytest.raises(ValueError):
            E.DistillLayout(bad)
        with pytest.raises(ValueError):
            ops.eval_distill_words(bad)
    for words in (114, 114 + 38, 114 + 38 * 10, 300):
        with pytest.raises(ValueError):
            E.PairLayout.of(np.zeros(words, np.int64))


def test_named_and_unnamed_round_trip():
    rng = np.random.default_rng(3)
    for lay in (E.PairLayout(5), E.DistillLayout(1), E.DistillLayout(8)):
        acc = rng.integers(0, 1 << 40, len(lay)).astype(np.int64)
        named = json.loads(json.dumps(lay.named(acc)))
        np.testing.assert_array_equal(lay.unnamed(named), acc)
    assert set(E.DistillLayout(5).named(E.DistillLayout(5).zeros())) == {"teacher", "student", "pair"}


def test_identical_arms_have_no_gap_and_tie_everywhere():
    acc = run(U.scene_identical())
    want = expect(frames=3, ego_gap=every((3, 0, 0)), ego_closer={(s, 2, TIE): 3 for s in range(S)}, cmd_agree={(2, 2): 3},
                  cmd_gap={m: (3, 0) for m in range(6)}, others=2, oth_closer={TIE: 2}, oth_closer_top={TIE: 2}, oth_same_min=2,
                  oth_top_agree={(0, 0): 2})
    np.testing.assert_array_equal(acc, want)
    # both agreement matrices are on their diagonal
    for name in ("cmd_agree", "oth_top_agree"):
        m = LAY.view(acc, name)
        assert m.sum() == np.trace(m) > 0


def test_closer_by_one_quantum():
    acc = run(U.scene_one_quantum())
    gaps = every((2, 0, 0), {(0, 2): (2, 2, 2)})
    gaps.update({(s, 2): (2, 1, 1) for s in range(1, S)})
    closer = {(0, 2, STUDENT): 1, (0, 2, TEACHER): 1}
    closer.update({(s, 2, k): 1 for s in range(1, S) for k in (STUDENT, TIE)})
    want = expect(frames=2, ego_gap=gaps, ego_closer=closer, cmd_agree={(2, 2): 2}, cmd_gap={m: (2, 0) for m in range(6)}, others=1,
                  oth_gap={4: (2 * T, 2)}, oth_closer={STUDENT: 1}, oth_closer_top={TIE: 1}, oth_top_agree={(0, 0): 1})
    np.testing.assert_array_equal(acc, want)


def test_a_nonfinite_value_moves_what_reads_it_only():
    acc = run(U.scene_nonfinite())
    closer = {(s, 3, TIE): 2 for s in range(S)}
    closer[(2, 3, TIE)] = 1
    want = expect(frames=2, ego_gap=every((2, 0, 0), {(2, 3): (1, 0, 0), (0, 0): (1, 0, 0)}), ego_gap_nonfinite={0: 1, 2: 1}, ego_closer=closer,
                  ego_unjudged={2: 1}, cmd_agree={(3, 3): 2}, cmd_gap={m: (2, 0) for m in range(6)}, others=1, oth_nonfinite=2,
                  oth_closer={TIE: 1}, oth_closer_top={TIE: 1}, oth_same_min=1, oth_top_agree={(0, 0): 1})
    np.testing.assert_array_equal(acc, want)


def test_a_nan_score_counts_as_the_maximum_and_has_no_gap():
    acc = run(U.scene_nan_scores())
    closer = {(s, c, TIE): 1 for s in range(S) for c in (1, 2)}
    gaps = {m: (2, 0) for m in range(6)}
    gaps[1] = gaps[4] = (1, 0)
    want = expect(frames=2, ego_gap=every((2, 0, 0)), ego_closer=closer, cmd_agree={(2, 4): 1, (1, 1): 1}, cmd_gap=gaps, cmd_nonfinite=2)
    np.testing.assert_array_equal(acc, want)


def test_a_command_outside_0_to_5_touches_frames_and_bad_cmd_only():
    acc = run(U.scene_bad_cmds())
    want = expect(frames=3, bad_cmd=2, ego_gap=every((1, 0, 0)), ego_closer={(s, 0, TIE): 1 for s in range(S)}, cmd_agree={(0, 0): 1},
                  cmd_gap={m: (1, 0) for m in range(6)})
    np.testing.assert_array_equal(acc, want)


def test_first_minimum_and_first_maximum_ties():
    acc = run(U.scene_ties())
    score = {m: (1, 0) for m in range(6)}
    score[1] = score[5] = (1, Q // 2)
    want = expect(frames=1, ego_gap=every((1, 0, 0)), ego_closer={(s, 2, TIE): 1 for s in range(S)}, cmd_agree={(1, 3): 1}, cmd_gap=score, others=2,
                  oth_gap={1: (6 * T, 6), 2: (4 * T, 4), 4: (6 * T, 6)}, oth_closer={STUDENT: 1, TIE: 1}, oth_closer_top={STUDENT: 1, TIE: 1},
                  oth_same_min=0, oth_top_agree={(0, 0): 1, (2, 2): 1})
    np.testing.assert_array_equal(acc, want)


def test_one_waypoint_and_no_forecasts_as_none_or_empty():
    s = U.scene_single_waypoint()
    acc = run(s)
    want = expect(frames=1, ego_gap=every((1, 0, 0), {(0, 0): (1, 2, 2)}), ego_closer={(st, 2, TIE): 1 for st in range(S)}, cmd_agree={(2, 2): 1},
                  cmd_gap={m: (1, 0) for m in range(6)})
    np.testing.assert_array_equal(acc, want)
    empty = dict(s, s_other_cast=np.zeros((0, 6, 1, 2), np.float32), t_other_cast=np.zeros((0, 6, 1, 2), np.float32),
                 s_other_cmds=np.zeros((0, 6), np.float32), t_other_cmds=np.zeros((0, 6), np.float32), other_locs=np.zeros((0, 1, 2), np.float32))
    np.testing.assert_array_equal(run(empty), want)


def test_an_absurd_score_gap_is_nonfinite_and_cannot_overflow():
    """Scores 3e38 apart would be 3e44 quanta: the gap is non-finite by the rule of the distances (not below 2^32)."""
    s = U.blank(1, 1)
    s["s_ego_cmds"][0, 0], s["t_ego_cmds"][0, 0] = 3e38, -3e38
    s["s_other_cmds"][0, 5] = 2.0 ** 33
    acc = run(s)
    assert LAY.view(acc, "cmd_nonfinite").item() == 1 and LAY.view(acc, "cmd_gap")[0].tolist() == [0, 0]
    assert LAY.view(acc, "oth_nonfinite").item() == 1 and LAY.view(acc, "others").item() == 0


def test_split_batches_add_up_and_random_batches_hold_every_kind_of_case():
    acc = LAY.zeros()
    for seed in range(8):
        s = U.random_batch(seed)
        run(s, acc)
    v = lambda n: LAY.view(acc, n)
    assert v("bad_cmd").item() > 0 and v("ego_gap_nonfinite").sum() > 0 and v("ego_unjudged").sum() > 0 and v("oth_nonfinite").item() > 0
    assert v("cmd_nonfinite").item() > 0 and (v("ego_closer").sum(axis=(0, 1)) > 0).all() and (v("oth_closer") > 0).all()
    assert 0 < v("oth_same_min").item() < v("others").item() and 0 < np.trace(v("cmd_agree")) < v("cmd_agree").sum()
    assert (acc >= 0).all()
    a, b = U.random_batch(1, Bn=4, K=3), U.random_batch(2, Bn=2, K=9)
    np.testing.assert_array_equal(run(b, run(a)), run(U.concat(a, b)))
    for s in range(S):
        assert v("ego_closer")[s].sum() + v("ego_unjudged")[s] + v("bad_cmd").item() == v("frames").item()


def test_summary_of_nothing_has_no_nan():
    for iters in (1, 5, 8):
        m = E.summarise(E.DistillLayout(iters).zeros())
        text = json.dumps(m)
        assert "NaN" not in text and "Infinity" not in text and m["frames"] == 0
        assert len(m["pair"]["stages"]) == len(m["stages"]) == iters + 1
        st = m["pair"]["stages"][0]
        assert st["ade"] is None and st["closer"]["student"] is None and st["per_mode"][3]["fde"] is None and st["teacher"]["ade"] is None
        assert m["pair"]["command"]["agreement"] is None and m["pair"]["others"]["same_min"] is None and m["pair"]["others"]["closer_min"]["tie"] is None


def test_summary_reports_gaps_and_shares():
    lay = E.DistillLayout(U.I)
    acc = lay.zeros()
    s = U.scene_one_quantum()
    s["s_ego_cast"][..., 0] += 2.0                          # the student's cast 2 m off in every mode of both frames
    E.eval_distill_numpy(lay.view(acc, "pair"), *U.positional(s))
    EB.eval_plans_numpy(lay.view(acc, "student"), *U.student_of(s))
    m = E.summarise(acc, T)
    assert m["frames"] == 2 and m["student"]["frames"] == 2 and m["teacher"]["frames"] == 0
    cast = m["pair"]["stages"][0]
    assert abs(cast["ade"] - 2.0) < 1e-5 and cast["items"] == 12 and cast["closer"]["teacher"] == 1.0 and cast["closer"]["judged"] == 2
    assert abs(cast["student"]["ade"] - 2.0) < 1e-5 and cast["teacher"]["ade"] is None
    plan = m["pair"]["stages"][1]["closer"]
    assert plan["student"] == plan["tie"] == 0.5 and plan["per_cmd"][2]["judged"] == 2 and plan["per_cmd"][0]["student"] is None
    o = m["pair"]["others"]
    assert o["scored"] == 1 and o["closer_min"]["student"] == 1.0 and o["closer_top"]["tie"] == 1.0 and o["same_min"] == 0.0
    assert o["top_agreement"] == 1.0 and o["mean_score_gap"] == 0.0 and o["gap_ade_per_mode"][4] == 2 / Q and o["gap_ade_per_mode"][0] == 0.0


def test_bad_arguments_raise():
    s = U.blank(2, 1)
    with pytest.raises(ValueError):
        E.eval_distill_numpy(LAY.zeros()[:-1], *U.positional(s))
    with pytest.raises(ValueError):
        E.eval_distill_numpy(LAY.zeros().astype(np.int32), *U.positional(s))
    with pytest.raises(ValueError):
        E.eval_distill_numpy(LAY.zeros(), *U.positional(dict(s, cmds=s["cmds"][:1])))
    with pytest.raises(ValueError):
        E.eval_distill_numpy(LAY.zeros(), *U.positional(dict(s, t_ego_cast=s["t_ego_cast"][:, :, :-1])))
    with pytest.raises(ValueError):
        E.eval_distill_numpy(LAY.zeros(), *U.positional(dict(s, t_other_cast=None)))
    with pytest.raises(ValueError):
        E.eval_distill_numpy(LAY.zeros(), *U.positional(dict(s, other_locs=s["other_locs"][:, :-1])))


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    """lav_eval_distill checks null, range and alignment first: no device is needed to be refused (the pointers are never read)."""
    from lav_amd import _lib
    lib = _lib.load()
    p = lambda off=0: C.c_void_p(4096 + off)

    def call(frame=None, batch=2, iters=5, num_plan=20, others=(None,) * 5, num_others=0, acc=p()):
        frame = frame or [p()] * 8
        return lib.lav_eval_distill(*frame, batch, iters, num_plan, *others, num_others, acc, None)

    for kw, word in ((dict(frame=[p()] * 3 + [None] + [p()] * 4), b"null"), (dict(acc=None), b"null"), (dict(batch=0), b"frames"),
                     (dict(iters=9), b"iterations"), (dict(iters=0), b"iterations"), (dict(num_plan=65), b"waypoints"), (dict(num_plan=0), b"waypoints"),
                     (dict(num_others=3), b"forecasts"), (dict(num_others=-1), b"forecasts"), (dict(others=[p()] * 4 + [None], num_others=2), b"forecasts"),
                     (dict(frame=[p()] * 6 + [p(2)] + [p()]), b"aligned"), (dict(others=[p()] * 3 + [p(1), p()], num_others=2), b"aligned"),
                     (dict(acc=p(4)), b"aligned")):
        assert call(**kw) != 0, kw
        assert word in lib.lav_last_error(), (kw, lib.lav_last_error())


def test_command_line_parser_builds():
    from lav_amd.train.eval_common import parser
    ap = parser(E.TOOL)
    args = ap.parse_args(["--synthetic", "--frames", "4", "--precision", "all", "--others", "all", "--bev", "bev_7.th", "--lidar", "l.th", "--uniplanner", "u.th"])
    assert (args.frames, args.precision, args.others, args.bev, args.lidar, args.uniplanner) == (4, "all", "all", "bev_7.th", "l.th", "u.th")
    args = ap.parse_args(["--config-path", "c.yaml", "--data-dir", "d"])
    assert args.bev is None and args.others == "ahead" and args.precision is None and args.batch_size == 8
    with pytest.raises(SystemExit):
        ap.parse_args(["--others", "behind"])
    assert "ground-truth poses" in E.NOTE and "eval_full_v2.py" in E.NOTE and "ground-truth poses" in ap.format_help()
