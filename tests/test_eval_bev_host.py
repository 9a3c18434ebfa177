"""CPU checks of the teacher's evaluation (lav_amd.train.evaluate_bev): the specification against counters derived by hand, the
accumulator's length through the C ABI, the summary, independence of batch split and frame order, and sample_others' random draws after
its split into a selection half and a random half.  The kernel is held to this specification in tests/test_gpu_eval_bev.py."""
import json

import numpy as np
import pytest
import torch

from lav_amd.train import evaluate_bev as E
from tests import eval_bev_util as U

Q = 1 << 20
LAY = E.PlanLayout(U.I)


def run(s, acc=None):
    acc = E.PlanLayout(s["ego_plan"].shape[1]).zeros() if acc is None else acc
    return E.eval_plans_numpy(acc, *U.positional(s))


def expect(lay=LAY, **fields):
    """An accumulator with the named slices set ({index tuple within the slice: value}, or a scalar), everything else 0."""
    acc = lay.zeros()
    for name, items in fields.items():
        view = lay.view(acc, name)
        if isinstance(items, dict):
            for at, v in items.items():
                view[at] = v
        else:
            view[...] = items
    return acc


def test_layout_is_57_plus_37_stages_and_the_library_agrees():
    from lav_amd import ops
    for iters in range(1, 9):
        lay = E.PlanLayout(iters)
        assert len(lay) == 57 + 37 * (iters + 1) == ops.eval_plans_words(iters)
        assert E.PlanLayout.of(lay.zeros()).iters == iters
        assert list(lay.fields)[:3] == ["frames", "bad_cmd", "plan"] and lay.fields["oth_top_is_min"][0].stop == len(lay)
        assert lay.view(lay.zeros(), "plan").shape == (2, iters + 1, 6, 3) and set(lay.named(lay.zeros())) == set(lay.fields)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            E.PlanLayout(bad)
        with pytest.raises(ValueError):
            ops.eval_plans_words(bad)
    for words in (57, 57 + 37, 57 + 37 * 10, 200):
        with pytest.raises(ValueError):
            E.PlanLayout.of(np.zeros(words, np.int64))


def test_a_3_4_5_offset_held_for_T_steps():
    acc = run(U.scene_345())
    stage = (1, 5 * Q * U.T, 5 * Q)
    want = expect(frames=1, plan={(0, s, 2): stage for s in range(U.I + 1)}, cmd_conf={(2, 2): 1}, others=1,
                  oth=(5 * Q * U.T, 5 * Q * U.T, 5 * Q, 5 * Q), oth_min_mode={0: 1}, oth_top_mode={0: 1}, oth_top_is_min=1)
    np.testing.assert_array_equal(acc, want)
    m = E.summarise(acc, U.T)
    assert all(st["ade"] == 5.0 and st["fde"] == 5.0 for st in m["plan"]["all"]) and m["others"]["min_ade"] == 5.0 == m["others"]["top_fde"]
    assert [st["gain"] for st in m["plan"]["all"]] == [None] + [0.0] * U.I


def test_ties_round_to_even():
    """1.5 and 2.5 quanta are both 2; the modes 0.5 .. 5.5 quanta off are 0, 2, 2, 4, 4, 6."""
    acc = run(U.scene_ties())
    plan = LAY.view(acc, "plan")
    assert plan[0, 0, 2].tolist() == [1, 2 * U.T, 2]
    assert all(plan[0, s, 2].tolist() == [1, 2 * U.T, 2] for s in range(1, U.I + 1))
    assert LAY.view(acc, "oth").tolist() == [0, 0, 0, 0] and LAY.view(acc, "oth_min_mode").tolist() == [1, 0, 0, 0, 0, 0]
    s = U.scene_ties()
    s["other_cast"][0, 0] = s["other_cast"][0, 5]           # now the nearest mode is 1 (2 quanta a step), the top mode 0 (6 a step)
    assert LAY.view(run(s), "oth").tolist() == [2 * U.T, 6 * U.T, 6, 2]


def test_identical_modes_and_tied_scores_give_the_first():
    acc = run(U.scene_identical_modes())
    want = expect(frames=1, plan={(0, s, 2): (1, 0, 0) for s in range(U.I + 1)}, cmd_conf={(2, 2): 1}, others=2,
                  oth=(Q // 4 * U.T + Q // 2 * U.T, Q // 4 * U.T + Q * U.T, Q // 4 + Q, Q // 4 + Q // 2),
                  oth_min_mode={1: 1, 4: 1}, oth_top_mode={3: 1, 2: 1}, oth_top_is_min=0)
    np.testing.assert_array_equal(acc, want)


def test_a_nan_score_counts_as_the_maximum():
    acc = run(U.scene_nan_scores())
    want = expect(frames=2, plan={(0, s, c): (1, 0, 0) for s in range(U.I + 1) for c in (1, 2)}, cmd_conf={(2, 4): 1, (1, 1): 1}, others=1,
                  oth_min_mode={0: 1}, oth_top_mode={3: 1})
    np.testing.assert_array_equal(acc, want)
    assert E.summarise(acc, U.T)["command"]["accuracy"] == 0.5


def test_a_nonfinite_stage_moves_that_stage_only():
    acc = run(U.scene_nan_stage())
    plan = {(0, s, 3): (1, 0, 0) for s in range(U.I + 1) if s != 2}
    plan.update({(1, s, 3): (1, 0, 0) for s in range(1, U.I + 1)})
    want = expect(frames=2, plan=plan, plan_nonfinite={0: 1, 2: 1}, cmd_conf={(3, 3): 2}, others=1, oth_nonfinite=1, oth_min_mode={0: 1},
                  oth_top_mode={0: 1}, oth_top_is_min=1)
    np.testing.assert_array_equal(acc, want)
    m = E.summarise(acc, U.T)
    assert m["plan"]["nonfinite"] == [1, 0, 1, 0, 0, 0] and m["plan"]["braking"][0]["ade"] is None and m["plan"]["braking"][1]["frames"] == 1


def test_a_command_outside_0_to_5_touches_frames_and_bad_cmd_only():
    acc = run(U.scene_bad_cmds())
    want = expect(frames=3, bad_cmd=2, plan={(0, s, 0): (1, 0, 0) for s in range(U.I + 1)}, cmd_conf={(0, 0): 1})
    np.testing.assert_array_equal(acc, want)
    only_bad = U.take(U.scene_bad_cmds(), [0, 1], [])
    np.testing.assert_array_equal(run(only_bad), expect(frames=2, bad_cmd=2))


def test_summary_of_nothing_has_no_nan():
    for iters in (1, 5, 8):
        m = E.summarise(E.PlanLayout(iters).zeros())
        text = json.dumps(m)
        assert "NaN" not in text and "Infinity" not in text and m["frames"] == 0
        assert m["plan"]["all"][0]["ade"] is None and m["command"]["accuracy"] is None and m["others"]["min_ade"] is None
        assert len(m["plan"]["all"]) == len(m["stages"]) == iters + 1 and m["others"]["top_is_min"] is None


def test_summary_reports_refinement_gain_and_mode_use():
    s = U.blank(2, 2)
    s["bras"][1] = 1
    s["ego_cast"][..., 0] += 2.0                            # the cast 2 m off, the plan stages 1 m, 0.5 m, then on target
    s["ego_plan"][:, 0, ..., 0] += 1.0
    s["ego_plan"][:, 1, ..., 0] += 0.5
    s["other_cast"][:, 0, :, 1] += 1.0                      # the top mode (0) 1 m off, the others on target: min mode 1
    m = E.summarise(run(s), U.T)
    assert [st["ade"] for st in m["plan"]["all"]] == [2.0, 1.0, 0.5, 0.0, 0.0, 0.0]
    assert [st["gain"] for st in m["plan"]["all"]] == [None, -1.0, -0.5, -0.5, 0.0, 0.0]
    assert m["plan"]["driving"][0]["frames"] == m["plan"]["braking"][0]["frames"] == 1 and m["plan"]["all"][0]["per_cmd"][2]["fde"] == 2.0
    assert m["frames_per_cmd"] == [0, 0, 2, 0, 0, 0] and m["command"]["per_cmd"][2] == 1.0 and m["command"]["per_cmd"][0] is None
    o = m["others"]
    assert (o["scored"], o["min_ade"], o["top_ade"], o["top_fde"], o["min_fde"], o["top_is_min"]) == (2, 0.0, 1.0, 1.0, 0.0, 0.0)
    assert o["min_mode"] == [0, 2, 0, 0, 0, 0] and o["top_mode"] == [2, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_split_and_permuted_batches_give_the_same_accumulator(seed):
    s = U.random_batch(seed, B=9, K=11)
    whole = run(s)
    assert LAY.view(whole, "frames").item() == 9
    halves = run(U.take(s, range(4, 9), range(0, 3)), run(U.take(s, range(0, 4), range(3, 11))))
    np.testing.assert_array_equal(halves, whole)
    rng = np.random.default_rng(seed)
    np.testing.assert_array_equal(run(U.take(s, rng.permutation(9), rng.permutation(11))), whole)
    no_others = run(U.take(s, range(9), []))
    assert LAY.view(no_others, "others").item() == 0 and np.array_equal(LAY.view(no_others, "plan"), LAY.view(whole, "plan"))


def test_random_batches_hold_every_kind_of_case():
    """What the kernel is compared on (tests/test_gpu_eval_bev.py) exercises every branch of the specification."""
    acc = LAY.zeros()
    for seed in range(8):
        run(U.random_batch(seed), acc)
    v = lambda n: LAY.view(acc, n)
    assert v("bad_cmd").item() > 0 and v("plan_nonfinite").sum() > 0 and v("oth_nonfinite").item() > 0
    assert v("plan")[0].sum() > 0 and v("plan")[1].sum() > 0 and 0 < v("oth_top_is_min").item() < v("others").item()
    assert (acc >= 0).all()


def test_bad_arguments_raise():
    s = U.blank(2, 1)
    with pytest.raises(ValueError):
        E.eval_plans_numpy(LAY.zeros()[:-1], *U.positional(s))
    with pytest.raises(ValueError):
        E.eval_plans_numpy(LAY.zeros().astype(np.int32), *U.positional(s))
    with pytest.raises(ValueError):
        E.eval_plans_numpy(LAY.zeros(), *U.positional(dict(s, cmds=s["cmds"][:1])))
    with pytest.raises(ValueError):
        E.eval_plans_numpy(LAY.zeros(), *U.positional(dict(s, other_locs=s["other_locs"][:, :-1])))


def _planner(max_num_cars):
    import lav_amd
    return lav_amd.BEVPlanner(pixels_per_meter=4, crop_size=96, feature_x_jitter=1.5, feature_angle_jitter=20, num_plan=20, num_plan_iter=5,
                              num_frame_stack=2, max_num_cars=max_num_cars)


def test_sample_others_draws_what_it_drew_before_the_split():
    """sample_others = select_others (no draw) + random_sample + picked_others with ITS jitter: after a seeded call the global generator
    stands where the draws it has always made leave it - one multinomial of `max_num_cars` per over-full row, then rand(K, 2), then
    rand(K) -, and the jitter it applied is those numbers."""
    from lav_amd import planner_common as P
    from lav_amd.train.synthetic import synthetic_bev_batch
    _, ego_locs, _, _, _, locs, oris, typs, _ = synthetic_bev_batch(3, seed=11, num_objs=8)
    ego_locs, locs, oris = ego_locs.float(), locs.float(), oris.float()
    typs[:, 1:] = 1
    locs[:, 1:, :, 1] = ego_locs[:, None, :1, 1] - 1.0 - locs[:, 1:, :, 1].abs()        # everybody a vehicle ahead: every row is over-full
    bp = _planner(max_num_cars=3)
    picked = P.select_others(ego_locs, locs, typs)
    assert picked.dtype == torch.bool and picked.shape == (3, locs.shape[1] - 1) and bool(picked.all())
    assert bool((P.select_others(ego_locs, locs, typs, ahead=False) == (typs[:, 1:] == 1)).all())

    torch.manual_seed(77)
    before = torch.get_rng_state()
    P.select_others(ego_locs, locs, typs)
    assert torch.equal(torch.get_rng_state(), before), "the selection half draws nothing"
    pick, N = P.sample_others(bp, ego_locs, locs, oris, typs)
    after = torch.get_rng_state()

    torch.manual_seed(77)                                   # the same draws, made by hand in the order sample_others has always made them
    kept = torch.zeros_like(picked)
    for i in range(3):
        nz = torch.nonzero(picked[i]).squeeze(1)
        kept[i, nz[torch.multinomial(torch.ones_like(nz).float(), 3)]] = True
    K = int(kept.sum())
    locs_jitter = (torch.rand((K, 2)) * 2 - 1).float() * bp.feature_x_jitter
    locs_jitter[:, 1] = 0
    oris_jitter = (torch.rand((K,)) * 2 - 1).float() * bp.feature_angle_jitter
    assert torch.equal(torch.get_rng_state(), after), "the generator stands where the same draws leave it"
    assert N == locs.shape[1] - 1 and K == 9 and torch.equal(pick["typs"], kept)
    rel_loc0 = (locs[:, 1:, 0] - ego_locs[:, None, 0])[kept]
    rel_ori0 = (oris[:, 1:] - oris[:, :1])[kept]
    assert torch.equal(pick["crop_locs"], rel_loc0 + locs_jitter) and torch.equal(pick["crop_oris"], rel_ori0 + oris_jitter)
    flat = (locs[:, 1:, 1:] - locs[:, 1:, :1])[kept]
    assert torch.equal(pick["other_locs"], P.transform_points(flat - locs_jitter[:, None], -rel_ori0 - oris_jitter))
    where = torch.nonzero(kept)
    assert torch.equal(pick["sample"], where[:, 0].int()) and torch.equal(pick["actor"], where[:, 1].int())
    # nobody qualifies: None, and no draw
    before = torch.get_rng_state()
    none, N0 = P.sample_others(bp, ego_locs, locs, oris, torch.zeros_like(typs))
    assert none is None and N0 == N and torch.equal(torch.get_rng_state(), before)


def test_held_out_bev_frames_have_no_jitter_and_do_not_depend_on_what_was_loaded_before(tmp_path):
    from tests.util import dataset_fixture_config
    cfg = dataset_fixture_config(str(tmp_path), routes=1, frames=24)
    frames = E.held_out_bev_frames(cfg, seed=5)
    assert len(frames) >= 2 and frames.dataset.x_jitter == 0 and frames.dataset.angle_jitter == 0
    first = frames[1]
    torch.rand(7)
    np.random.rand(3)
    frames[0]
    again = frames[1]
    for a, b in zip(first, again):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert np.asarray(first[0]).shape[0] == 9 and np.asarray(first[1]).shape == (21, 2)
