"""CPU checks of the rule-layer evaluation (lav_amd.train.evaluate_drive): the specification against counters derived by hand, the
restated rules against LAVAgent.plan_collide and LAVAgent.pid_control themselves on random scenes, the accumulator's layout through the
C ABI, the summary, and the command line.  The kernel is held to this specification in tests/test_gpu_eval_drive.py."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from lav_amd.train import evaluate_drive as E
from lav_amd.train.eval_common import parser
from tests import eval_drive_util as U

Q = 1 << 20
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(f, acc=None):
    acc = E.DriveLayout(f["kw"]["nbins"]).zeros() if acc is None else acc
    return E.eval_drive_numpy(acc, *U.positional(f), **f["kw"])


def differing(lay, got, want):
    return {k: (g, w) for (k, g), w in zip(lay.named(got).items(), lay.named(want).values()) if g != w}


@pytest.mark.parametrize("name", sorted(U.SCENES))
def test_specification_equals_hand_derived_counters(name):
    f, want = U.SCENES[name]()
    got = run(f)
    assert not differing(E.DriveLayout(f["kw"]["nbins"]), got, want)
    np.testing.assert_array_equal(got, want)


def test_frames_add_up_and_tensors_are_taken():
    """Every built scene with 64 bins into one accumulator, in both orders, as arrays and as tensors."""
    built = [U.SCENES[k]() for k in sorted(U.SCENES)]
    built = [(f, want) for f, want in built if f["kw"]["nbins"] == 64]
    total = sum(want for _, want in built)
    acc = back = tens = None
    for f, _ in built:
        acc = run(f, acc)
    for f, _ in reversed(built):
        back = run(f, back)
        g = dict(f, **{k: torch.from_numpy(v) for k, v in f.items() if isinstance(v, np.ndarray)})
        tens = run(g, tens)
    np.testing.assert_array_equal(acc, total)
    np.testing.assert_array_equal(back, total)
    np.testing.assert_array_equal(tens, total)


def test_no_vehicles_given_as_none_or_as_empty_tensors():
    f, want = U.scene_empty()
    f["other_cast"], f["other_cmds"] = torch.zeros((0, 6, U.T, 2)), torch.zeros((0, 6))
    np.testing.assert_array_equal(run(f), want)


def test_bad_arguments_are_refused():
    f, _ = U.scene_static()
    for changed in (dict(cmd=6), dict(cmd=-1), dict(bra=2), dict(n=5), dict(ego_cast=f["ego_cast"][:-1]), dict(typs=f["typs"][:-1]),
                    dict(other_cmds=f["other_cmds"][:, :5]), dict(ego_plan=f["ego_plan"][:1], ego_cast=f["ego_cast"][:1], ego_locs=f["ego_locs"][:2]),
                    dict(kw=dict(rules=E.DriveRules(aim_point=(4, 4, 4, 3, 6, U.T)), nbins=64)), dict(kw=dict(rules=E.DriveRules(), nbins=0))):
        with pytest.raises(ValueError):
            run(dict(f, **changed))
    with pytest.raises(ValueError):
        E.eval_drive_numpy(np.zeros(5, np.int64), *U.positional(f), **f["kw"])
    for bad in (dict(brake_speed=-0.1), dict(dist_static=float("nan")), dict(behind=float("inf")), dict(aim_point=(4, 4, 4)), dict(aim_point=(4, 4, 4, 3, 6, -1))):
        with pytest.raises(ValueError):
            E.DriveRules(**bad)


# ------------------------------------------------------------------------------------------------------------ the rules against the agent's code
def _agent(rules):
    from lav_amd.agent import PIDController
    from lav_amd.lav_agent import DEFAULT_CONFIG as C
    return types.SimpleNamespace(pixels_per_meter=C["pixels_per_meter"], cmd_thresh=rules.cmd_thresh, brake_speed=rules.brake_speed,
                                 aim_point=list(rules.aim_point), speed_ratio=C["speed_ratio"], clip_delta=C["clip_delta"], max_throttle=C["max_throttle"],
                                 turn_controller=PIDController(K_P=C["turn_KP"], K_I=C["turn_KI"], K_D=C["turn_KD"], n=C["turn_n"]),
                                 speed_controller=PIDController(K_P=C["speed_KP"], K_I=C["speed_KI"], K_D=C["speed_KD"], n=C["speed_n"]))


def _near_a_threshold(f, wp, margin=1e-4):
    """Whether some comparison of the rules on this scene lies within `margin` of its threshold (float64, written out independently)."""
    r = f["kw"]["rules"]
    step = lambda p: np.linalg.norm(np.diff(p.astype(np.float64), axis=0), axis=1).mean()
    if abs(step(wp) - r.brake_speed) < margin:
        return True
    for k in range(0 if f["other_cast"] is None else len(f["other_cast"])):
        y = float(f["other_cast"][k, 0, 0, 1])
        if abs(y - r.behind) < margin:
            return True
        if y > r.behind:
            continue
        for m in range(6):
            score = float(f["other_cmds"][k, m])
            if abs(score - r.cmd_thresh) < margin:
                return True
            if score < r.cmd_thresh:
                continue
            traj = f["other_cast"][k, m]
            speed = step(traj)
            if abs(speed - r.brake_speed) < margin:
                return True
            limit = r.dist_static if speed < r.brake_speed else r.dist_moving
            if abs(np.linalg.norm(traj.astype(np.float64) - wp.astype(np.float64), axis=1).min() - limit) < margin:
                return True
    return False


def test_the_rules_are_the_agents_own_on_random_scenes():
    """2000 seeded scenes, T in {2, 5, 20, 64}, 0 .. 6 vehicles: the specification's "any forecast hit" is LAVAgent.plan_collide's answer
    and its slow bit is the brake flag LAVAgent.pid_control returns (T >= 7: the aim points reach waypoint 6).  A scene is left out only
    where a comparison lies within 1e-4 of its threshold - there float32 (the agent) and quantised float64 (here) may differ."""
    from lav_amd.lav_agent import LAVAgent
    scenes, left_out, hits, misses, disagree = 2000, 0, 0, 0, []
    for seed in range(scenes):
        T = (2, 5, 20, 64)[seed % 4]
        f = U.random_frame(1000 + seed, T=T, N=seed % 7, G=2)
        wp = f["ego_cast"] if f["cmd"] in (4, 5) else f["ego_plan"]
        if _near_a_threshold(f, wp):
            left_out += 1
            continue
        agent = _agent(f["kw"]["rules"])
        N = 0 if f["other_cast"] is None else len(f["other_cast"])
        theirs = LAVAgent.plan_collide(agent, wp, f["other_cast"] if N else np.zeros((0, 6, T, 2), np.float32), f["other_cmds"] if N else np.zeros((0, 6), np.float32))
        cause = E.DriveLayout(64).view(run(f), "cause")[f["bra"]]
        mask = int(np.flatnonzero(cause)[0])
        assert cause.sum() == 1
        ours = mask >> 1 != 0
        hits, misses = hits + int(ours), misses + int(not ours)
        if ours != bool(theirs):
            disagree.append((seed, "collide", ours, theirs))
        if T >= 7:
            _, _, brake = LAVAgent.pid_control(agent, wp, 3.0, f["cmd"])
            if bool(brake) != bool(mask & 1):
                disagree.append((seed, "slow", mask & 1, brake))
    print(f"{scenes} scenes: {left_out} left out, {hits} hit, {misses} do not, {len(disagree)} disagree")
    assert not disagree
    assert left_out <= scenes // 100
    assert hits >= scenes // 10 and misses >= scenes // 10


# ------------------------------------------------------------------------------------------------------------ layout, summary, command line
def test_layout_is_92_plus_6_nbins_and_the_library_agrees():
    from lav_amd import ops
    shapes = dict(frames=(), plan_nonfinite=(), expert_nonfinite=(), cause=(2, 8), gt_cause=(2, 8), collide_conf=(2, 2), ped=(2, 2), expert=(2, 2),
                  speed=(6, 4), aim=(6, 2), modes=(4,), vehicles_behind=(), clear_none=(2, 2))
    for nbins in (1, 64, 100, 1024):
        lay = E.DriveLayout(nbins)
        table = dict(shapes, speed_hist=(2, nbins), clear_hist=(2, 2, nbins))
        assert len(lay) == 92 + 6 * nbins == sum(int(np.prod(s)) for s in table.values()) == ops.eval_drive_words(nbins)
        assert list(lay.fields) == list(table) and all(lay.view(lay.zeros(), k).shape == s for k, s in table.items())
        assert lay.fields["clear_hist"][0].stop == len(lay) and E.DriveLayout.of(lay.zeros()).nbins == nbins
    for bad in (0, 1025, -1):
        with pytest.raises(ValueError):
            E.DriveLayout(bad)
        with pytest.raises(ValueError):
            ops.eval_drive_words(bad)
    for words in (92, 93, 92 + 6 * 1025, 100):
        with pytest.raises(ValueError):
            E.DriveLayout.of(np.zeros(words, np.int64))


def test_named_and_unnamed_round_trip():
    lay = E.DriveLayout(7)
    acc = np.random.default_rng(0).integers(0, 1 << 50, len(lay)).astype(np.int64)
    named = json.loads(json.dumps(lay.named(acc)))
    assert set(named) == set(lay.fields) and np.asarray(named["clear_hist"]).shape == (2, 2, 7)
    np.testing.assert_array_equal(lay.unnamed(named), acc)


def test_summary_of_a_hand_made_accumulator():
    lay = E.DriveLayout(4)
    # 10 frames: 4 labelled braking.  The rule brakes on 5: 3 of the braking ones (slow; static; slow + moving) and 2 of the driving ones (moving)
    acc = U.expect(lay, frames=12, plan_nonfinite=1, expert_nonfinite=1, cause={(1, 0): 1, (1, 1): 1, (1, 2): 1, (1, 5): 1, (0, 0): 4, (0, 4): 2},
                   gt_cause={(1, 0): 2, (1, 2): 2, (0, 0): 6}, collide_conf={(0, 0): 5, (0, 1): 3, (1, 1): 1, (1, 0): 1}, ped={(1, 1): 1, (1, 0): 3, (0, 0): 6},
                   expert={(1, 1): 3, (1, 0): 1, (0, 0): 6}, speed={2: (4, 4 * 19 * Q // 2, 4 * 19 * Q // 4, 4 * 19 * Q // 4)}, aim={2: (4 * Q, 2 * Q)},
                   modes=(9, 4, 3, 1), vehicles_behind=2, clear_none={(0, 0): 6, (1, 0): 2, (0, 1): 3, (1, 1): 3},
                   speed_hist={(1, 0): 2, (1, 1): 1, (1, 3): 1, (0, 1): 1, (0, 3): 5}, clear_hist={(1, 0, 0): 2, (0, 1, 1): 3, (1, 1, 3): 1})
    m = E.summarise(acc, 20)
    assert (m["frames"], m["plan_nonfinite"], m["expert_nonfinite"], m["evaluated"], m["labelled_brake"]) == (12, 1, 1, 10, 4)
    b = m["brake"]
    assert (b["tp"], b["fp"], b["fn"], b["brakes"]) == (3, 2, 1, 5) and b["precision"] == 0.6 and b["recall"] == 0.75 and b["f1"] == pytest.approx(2 / 3)
    assert b["share"] == dict(slow=0.4, collide_static=0.2, collide_moving=0.6, slow_only=0.2)
    g = m["brake_gt_futures"]
    assert (g["tp"], g["fp"], g["fn"]) == (2, 0, 2) and g["precision"] == 1.0 and g["recall"] == 0.5 and g["share"]["collide_static"] == 1.0
    c = m["collide_agreement"]
    assert (c["both"], c["forecast_only"], c["gt_only"], c["neither"]) == (1, 3, 1, 5) and c["agreement"] == 0.6 and c["precision"] == 0.25 and c["recall"] == 0.5
    assert m["pedestrian_near"] == dict(braking=0.25, driving=0.0) and m["expert_slow"] == dict(braking=0.75, driving=0.0)
    assert m["modes"] == dict(considered=9, static=4, hits=3, nonfinite=1, vehicles_behind=2)
    two = m["per_cmd"][2]
    assert two == dict(frames=4, desired_speed=0.5, expert_speed=0.25, speed_error=0.25, aim_error=1.0, lateral_error=0.5)
    assert m["per_cmd"][0] == dict(frames=0, desired_speed=None, expert_speed=None, speed_error=None, aim_error=None, lateral_error=None)
    # brake_speed: thresholds at the edges 1/64, 2/64, 3/64; braking frames in bins 0, 0, 1, 3, driving ones in 1 and 3 (x5)
    s = m["sweep"]["brake_speed"]
    assert [r["threshold"] for r in s] == [1 / 64, 2 / 64, 3 / 64]
    assert [(r["tp"], r["fp"], r["fn"]) for r in s] == [(2, 0, 2), (3, 1, 1), (3, 1, 1)] and s[0]["precision"] == 1.0 and s[1]["recall"] == 0.75
    # dist_static: two braking frames with a clearance in bin 0, two braking frames without a static forecast (they never brake)
    d = m["sweep"]["dist_static"]
    assert [r["threshold"] for r in d] == [0.125, 0.25, 0.375] and [(r["tp"], r["fp"], r["fn"]) for r in d] == [(2, 0, 2)] * 3
    v = m["sweep"]["dist_moving"]
    assert [(r["tp"], r["fp"], r["fn"]) for r in v] == [(0, 0, 4), (0, 3, 4), (0, 3, 4)] and v[0]["precision"] is None and v[1]["precision"] == 0.0
    json.dumps(m)


def test_summary_of_nothing_has_no_number():
    for nbins in (1, 64):
        m = E.summarise(E.DriveLayout(nbins).zeros(), 20)
        assert m["frames"] == 0 and len(m["sweep"]["brake_speed"]) == nbins - 1

        def numbers(x):
            if isinstance(x, dict):
                return [n for v in x.values() for n in numbers(v)]
            if isinstance(x, list):
                return [n for v in x for n in numbers(v)]
            return [x]
        ratios = [x for x in numbers({k: v for k, v in m.items() if k != "sweep"}) if not isinstance(x, int)]
        assert ratios and all(x is None for x in ratios)
        assert all(r["precision"] is None and r["recall"] is None and r["f1"] is None for table in m["sweep"].values() for r in table)


def test_rules_from_the_agents_config(tmp_path):
    from lav_amd.lav_agent import DEFAULT_CONFIG
    assert E.DriveRules.from_config(None) == E.DriveRules() == E.DriveRules.from_config(dict(DEFAULT_CONFIG))
    r = E.DriveRules.from_config(dict(pixels_per_meter=8, brake_speed=0.3, aim_point=[1, 2, 3, 4, 5, 6]), cmd_thresh=0.5, dist_static=None)
    assert (r.behind, r.ego_radius, r.brake_speed, r.cmd_thresh, r.dist_static, r.aim_point) == (4.0, 0.5, 0.3, 0.5, 1.0, (1, 2, 3, 4, 5, 6))
    assert json.loads(json.dumps(r.named()))["aim_point"] == [1, 2, 3, 4, 5, 6]
    path = tmp_path / "agent.yaml"
    path.write_text("brake_speed: 0.25\ncmd_thresh: 0.1\n")
    args = parser(E.TOOL).parse_args(["--synthetic", "--agent-config", str(path), "--dist-moving", "3", "--aim-point", "1", "1", "1", "1", "1", "1"])
    r = E._rules(args)
    assert (r.brake_speed, r.cmd_thresh, r.dist_static, r.dist_moving, r.aim_point) == (0.25, 0.1, 1.0, 3.0, (1,) * 6)


def test_command_line_help_and_the_message_without_a_gpu():
    tool = os.path.join(REPO, "eval_drive_v2.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, cwd=REPO)
    assert out.returncode == 0 and all(flag in out.stdout for flag in ("--brake-speed", "--cmd-thresh", "--dist-static", "--dist-moving", "--aim-point",
                                                                        "--agent-config", "--precision"))
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit) as e:
            E.main(["--synthetic", "--frames", "1"])
        assert "eval_drive_v2: no GPU visible" in str(e.value.code)
