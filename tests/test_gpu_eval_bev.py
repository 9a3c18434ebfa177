"""lav_eval_plans on the MI355X against its specification (lav_amd.train.evaluate_bev.eval_plans_numpy), every word of the accumulator
compared exactly; BEVPlanner.infer_batch against BEVPlanner.forward and BEVPlanner.infer; the evaluator and its command line end to end.
The specification itself is checked in tests/test_eval_bev_host.py.

The kernel gives every frame and every forecast a wave, four waves to a workgroup: the shapes below put B, K and B + K one below, at and
one above that share."""
import json

import numpy as np
import pytest
import torch

from lav_amd import ops, synth
from lav_amd.train import evaluate_bev as E
from tests import eval_bev_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def on_device(s):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in U.positional(s)]


def kernel(s, acc=None):
    acc = torch.zeros(len(E.PlanLayout(s["ego_plan"].shape[1])), dtype=torch.int64, device=DEV) if acc is None else acc
    return ops.eval_plans(acc, *on_device(s))


def spec(s, acc=None):
    acc = E.PlanLayout(s["ego_plan"].shape[1]).zeros() if acc is None else acc
    return E.eval_plans_numpy(acc, *U.positional(s))


@pytest.mark.parametrize("name", sorted(U.SCENES))
def test_kernel_equals_specification_on_every_scene(name):
    s = U.SCENES[name]()
    np.testing.assert_array_equal(kernel(s).cpu().numpy(), spec(s))


SHAPES = [(1, 0, 20, 5),                                                    # one frame, no forecast: one wave of one workgroup
          (5, 7, 1, 5), (5, 7, 20, 5), (5, 7, 64, 5),                       # T = 1, the teacher's 20, one full wave
          (5, 7, 20, 1), (5, 7, 20, 8),                                     # the fewest and the most stages
          (3, 0, 20, 5), (4, 0, 20, 5), (5, 0, 20, 5),                      # frames: one below, at and one above a workgroup's four waves
          (4, 3, 20, 5), (4, 4, 20, 5), (4, 5, 20, 5),                      # forecasts likewise, starting on a workgroup's first wave
          (1, 2, 20, 5), (1, 3, 20, 5), (1, 4, 20, 5), (3, 5, 20, 5),       # ... and frames and forecasts sharing a workgroup
          (2, 37, 20, 5), (37, 41, 64, 8)]


@pytest.mark.parametrize("B,K,T,I", SHAPES)
def test_kernel_equals_specification_on_random_batches(B, K, T, I):
    for seed in (0, 1):
        s = U.random_batch(100 * B + K + seed, B=B, K=K, T=T, I=I)
        np.testing.assert_array_equal(kernel(s).cpu().numpy(), spec(s))


def test_no_forecasts_may_be_none_or_empty():
    s = U.random_batch(3, B=2, K=0)
    args = on_device(s)
    empty = [torch.zeros((0, 6, U.T, 2), device=DEV), torch.zeros((0, 6), device=DEV), torch.zeros((0, U.T, 2), device=DEV)]
    acc = ops.eval_plans(torch.zeros(len(E.PlanLayout(U.I)), dtype=torch.int64, device=DEV), *args[:6], *empty)
    np.testing.assert_array_equal(acc.cpu().numpy(), spec(s))
    np.testing.assert_array_equal(kernel(s).cpu().numpy(), spec(s))


def test_two_batches_into_one_accumulator():
    a, b = U.random_batch(7, B=5, K=3), U.random_batch(8, B=2, K=9)
    acc = kernel(b, kernel(a))
    want = spec(b, spec(a))
    np.testing.assert_array_equal(acc.cpu().numpy(), want)
    np.testing.assert_array_equal(kernel(U.concat(a, b)).cpu().numpy(), want)
    assert E.PlanLayout(U.I).view(want, "frames").item() == 7


def test_the_accumulator_is_added_to():
    s = U.random_batch(9, B=6, K=10)
    lay = E.PlanLayout(U.I)
    start = np.random.default_rng(0).integers((1 << 40) - 1000, (1 << 40) + 1000, len(lay)).astype(np.int64)
    acc = torch.from_numpy(start.copy()).to(DEV)
    kernel(s, acc)
    kernel(s, acc)
    np.testing.assert_array_equal(acc.cpu().numpy(), start + 2 * spec(s))


def test_bad_arguments_raise_before_any_launch():
    s = U.random_batch(4, B=3, K=4)
    acc = torch.zeros(len(E.PlanLayout(U.I)), dtype=torch.int64, device=DEV)

    def call(acc=acc, **changed):
        g = dict(zip(U.ARGS, on_device(s)))
        g.update(changed)
        return ops.eval_plans(acc, *[g[k] for k in U.ARGS])

    with pytest.raises(ValueError, match="HBM"):
        call(ego_locs=torch.from_numpy(s["ego_locs"]))
    with pytest.raises(ValueError, match="cmds"):
        call(cmds=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="bras"):
        call(bras=torch.zeros(3, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="ego_cast"):
        call(ego_cast=torch.zeros((3, 6, U.T + 1, 2), device=DEV))
    with pytest.raises(ValueError, match="ego_plan"):
        call(ego_plan=torch.zeros((3, U.I, 6, 65, 2), device=DEV))
    with pytest.raises(ValueError, match="ego_plan"):
        call(ego_plan=torch.zeros((0, U.I, 6, U.T, 2), device=DEV))
    with pytest.raises(ValueError, match="forecasts"):
        call(other_cmds=torch.zeros((5, 6), device=DEV))
    with pytest.raises(ValueError, match="forecasts"):
        call(other_locs=None)
    with pytest.raises(ValueError, match="other_locs"):
        call(other_locs=torch.zeros((4, U.T + 1, 2), device=DEV))
    with pytest.raises(ValueError, match="contiguous"):
        call(ego_cmds=torch.zeros((6, 3), device=DEV).t())
    with pytest.raises(ValueError, match="words"):
        call(acc=torch.zeros(len(E.PlanLayout(U.I - 1)), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="acc"):
        call(acc=torch.zeros(len(E.PlanLayout(U.I)), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="acc"):
        call(acc=torch.zeros(len(E.PlanLayout(U.I)), dtype=torch.int64))
    assert int(acc.sum()) == 0


# ------------------------------------------------------------------------------------------------------------ infer_batch
@pytest.fixture(scope="module")
def teacher():
    import lav_amd
    from tests.util import Y_OFF
    bp = lav_amd.BEVPlanner(pixels_per_meter=4, crop_size=96, feature_x_jitter=1.5, feature_angle_jitter=20, x_offset=0, y_offset=Y_OFF,
                            num_cmds=6, num_plan=20, num_plan_iter=5, num_frame_stack=2)
    bp.load_state_dict(synth.seeded_state_dict(bp, prefix="uni.bev_planner."))
    return bp.eval().to(DEV)


@pytest.fixture(scope="module")
def batch3():
    from lav_amd.train.synthetic import synthetic_bev_batch
    bev, ego_locs, cmds, nxps, bras, locs, oris, typs, _ = synthetic_bev_batch(3, seed=2021)
    return dict(bev=bev.float().to(DEV), ego_locs=ego_locs.float().to(DEV), locs=locs.float().to(DEV), oris=oris.float().to(DEV),
                nxps=nxps.float().to(DEV), typs=typs.to(DEV))


@pytest.fixture(scope="module")
def inferred(teacher, batch3):
    """infer_batch(others="ahead") of the seeded batch, computed once and left unchanged, with the generators' states around it."""
    states = (torch.get_rng_state(), np.random.get_state()[1].copy(), torch.cuda.get_rng_state())
    out = teacher.infer_batch(**batch3)
    after = (torch.get_rng_state(), np.random.get_state()[1].copy(), torch.cuda.get_rng_state())
    return out, states, after


def test_infer_batch_equals_forward_without_jitter_bit_for_bit(teacher, batch3, inferred, monkeypatch):
    """forward in eval mode, its jitters at 0 and max_num_cars = N (nothing is sub-sampled), runs the same kernels on the same inputs in the
    same crop order (nonzero's: sample-major, then actor): all six outputs are equal in every bit."""
    out = inferred[0]
    monkeypatch.setattr(teacher, "feature_x_jitter", 0)
    monkeypatch.setattr(teacher, "feature_angle_jitter", 0.0)
    monkeypatch.setattr(teacher, "max_num_cars", batch3["locs"].shape[1] - 1)
    with torch.no_grad():
        want = teacher(batch3["bev"], batch3["ego_locs"], batch3["locs"], batch3["oris"], batch3["nxps"], batch3["typs"])
    K = out.other_locs.shape[0]
    assert 0 < K < 3 * (batch3["locs"].shape[1] - 1), "the seeded batch has vehicles ahead, and some that are not"
    assert out.ego_plan.shape == (3, 5, 6, 20, 2) and out.other_cast.shape == (K, 6, 20, 2) and out.sample.shape == out.actor.shape == (K,)
    for name, got, ref in zip(out._fields, out[:6], want):
        assert got.shape == ref.shape and torch.equal(got, ref), name
    # the index of every forecast: the picked vehicles in nonzero's order
    ahead = (batch3["typs"][:, 1:] == 1) & (batch3["locs"][:, 1:, 0, 1] < batch3["ego_locs"][:, None, 0, 1])
    where = torch.nonzero(ahead)
    assert torch.equal(out.sample, where[:, 0].int()) and torch.equal(out.actor, where[:, 1].int())


def test_infer_batch_ego_outputs_agree_with_infer_frame_by_frame(teacher, batch3, inferred):
    """BEVPlanner.infer crops and plans with other kernels (lav_crop_rotate, one frame): within the project's waypoint bar, 1e-4."""
    out = inferred[0]
    for i in range(3):
        plan, cast, cmds = teacher.infer(batch3["bev"][i:i + 1], batch3["nxps"][i:i + 1])
        for name, got, ref in (("plan", out.ego_plan[i], plan[0]), ("cast", out.ego_cast[i], cast[0]), ("cmds", out.ego_cmds[i], cmds[0])):
            err = float((got - ref).abs().max())
            print(f"frame {i} {name}: max |infer_batch - infer| = {err:.3e}")
            assert err <= 1e-4, (i, name, err)


def test_infer_batch_draws_nothing_and_takes_all_or_none(teacher, batch3, inferred):
    out, before, after = inferred
    assert torch.equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and torch.equal(before[2], after[2])
    everyone = teacher.infer_batch(**batch3, others="all")
    vehicles = int((batch3["typs"][:, 1:] == 1).sum())
    assert everyone.other_locs.shape[0] == vehicles > out.other_locs.shape[0]
    assert torch.equal(everyone.ego_plan, out.ego_plan), "the ego's outputs do not depend on who else is scored"
    nobody = teacher.infer_batch(**dict(batch3, typs=torch.zeros_like(batch3["typs"])))
    assert nobody.other_locs.shape == (0, 20, 2) and nobody.other_cast.shape == (0, 6, 20, 2) and nobody.other_cmds.shape == (0, 6)
    assert nobody.other_cast.is_cuda and nobody.sample.numel() == 0 and torch.equal(nobody.ego_cast, out.ego_cast)
    with pytest.raises(ValueError):
        teacher.infer_batch(**batch3, others="behind")
    teacher.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            teacher.infer_batch(**batch3)
    finally:
        teacher.eval()


# ------------------------------------------------------------------------------------------------------------ the evaluator
def test_evaluator_adds_the_same_counters_on_the_device_and_on_the_host(teacher):
    from lav_amd.train.synthetic import synthetic_bev_batch
    batches = [synthetic_bev_batch(3, seed=5), synthetic_bev_batch(2, seed=6)]
    on_gpu, on_host = E.BevEvaluator(teacher), E.BevEvaluator(teacher, device="cpu")
    assert on_gpu.run(batches) == on_host.run(batches) == 5
    assert on_gpu.acc.is_cuda and not on_host.acc.is_cuda
    np.testing.assert_array_equal(on_gpu.counters(), on_host.counters())
    m = E.summarise(on_gpu.counters())
    assert m["frames"] == 5 and m["plan"]["all"][0]["frames"] + m["plan"]["nonfinite"][0] + m["bad_cmd"] == 5 and m["others"]["scored"] > 0
    lay = on_gpu.layout
    everyone = E.BevEvaluator(teacher, others="all")
    assert everyone.run(batches) == 5 and on_gpu.run(batches, max_frames=5) == 5
    scored = lambda acc: int(lay.view(acc, "others").sum() + lay.view(acc, "oth_nonfinite").sum())
    assert scored(everyone.counters()) >= scored(on_gpu.counters())
    np.testing.assert_array_equal(lay.view(everyone.counters(), "plan"), lay.view(on_gpu.counters(), "plan"))
    limited = E.BevEvaluator(teacher)
    assert limited.run(batches, max_frames=4) == 4 and lay.view(limited.counters(), "frames").item() == 4
    # run() regroups: the same five frames handed over one by one, or in one batch, run as the same forwards
    one_by_one = [tuple(t[i:i + 1] for t in b) for b in batches for i in range(len(b[2]))]
    regrouped, whole = E.BevEvaluator(teacher), E.BevEvaluator(teacher)
    assert regrouped.run(one_by_one) == 5 and whole.run([tuple(torch.cat([a, b]) for a, b in zip(*batches))]) == 5
    np.testing.assert_array_equal(regrouped.counters(), whole.counters())
    np.testing.assert_array_equal(on_gpu.counters(), whole.counters())
    pairs = E.BevEvaluator(teacher, frames_per_forward=2)
    assert pairs.run(batches) == 5 and lay.view(pairs.counters(), "others").item() == lay.view(whole.counters(), "others").item()


@pytest.fixture(scope="module")
def seeded_checkpoint(tmp_path_factory):
    from lav_amd.train import LAV, TrainConfig
    path = tmp_path_factory.mktemp("eval_bev_ck") / "bev_seed.th"
    torch.save(LAV(TrainConfig(), torch.device("cpu"), what="bev").state_dict("bev"), path)
    return path


def test_command_line_on_recorded_routes(tmp_path, seeded_checkpoint, monkeypatch, capsys):
    """eval_bev_v2 over a 5-frame synthetic route with a saved seeded checkpoint: the JSON's counters are the specification's on what the
    kernel was handed (captured on the way in), a second run prints the same counters, so do batches of 1 and of 4, a missing
    checkpoint is an error that names the config's key."""
    from tests.util import dataset_fixture_config
    cfg = dataset_fixture_config(str(tmp_path), routes=1, frames=25)
    base = ["--config-path", cfg, "--num-workers", "0"]
    with pytest.raises(SystemExit) as e:
        E.main(base)
    assert e.value.code not in (0, None) and "bev_model_dir" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        E.main(base + ["--bev", str(tmp_path / "absent.th")])
    assert e.value.code not in (0, None) and "bev_model_dir" in str(e.value.code)

    seen, real = [], ops.eval_plans

    def spy(acc, *args):
        seen.append([None if a is None else a.detach().cpu().numpy().copy() for a in args])
        return real(acc, *args)

    monkeypatch.setattr(ops, "eval_plans", spy)
    capsys.readouterr()
    out_file = tmp_path / "eval.json"
    base += ["--bev", str(seeded_checkpoint)]
    lines = E.main(base + ["--batch-size", "4", "--out", str(out_file)])
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == len(printed) == 1 and printed[0] == json.loads(json.dumps(lines[0])) == json.loads(out_file.read_text())
    frames = printed[0]["summary"]["frames"]
    assert frames >= 5 and [len(args[4]) for args in seen] == [8] * (frames // 8) + ([frames % 8] if frames % 8 else [])     # (frames_per_forward)
    lay = E.PlanLayout(seen[0][0].shape[1])
    want = lay.zeros()
    for args in seen:
        assert args[0].shape[2:] == (6, 20, 2) and args[4].dtype == np.int32 and args[5].dtype == np.uint8
        E.eval_plans_numpy(want, *args)
    assert printed[0]["counters"] == lay.named(want)
    assert printed[0]["counters"]["frames"] == frames and printed[0]["counters"]["others"] + printed[0]["counters"]["oth_nonfinite"] > 0
    assert printed[0]["precision"] in E.PRECISIONS and printed[0]["others"] == "ahead"
    again = E.main(base + ["--batch-size", "4"])
    assert again[0]["counters"] == printed[0]["counters"]
    ones = E.main(base + ["--batch-size", "1"])              # (the forward's batch is the evaluator's, not the loader's)
    for name in lay.fields:
        print(name, "batch 1:", ones[0]["counters"][name], "batch 4:", printed[0]["counters"][name])
    assert ones[0]["counters"] == printed[0]["counters"]
    assert ones[0]["batch_size"] == 1 and printed[0]["batch_size"] == 4


def test_command_line_synthetic_at_every_precision(capsys):
    """--precision all: three summaries of the same frames.  What does not depend on the arithmetic - frames, frames per command, the
    forecasts made - is identical; how the predictions differ is what the tool is there to measure, nothing is asserted."""
    lines = E.main(["--synthetic", "--frames", "3", "--batch-size", "2", "--precision", "all"])
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["asked"] for l in printed] == ["f16x3", "bf16x6", "f32"] and len(lines) == 3
    forecasts = lambda l: l["counters"]["others"] + l["counters"]["oth_nonfinite"]
    for l in printed:
        assert l["summary"]["frames"] == l["counters"]["frames"] == 3
        assert l["summary"]["frames_per_cmd"] == printed[0]["summary"]["frames_per_cmd"] and sum(l["summary"]["frames_per_cmd"]) == 3
        assert forecasts(l) == forecasts(printed[0]) > 0
    assert [l["precision"] for l in printed] == ["f16x3", "bf16x6", "f32"]
