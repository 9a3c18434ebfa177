"""lav_eval_distill on the MI355X against its specification (lav_amd.train.evaluate_distill.eval_distill_numpy), every word of the
accumulator compared exactly; UniPlanner.infer_batch and BEVPlanner.infer_batch against UniPlanner.forward, bit for bit, and against
UniPlanner.infer_all; the evaluator and its command line end to end.  The specification itself is checked in
tests/test_eval_distill_host.py.

The kernel gives every frame and every forecast a wave, four waves to a workgroup: the shapes below put B + K below, at and above that
share, with T at 1, 2, the networks' 20 and a full wave, and the fewest, the usual and the most stages."""
import json

import numpy as np
import pytest
import torch

from lav_amd import ops
from lav_amd.train import evaluate_bev as EB
from lav_amd.train import evaluate_distill as E
from tests import eval_distill_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def on_device(s):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in U.positional(s)]


def kernel(s, acc=None):
    acc = torch.zeros(len(E.PairLayout(s["s_ego_plan"].shape[1])), dtype=torch.int64, device=DEV) if acc is None else acc
    return ops.eval_distill(acc, *on_device(s))


def spec(s, acc=None):
    acc = E.PairLayout(s["s_ego_plan"].shape[1]).zeros() if acc is None else acc
    return E.eval_distill_numpy(acc, *U.positional(s))


@pytest.mark.parametrize("name", sorted(U.SCENES))
def test_kernel_equals_specification_on_every_scene(name):
    s = U.SCENES[name]()
    np.testing.assert_array_equal(kernel(s).cpu().numpy(), spec(s))


SHAPES = [(B, K, 20, 5) for B in (1, 4, 5) for K in (0, 1, 3, 4, 9)]             # B + K = 1 .. 14: 4 and 5 straddle a workgroup's four waves
SHAPES += [(B, K, T, I) for (B, K) in ((1, 3), (4, 1), (5, 9)) for T in (1, 2, 64) for I in (1, 8)]
SHAPES += [(1, 0, 1, 1), (5, 4, 64, 5), (4, 0, 2, 8)]


@pytest.mark.parametrize("B,K,T,I", SHAPES)
def test_kernel_equals_specification_on_random_batches(B, K, T, I):
    """(Planted NaNs, infinities, bad commands, identical modes and tied scores: eval_distill_util.random_batch.)"""
    for seed in (0, 1):
        s = U.random_batch(100 * B + K + seed, Bn=B, K=K, T=T, I=I)
        np.testing.assert_array_equal(kernel(s).cpu().numpy(), spec(s))


def test_no_forecasts_may_be_none_or_empty():
    s = U.random_batch(3, Bn=2, K=0)
    args = on_device(s)
    empty = [torch.zeros((0, 6, U.T, 2), device=DEV), torch.zeros((0, 6), device=DEV), torch.zeros((0, 6, U.T, 2), device=DEV),
             torch.zeros((0, 6), device=DEV), torch.zeros((0, U.T, 2), device=DEV)]
    acc = ops.eval_distill(torch.zeros(len(E.PairLayout(U.I)), dtype=torch.int64, device=DEV), *args[:8], *empty)
    np.testing.assert_array_equal(acc.cpu().numpy(), spec(s))
    np.testing.assert_array_equal(kernel(s).cpu().numpy(), spec(s))


def test_two_batches_into_one_accumulator():
    a, b = U.random_batch(7, Bn=5, K=3), U.random_batch(8, Bn=2, K=9)
    acc = kernel(b, kernel(a))
    want = spec(b, spec(a))
    np.testing.assert_array_equal(acc.cpu().numpy(), want)
    np.testing.assert_array_equal(kernel(U.concat(a, b)).cpu().numpy(), want)
    assert E.PairLayout(U.I).view(want, "frames").item() == 7


def test_the_accumulator_is_added_to():
    s = U.random_batch(9, Bn=6, K=10)
    lay = E.PairLayout(U.I)
    start = np.random.default_rng(0).integers((1 << 40) - 1000, (1 << 40) + 1000, len(lay)).astype(np.int64)
    acc = torch.from_numpy(start.copy()).to(DEV)
    kernel(s, acc)
    kernel(s, acc)
    np.testing.assert_array_equal(acc.cpu().numpy(), start + 2 * spec(s))


def test_bad_arguments_raise_before_any_launch():
    import ctypes as C
    from lav_amd import _lib
    s = U.random_batch(4, Bn=3, K=4)
    words = len(E.PairLayout(U.I))
    acc = torch.zeros(words, dtype=torch.int64, device=DEV)

    def call(acc=acc, **changed):
        g = dict(zip(U.ARGS, on_device(s)))
        g.update(changed)
        return ops.eval_distill(acc, *[g[k] for k in U.ARGS])

    with pytest.raises(ValueError, match="HBM"):
        call(ego_locs=torch.from_numpy(s["ego_locs"]))                                      # a host tensor
    with pytest.raises(ValueError, match="acc"):
        call(acc=torch.zeros(words, dtype=torch.int64))
    with pytest.raises(ValueError, match="words"):
        call(acc=torch.zeros(words - 1, dtype=torch.int64, device=DEV))                     # a wrong length
    with pytest.raises(ValueError, match="words"):
        call(acc=torch.zeros(len(E.PairLayout(U.I - 1)), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="acc"):
        call(acc=torch.zeros(words, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="s_ego_plan"):
        call(s_ego_plan=torch.zeros((3, U.I, 6, 65, 2), device=DEV))                        # T = 65
    with pytest.raises(ValueError, match="s_ego_plan"):
        call(s_ego_plan=torch.zeros((3, 9, 6, U.T, 2), device=DEV))                         # I = 9
    with pytest.raises(ValueError, match="t_ego_plan"):
        call(t_ego_plan=torch.zeros((3, U.I - 1, 6, U.T, 2), device=DEV))
    with pytest.raises(ValueError, match="t_ego_cast"):
        call(t_ego_cast=torch.zeros((3, 6, U.T + 1, 2), device=DEV))
    with pytest.raises(ValueError, match="cmds"):
        call(cmds=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="forecasts"):
        call(t_other_cmds=torch.zeros((5, 6), device=DEV))
    with pytest.raises(ValueError, match="forecasts"):
        call(other_locs=None)
    with pytest.raises(ValueError, match="other_locs"):
        call(other_locs=torch.zeros((4, U.T + 1, 2), device=DEV))
    with pytest.raises(ValueError, match="contiguous"):
        call(t_ego_cmds=torch.zeros((6, 3), device=DEV).t())                                # a strided view
    with pytest.raises(ValueError, match="contiguous|acc"):
        call(acc=torch.zeros(2 * words, dtype=torch.int64, device=DEV)[::2])
    # a misaligned view: torch cannot make one of these dtypes, so the entry point is handed the tensors' own addresses, one moved by 2
    # (4) bytes - it refuses on the addresses alone, before any launch
    lib = _lib.load()
    held = on_device(s)                                                                     # (keeps the addresses alive)
    ptrs = [None if t is None else t.data_ptr() for t in held]
    for moved, acc_off in ((6, 0), (10, 0), (None, 4)):
        p = [None if a is None else C.c_void_p(a + (2 if i == moved else 0)) for i, a in enumerate(ptrs)]
        rc = lib.lav_eval_distill(*p[:8], 3, U.I, U.T, *p[8:], 4, C.c_void_p(acc.data_ptr() + acc_off), None)
        assert rc != 0 and b"aligned" in lib.lav_last_error()
    torch.cuda.synchronize()
    assert int(acc.sum()) == 0


# ------------------------------------------------------------------------------------------------------------ infer_batch
N_FRAMES, CLOUD = 3, 20000


@pytest.fixture(scope="module")
def models():
    from tests.util import build_models
    return build_models(DEV)


@pytest.fixture(scope="module")
def batch3(models):
    """synthetic_lidar_batch(3) - its BEV half is synthetic_bev_batch(3, seed=2021), the batch of tests/test_gpu_eval_bev.py - with the
    student's feature map, computed once and left unchanged."""
    from lav_amd.train.synthetic import synthetic_lidar_batch
    lidars, num_points, _, _, _, bev, ego_locs, cmds, nxps, _, locs, oris, typs, _ = synthetic_lidar_batch(N_FRAMES, seed=2014, max_points=CLOUD)
    with torch.no_grad():
        features = models[0](lidars.float().to(DEV), [int(n) for n in num_points])[0].clone()
    return dict(features=features, bev=bev.float().to(DEV), cmds=cmds, poses=dict(ego_locs=ego_locs.float().to(DEV), locs=locs.float().to(DEV),
                oris=oris.float().to(DEV), nxps=nxps.float().to(DEV), typs=typs.to(DEV)))


@pytest.fixture(scope="module")
def inferred(models, batch3):
    """Both infer_batch(others="ahead") of the seeded batch, computed once and left unchanged, with the generators' states around them."""
    up = models[1]
    states = (torch.get_rng_state(), np.random.get_state()[1].copy(), torch.cuda.get_rng_state())
    student = up.infer_batch(batch3["features"], **batch3["poses"])
    teacher = up.bev_planner.infer_batch(batch3["bev"], **batch3["poses"])
    after = (torch.get_rng_state(), np.random.get_state()[1].copy(), torch.cuda.get_rng_state())
    return student, teacher, states, after


def test_infer_batch_equals_forward_without_jitter_bit_for_bit(models, batch3, inferred, monkeypatch):
    """UniPlanner.forward in eval mode, its jitters at 0 and max_num_cars = N (nothing is sub-sampled), runs the same kernels on the same
    inputs in the same crop order (nonzero's: sample-major, then actor): the student's six outputs and the teacher's four are equal in
    every bit."""
    up = models[1]
    student, teacher = inferred[:2]
    p = batch3["poses"]
    N = p["locs"].shape[1] - 1
    monkeypatch.setattr(up, "feature_x_jitter", 0)
    monkeypatch.setattr(up, "feature_angle_jitter", 0.0)
    monkeypatch.setattr(up, "max_num_cars", N)
    assert not up.training
    with torch.no_grad():
        (other_locs, other_cast, other_cmds, other_cast_expert, other_cmds_expert, _, ego_plan, ego_cast, ego_cmds, ego_cast_expert,
         ego_plan_expert) = up(batch3["features"], batch3["bev"], p["ego_locs"], p["locs"], p["oris"], p["nxps"], p["typs"])
    K = student.other_locs.shape[0]
    assert 0 < K < N_FRAMES * N, "the seeded batch has vehicles ahead, and some that are not"
    assert student.ego_plan.shape == (N_FRAMES, 5, 6, 20, 2) and student.other_cast.shape == (K, 6, 20, 2) and student.sample.shape == student.actor.shape == (K,)
    for name, got, ref in (("other_locs", student.other_locs, other_locs), ("other_cast", student.other_cast, other_cast),
                           ("other_cmds", student.other_cmds, other_cmds), ("ego_plan", student.ego_plan, ego_plan),
                           ("ego_cast", student.ego_cast, ego_cast), ("ego_cmds", student.ego_cmds, ego_cmds),
                           ("teacher other_cast", teacher.other_cast, other_cast_expert), ("teacher other_cmds", teacher.other_cmds, other_cmds_expert),
                           ("teacher ego_cast", teacher.ego_cast, ego_cast_expert), ("teacher ego_plan", teacher.ego_plan, ego_plan_expert)):
        assert got.shape == ref.shape and torch.equal(got, ref), name
    # the index of every forecast: the picked vehicles in nonzero's order, the same for both arms
    ahead = (p["typs"][:, 1:] == 1) & (p["locs"][:, 1:, 0, 1] < p["ego_locs"][:, None, 0, 1])
    where = torch.nonzero(ahead)
    for out in (student, teacher):
        assert torch.equal(out.sample, where[:, 0].int()) and torch.equal(out.actor, where[:, 1].int())
    assert torch.equal(student.other_locs, teacher.other_locs)


def test_infer_batch_ego_outputs_agree_with_infer_all_frame_by_frame(models, batch3, inferred):
    """UniPlanner.infer_all crops, embeds and plans with other kernels (lav_crop_rotate, lav_embed_cast, one frame, one command): within
    the project's waypoint bar, 1e-4."""
    up, out = models[1], inferred[0]
    worst = 0.0
    for i in range(N_FRAMES):
        cmd = int(batch3["cmds"][i])
        _, plan, cast, _, _ = up.infer_all(batch3["features"][i], [], cmd, batch3["poses"]["nxps"][i])
        for name, got, ref in (("plan", out.ego_plan[i, -1, cmd], plan), ("cast", out.ego_cast[i, cmd], cast)):
            err = float((got - ref).abs().max())
            worst = max(worst, err)
            print(f"frame {i} command {cmd} {name}: max |infer_batch - infer_all| = {err:.3e}")
            assert err <= 1e-4, (i, name, err)
    print(f"measured maximum: {worst:.3e}")


def test_infer_batch_draws_nothing_and_takes_all_or_none(models, batch3, inferred):
    up = models[1]
    out, _, before, after = inferred
    assert torch.equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and torch.equal(before[2], after[2])
    f, p = batch3["features"], batch3["poses"]
    everyone = up.infer_batch(f, **p, others="all")
    vehicles = int((p["typs"][:, 1:] == 1).sum())
    assert everyone.other_locs.shape[0] == vehicles >= out.other_locs.shape[0]
    for a, b in ((everyone.ego_plan, out.ego_plan), (everyone.ego_cast, out.ego_cast), (everyone.ego_cmds, out.ego_cmds)):
        assert torch.equal(a, b), "the ego's outputs do not depend on who else is scored"
    nobody = up.infer_batch(f, **dict(p, typs=torch.zeros_like(p["typs"])))
    assert nobody.other_locs.shape == (0, 20, 2) and nobody.other_cast.shape == (0, 6, 20, 2) and nobody.other_cmds.shape == (0, 6)
    assert nobody.other_cast.is_cuda and nobody.other_cmds.is_cuda and nobody.sample.numel() == 0 and torch.equal(nobody.ego_cast, out.ego_cast)
    with pytest.raises(ValueError):
        up.infer_batch(f, **p, others="behind")
    with pytest.raises(RuntimeError, match="HBM"):
        up.infer_batch(f.cpu(), **p)
    up.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            up.infer_batch(f, **p)
    finally:
        up.eval()


# ------------------------------------------------------------------------------------------------------------ the evaluator
@pytest.fixture(scope="module")
def five_frames():
    from lav_amd.train.synthetic import synthetic_lidar_batch
    return [synthetic_lidar_batch(3, seed=5, max_points=CLOUD), synthetic_lidar_batch(2, seed=6, max_points=CLOUD)]


def test_evaluator_adds_the_same_counters_on_the_device_and_on_the_host(models, five_frames):
    batches = five_frames
    on_gpu, on_host = E.DistillEvaluator(models), E.DistillEvaluator(models, device="cpu")
    assert on_gpu.run(batches) == on_host.run(batches) == 5
    assert on_gpu.acc.is_cuda and not on_host.acc.is_cuda
    acc = on_gpu.counters()
    np.testing.assert_array_equal(acc, on_host.counters())
    assert "student" in on_gpu.precision() and "teacher" in on_gpu.precision()
    lay = on_gpu.layout
    pair, t_sec, s_sec = lay.fields(acc, "pair"), lay.fields(acc, "teacher"), lay.fields(acc, "student")
    assert pair["frames"].item() == t_sec["frames"].item() == s_sec["frames"].item() == 5
    for s in range(lay.stages):
        assert pair["ego_closer"][s].sum() + pair["ego_unjudged"][s] + pair["bad_cmd"].item() == pair["frames"].item()
    m = E.summarise(acc)
    assert m["frames"] == 5 and len(m["pair"]["stages"]) == 6 and m["pair"]["others"]["scored"] > 0 and "NaN" not in json.dumps(m)

    # run() regroups: the same five frames handed over one by one, or in one batch, run as the same forwards
    one_by_one = [tuple(t[i:i + 1] for t in b) for b in batches for i in range(len(b[7]))]
    regrouped, whole = E.DistillEvaluator(models), E.DistillEvaluator(models)
    assert regrouped.run(one_by_one) == 5 and whole.run([tuple(torch.cat([a, b]) for a, b in zip(*batches))]) == 5
    np.testing.assert_array_equal(regrouped.counters(), whole.counters())
    np.testing.assert_array_equal(acc, whole.counters())
    limited = E.DistillEvaluator(models)
    assert limited.run(batches, max_frames=4) == 4 and lay.fields(limited.counters(), "pair")["frames"].item() == 4

    # the teacher section is eval_bev_v2's accumulator on the same frames (train_bev's tuple is the tail of train_lidar's)
    bev = EB.BevEvaluator(models[1].bev_planner, others="ahead", frames_per_forward=8)
    assert bev.run([b[5:] for b in batches]) == 5
    np.testing.assert_array_equal(lay.view(acc, "teacher"), bev.counters())

    # the student section is eval_plans' specification on what the student's infer_batch returned
    again = E.DistillEvaluator(models)
    again.upload([torch.cat([a, b]) for a, b in zip(*batches)])
    with torch.no_grad():
        student, _ = again.infer()
    for t in student[:6]:
        assert bool(torch.isfinite(t).all()), "no student output is non-finite (the premise of the forecast count below)"
    b = again._batch
    want = EB.eval_plans_numpy(EB.PlanLayout(5).zeros(), student.ego_plan, student.ego_cast, student.ego_cmds, b["ego_locs"], b["cmds"], b["bras"],
                               student.other_cast, student.other_cmds, student.other_locs)
    np.testing.assert_array_equal(lay.view(acc, "student"), want)
    assert pair["others"].item() + pair["oth_nonfinite"].item() == t_sec["others"].item() + t_sec["oth_nonfinite"].item() > 0

    everyone = E.DistillEvaluator(models, others="all")
    assert everyone.run(batches) == 5
    scored = lambda f: int(f["others"].item() + f["oth_nonfinite"].item())
    assert scored(lay.fields(everyone.counters(), "pair")) >= scored(pair)
    np.testing.assert_array_equal(lay.fields(everyone.counters(), "pair")["ego_gap"], pair["ego_gap"])


@pytest.fixture(scope="module")
def seeded_checkpoints(tmp_path_factory):
    from lav_amd.train import LAV, TrainConfig
    root = tmp_path_factory.mktemp("eval_distill_ck")
    seeded = LAV(TrainConfig(), torch.device("cpu"), what="lidar")
    for k in ("lidar", "uniplanner"):
        torch.save(seeded.state_dict(k), root / f"{k}_seed.th")
    return root


def test_command_line_on_recorded_routes(tmp_path, seeded_checkpoints, monkeypatch, capsys):
    """eval_distill_v2 over a short synthetic route with saved seeded checkpoints: the JSON's counters are the three specifications' on
    what the kernels were handed (captured on the way in); a missing checkpoint is an error that names the config's key."""
    from tests.util import dataset_fixture_config
    cfg = dataset_fixture_config(str(tmp_path), routes=1, frames=23)
    ck = seeded_checkpoints
    base = ["--config-path", cfg, "--num-workers", "0", "--precision", "f16x3", "--uniplanner", str(ck / "uniplanner_seed.th")]
    with pytest.raises(SystemExit) as e:
        E.main(base)
    assert e.value.code not in (0, None) and "lidar_model_dir" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        E.main(base + ["--lidar", str(ck / "lidar_seed.th"), "--bev", str(tmp_path / "absent.th")])
    assert e.value.code not in (0, None) and "--bev" in str(e.value.code)

    seen = {"eval_plans": [], "eval_distill": []}

    def spy(name):
        real = getattr(ops, name)

        def wrapped(acc, *args):
            seen[name].append([None if a is None else a.detach().cpu().numpy().copy() for a in args])
            return real(acc, *args)
        return wrapped

    monkeypatch.setattr(ops, "eval_plans", spy("eval_plans"))
    monkeypatch.setattr(ops, "eval_distill", spy("eval_distill"))
    capsys.readouterr()
    out_file = tmp_path / "eval.json"
    lines = E.main(base + ["--lidar", str(ck / "lidar_seed.th"), "--batch-size", "2", "--out", str(out_file)])
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == len(printed) == 1 and printed[0] == json.loads(json.dumps(lines[0])) == json.loads(out_file.read_text())
    line = printed[0]
    frames = line["summary"]["frames"]
    groups = [8] * (frames // 8) + ([frames % 8] if frames % 8 else [])                     # (frames_per_forward, not the loader's 2)
    assert frames >= 3 and [len(a[7]) for a in seen["eval_distill"]] == groups and len(seen["eval_plans"]) == 2 * len(groups)
    lay = E.DistillLayout(seen["eval_distill"][0][0].shape[1])
    want = lay.zeros()
    for i, args in enumerate(seen["eval_distill"]):
        assert args[0].shape[2:] == (6, 20, 2) and args[7].dtype == np.int32
        EB.eval_plans_numpy(lay.view(want, "teacher"), *seen["eval_plans"][2 * i])
        EB.eval_plans_numpy(lay.view(want, "student"), *seen["eval_plans"][2 * i + 1])
        E.eval_distill_numpy(lay.view(want, "pair"), *args)
        for k in (0, 1, 2, 8, 9):                                                           # the pair launch read the student launch's tensors
            j = {0: 0, 1: 1, 2: 2, 8: 6, 9: 7}[k]
            np.testing.assert_array_equal(args[k], seen["eval_plans"][2 * i + 1][j])
    assert line["counters"] == lay.named(want)
    assert line["counters"]["pair"]["frames"] == frames and "student" in line["precision"] and "f16x3" in line["precision"]
    assert line["others"] == "ahead" and "ground-truth poses" in line["note"] and "eval_full_v2.py" in line["note"]


def test_command_line_synthetic_at_every_precision(capsys):
    """--precision all: three summaries of the same frames with the arithmetic in force.  What does not depend on the arithmetic - the
    frames, the forecasts made - is identical; how the outputs differ is what the tool is there to measure, nothing is asserted."""
    lines = E.main(["--synthetic", "--frames", "4", "--max-points", str(CLOUD), "--precision", "all"])
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["asked"] for l in printed] == ["f16x3", "bf16x6", "f32"] and len(lines) == 3
    forecasts = lambda l: l["counters"]["pair"]["others"] + l["counters"]["pair"]["oth_nonfinite"]
    for l, name in zip(printed, ("f16x3", "bf16x6", "f32")):
        assert l["summary"]["frames"] == l["counters"]["pair"]["frames"] == l["counters"]["student"]["frames"] == 4
        assert forecasts(l) == forecasts(printed[0]) > 0
        assert l["precision"] == f"student {name}+teacher {name}" and "ground-truth poses" in l["note"]
