"""lav_eval_drive on the MI355X against its specification (lav_amd.train.evaluate_drive.eval_drive_numpy), every word of the accumulator
compared exactly, DriveEvaluator with the accumulator in HBM against the same run on the host, and Evaluator (eval_full) after the
split of its frame.  The specification itself is checked in tests/test_eval_drive_host.py."""
import json

import numpy as np
import pytest
import torch

from lav_amd import ops
from lav_amd.train import evaluate as F
from lav_amd.train import evaluate_drive as E
from tests import eval_drive_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def on_device(f):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if isinstance(a, np.ndarray) else a for a in U.positional(f)]


def kernel(f, acc=None):
    acc = torch.zeros(len(E.DriveLayout(f["kw"]["nbins"])), dtype=torch.int64, device=DEV) if acc is None else acc
    return ops.eval_drive(acc, *on_device(f), **f["kw"])


def spec(f, acc=None):
    acc = E.DriveLayout(f["kw"]["nbins"]).zeros() if acc is None else acc
    return E.eval_drive_numpy(acc, *U.positional(f), **f["kw"])


def same(f):
    got, want = kernel(f).cpu().numpy(), spec(f)
    lay = E.DriveLayout(f["kw"]["nbins"])
    assert lay.named(got) == lay.named(want)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", sorted(U.SCENES))
def test_kernel_equals_specification_on_every_scene(name):
    f, want = U.SCENES[name]()
    np.testing.assert_array_equal(kernel(f).cpu().numpy(), want)
    same(f)


@pytest.mark.parametrize("T", [2, 20, 64])
@pytest.mark.parametrize("N", [0, 1, 5, 64])
def test_kernel_equals_specification_on_random_frames(T, N):
    """N = 5 is 30 modes for four waves (the item loop runs), N = 64 and G = 64 the most the kernel takes; n = 0 and n = G."""
    for G in (1, 10, 64):
        for n in (0, G):
            same(U.random_frame(7 * T + 3 * N + G + n, T=T, N=N, G=G, n=n))


def test_random_frames_with_values_that_are_not_finite():
    f = U.random_frame(77, N=5)
    f["other_cast"][1, 2, 5, 0] = np.nan
    f["other_cast"][3, 0, 0, 1] = np.nan              # the behind test of a NaN: not behind
    f["other_cmds"][:, 4] = np.nan
    f["other_cmds"][2, :] = 1.0
    f["locs"][3, 7, 1] = np.inf
    f["locs"][4, 0, :] = np.nan
    f["typs"][3], f["typs"][4], f["typs"][5] = 1, 1, 0
    f["locs"][5, 2, 0] = np.nan
    same(f)
    f["ego_locs"][U.T - 1, 1] = np.nan
    same(f)


@pytest.mark.parametrize("nbins", [1, 64, 1024])
def test_several_frames_into_one_accumulator_that_is_not_zero(nbins):
    lay = E.DriveLayout(nbins)
    start = np.random.default_rng(nbins).integers(0, 1 << 40, len(lay)).astype(np.int64)
    acc, want = torch.from_numpy(start.copy()).to(DEV), start.copy()
    for seed, N in ((1, 0), (2, 3), (3, 7), (4, 2)):
        f = U.random_frame(seed, N=N, nbins=nbins)
        acc, want = kernel(f, acc), spec(f, want)
    f, _ = U.scene_nan_plan()
    f["kw"]["nbins"] = nbins
    acc, want = kernel(f, acc), spec(f, want)
    np.testing.assert_array_equal(acc.cpu().numpy(), want)
    assert lay.view(want - start, "frames").item() == 5 and lay.view(want - start, "plan_nonfinite").item() == 1


def test_the_library_and_the_layout_agree_on_the_length():
    for nbins in (1, 7, 64, 1024):
        assert ops.eval_drive_words(nbins) == len(E.DriveLayout(nbins))


def test_bad_arguments_raise_before_any_launch():
    f = U.random_frame(5, N=3)
    acc = torch.zeros(len(E.DriveLayout(64)), dtype=torch.int64, device=DEV)

    def call(acc=acc, rules=None, nbins=64, **changed):
        g = dict(zip(U.ARGS, on_device(f)))
        g.update(changed)
        return ops.eval_drive(acc, *[g[k] for k in U.ARGS], rules=rules or f["kw"]["rules"], nbins=nbins)

    z = lambda *shape, dtype=torch.float32, device=DEV: torch.zeros(shape, dtype=dtype, device=device)
    bad = [dict(ego_plan=z(U.T, 3)), dict(ego_cast=z(U.T - 1, 2)), dict(ego_locs=z(U.T, 2)), dict(ego_plan=z(U.T, 2, dtype=torch.float64)),
           dict(ego_plan=z(1, 2), ego_cast=z(1, 2), ego_locs=z(2, 2)), dict(ego_plan=z(65, 2), ego_cast=z(65, 2), ego_locs=z(66, 2)),
           dict(ego_locs=torch.from_numpy(f["ego_locs"])), dict(locs=torch.from_numpy(f["locs"])), dict(typs=z(10, dtype=torch.int64)), dict(typs=z(9, dtype=torch.int32)),
           dict(locs=z(65, U.T + 1, 2), typs=z(65, dtype=torch.int32)), dict(locs=z(10, U.T, 2)), dict(n=11), dict(n=-1), dict(cmd=6), dict(cmd=-1), dict(bra=2),
           dict(bra=-1), dict(other_cast=z(3, 6, U.T + 1, 2)), dict(other_cmds=z(2, 6)), dict(other_cmds=None), dict(other_cast=z(3, 6, U.T, 2, device="cpu")),
           dict(other_cast=z(65, 6, U.T, 2), other_cmds=z(65, 6)), dict(other_cmds=z(3, 6, dtype=torch.float16)),
           dict(rules=E.DriveRules(aim_point=(4, 4, 4, 3, 6, U.T))), dict(nbins=0), dict(nbins=1025), dict(nbins=32), dict(acc=acc[:-1]), dict(acc=acc.cpu()),
           dict(acc=acc.to(torch.int32))]
    for changed in bad:
        with pytest.raises(ValueError):
            call(**changed)
    assert int(acc.abs().sum()) == 0
    call()
    assert int(acc[0]) == 1


def test_no_vehicles_as_none_as_empty_tensors_and_as_cpu_zeros():
    f = U.random_frame(11, N=0)
    want = spec(f)
    args = dict(zip(U.ARGS, on_device(f)))
    for cast, cmds in ((None, None), (torch.zeros((0, 6, U.T, 2), device=DEV), torch.zeros((0, 6), device=DEV)),
                       (torch.zeros((0, 6, U.T, 2)), torch.zeros((0, 6)))):
        g = dict(args, other_cast=cast, other_cmds=cmds)
        acc = torch.zeros(len(want), dtype=torch.int64, device=DEV)
        np.testing.assert_array_equal(ops.eval_drive(acc, *[g[k] for k in U.ARGS], **f["kw"]).cpu().numpy(), want)


@pytest.fixture(scope="module")
def three_frames():
    from lav_amd.train.synthetic import synthetic_lidar_batch
    from tests.util import build_models
    return build_models(DEV), synthetic_lidar_batch(3, seed=5, max_points=20000)


def test_evaluator_adds_the_same_counters_on_the_device_and_on_the_host(three_frames):
    """DriveEvaluator over three synthetic frames: the accumulator in HBM (the kernel) and on the host (the specification, on copies of
    the frame's tensors) end equal, the brake labels are the batch's, and the counters re-summarise."""
    models, batch = three_frames
    on_gpu, on_host = E.DriveEvaluator(models), E.DriveEvaluator(models, device="cpu")
    assert on_gpu.run([batch]) == on_host.run([batch]) == 3
    assert on_gpu.acc.is_cuda and not on_host.acc.is_cuda and len(on_gpu.acc) == len(E.DriveLayout(64))
    np.testing.assert_array_equal(on_gpu.counters(), on_host.counters())
    lay, acc = on_gpu.layout, on_gpu.counters()
    assert lay.view(acc, "frames").item() == 3
    finite = 3 - lay.view(acc, "plan_nonfinite").item()
    assert lay.view(acc, "cause").sum() == lay.view(acc, "gt_cause").sum() == lay.view(acc, "speed_hist").sum() == finite
    assert on_gpu._batch["bras"] == [int(b != 0) for b in batch[9].tolist()]
    m = E.summarise(acc, on_gpu.num_plan)
    assert m["frames"] == 3 and m == E.summarise(lay.unnamed(json.loads(json.dumps(lay.named(acc)))), on_gpu.num_plan)


def test_eval_full_counts_what_it_counted_before_the_split(three_frames):
    """Evaluator.frame is forward + metrics now: two Evaluators and a DriveEvaluator in between, in one process, on the same frames - the
    eval_full counters of the two runs are equal word for word, and equal to the specification's on the host."""
    models, batch = three_frames
    first = F.Evaluator(models)
    assert first.run([batch]) == 3
    assert E.DriveEvaluator(models).run([batch]) == 3
    second, on_host = F.Evaluator(models), F.Evaluator(models, device="cpu")
    for i in range(second.upload(batch)):                   # the two halves by hand: what frame() does
        second.metrics(i, second.forward(i))
    assert on_host.run([batch]) == 3
    np.testing.assert_array_equal(first.counters(), second.counters())
    np.testing.assert_array_equal(first.counters(), on_host.counters())
    assert F.summarise(first.counters())["frames"] == 3


def test_command_line_synthetic(capsys):
    lines = E.main(["--synthetic", "--frames", "2", "--precision", "f16x3", "--max-points", "20000", "--brake-speed", "0.25"])
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == len(printed) == 1
    line = printed[0]
    assert line["what"] == "eval_drive" and line["precision"] == "f16x3" and line["camera_brake"] == "not evaluated"
    assert line["rules"] == E.DriveRules(brake_speed=0.25).named() and line["summary"]["frames"] == 2
    assert line["summary"] == json.loads(json.dumps(E.summarise(E.DriveLayout(64).unnamed(line["counters"]), 20)))
