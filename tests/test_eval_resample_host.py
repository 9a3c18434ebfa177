"""The eval tools' --bootstrap on the CPU: the draws of eval_resample_numpy (the specification of lav_eval_resample), EvaluatorBase's row
rule, the interval rule and the coverage of the intervals on rows of known mean.  The kernel against the specification and the seven
tools' lines are checked in tests/test_gpu_eval_resample.py."""
import argparse

import numpy as np
import pytest
import torch

from lav_amd.data.augment import philox4x32
from lav_amd.train import eval_common as C


# ------------------------------------------------------------------------------------------------------------ 1. the index rule
def one_hot_counts(B, seed, R=64):
    return C.eval_resample_numpy(np.eye(R, dtype=np.int64), B, seed)


def test_draws_are_philox_words_through_the_multiply_high_map():
    """Rows e_r make the replicates the draw counts.  Every replicate draws R rows, replicate 0 every row once; over 4096 replicates a
    row's total is Binomial(4096 * 64, 1 / 64): mean 4096, sigma = sqrt(4096 (1 - 1/64)) = 63.5, and every row lies within 5 sigma
    (the map's own bias, R / 2^32 of a row's share, is 1e-8 of that).  Seeds change the draws and repeat them."""
    B, R = 4096, 64
    out = one_hot_counts(B, 7)
    assert out.shape == (B + 1, R) and out.dtype == np.int64
    assert (out.sum(axis=1) == R).all() and (out >= 0).all()
    assert (out[0] == 1).all()
    sigma = np.sqrt(4096 * (1 - 1 / 64))
    assert (np.abs(out[1:].sum(axis=0) - 4096) <= 5 * sigma).all(), out[1:].sum(axis=0)
    assert (out[1:] != 1).any(axis=1).all()                                       # (64 draws that hit 64 different rows: 64! / 64^64)
    np.testing.assert_array_equal(one_hot_counts(64, 7), out[:65])                # the same seed, the same draws, whatever B is
    other = one_hot_counts(64, 8)
    assert (other[1:] != out[1:65]).any(axis=1).all()
    high = one_hot_counts(64, 7 + (1 << 32))                                      # the seed's high word is key word 1
    assert (high[1:] != out[1:65]).any(axis=1).all()


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 9, 1000])
def test_specification_equals_the_rule_word_by_word(R):
    """idx(b, j) = (u * R) >> 32 with u = word j & 3 of Philox4x32-10 at counter (j >> 2, b, 0x52534D50, 0), one draw at a time in Python
    integers; sums modulo 2^64 on values that reach 2^62."""
    B, W, seed = 5, 3, 0x1234567887654321
    rng = np.random.default_rng(R)
    rows = rng.integers(-(1 << 62), 1 << 62, (R, W), dtype=np.int64)
    got = C.eval_resample_numpy(rows, B, seed)
    want = np.zeros((B + 1, W), np.uint64)
    want[0] = rows.astype(np.uint64).sum(axis=0)
    for b in range(1, B + 1):
        for j in range(R):
            u = int(philox4x32(j >> 2, b, 0x52534D50, 0, seed)[j & 3])
            idx = (u * R) >> 32
            assert 0 <= idx < R
            want[b] += rows[idx].astype(np.uint64)
    np.testing.assert_array_equal(got.view(np.uint64), want)


def test_specification_refuses_what_the_kernel_refuses():
    for bad in (np.zeros((0, 3), np.int64), np.zeros((3, 0), np.int64), np.zeros(3, np.int64)):
        with pytest.raises(ValueError):
            C.eval_resample_numpy(bad, 2, 0)
    assert C.eval_resample_numpy(np.arange(6).reshape(2, 3), 0, 0).tolist() == [[3, 5, 7]]


# ------------------------------------------------------------------------------------------------------------ 2. the row rule
LAYOUT = C.AccLayout((("count", (1,)), ("sum", (1,)), ("phase", (5,))))
VALUES = np.random.default_rng(3).integers(0, 1000, 64)


def unit_spec(acc, first, count):
    """The stub's metrics `kernel`: units first .. first + count - 1."""
    for u in range(first, first + count):
        acc[0] += 1
        acc[1] += VALUES[u]
        acc[2 + u % 5] += 1


class Stub(C.EvaluatorBase):
    """`group` units per forward, `launches` launches per forward, on the host."""

    def __init__(self, group, launches=1):
        super().__init__(torch.nn.Linear(1, 1), LAYOUT, 1, "cpu")
        self.frames, self.group, self.launches = 0, group, launches

    def run(self, units):
        while self.frames < units:
            g = min(self.group, units - self.frames)
            for k in range(self.launches):                       # (a forward's launches land in one row: the units are split over them)
                first = self.frames + k * g // self.launches
                self._add(None, unit_spec, None, first, self.frames + (k + 1) * g // self.launches - first)
            self.frames += g
        return self.frames


def rows_by_the_rule(units, group, L):
    opened = []
    for u in range(0, units, group):
        if not opened or u - opened[-1] >= L:
            opened.append(u)
    return np.diff(opened + [units]).tolist()


HAND_ROWS = {(10, 1, 4): [4, 4, 2], (20, 8, 4): [8, 8, 4], (50, 8, 20): [24, 24, 2], (16, 8, 1): [8, 8], (3, 1, 1): [1, 1, 1],
             (45, 1, 20): [20, 20, 5], (24, 8, 8): [8, 8, 8], (16, 1, 8): [8, 8], (16, 1, 4): [4, 4, 4, 4], (16, 8, 4): [8, 8]}


@pytest.mark.parametrize("group", [1, 8])
@pytest.mark.parametrize("L", [1, 4, 8, 20])
@pytest.mark.parametrize("units", [1, 16, 50])
def test_row_rule(units, group, L):
    plain = Stub(group)
    plain.run(units)
    assert plain.table is None and tuple(plain.acc.shape) == (len(LAYOUT),)
    ev = Stub(group, launches=3)
    ev.resample(L, units)
    assert tuple(ev.table.shape) == (-(-units // L), len(LAYOUT)) and ev.table.dtype == torch.int64 and int(ev.table.abs().sum()) == 0
    assert ev.acc.is_contiguous() and ev.acc.data_ptr() == ev.table.data_ptr()
    assert ev.run(units) == units
    table, row_units = ev.row_table()
    want = rows_by_the_rule(units, group, L)
    assert row_units.tolist() == want and sum(want) == units
    assert all(L <= n <= L + group - 1 for n in want[:-1]) and 1 <= want[-1] <= L + group - 1
    if (units, group, L) in HAND_ROWS:
        assert want == HAND_ROWS[units, group, L]
    table = table.numpy()
    assert table.shape[0] == len(want) and (table[:, 0] == want).all()                      # no row is empty: each counts its units
    np.testing.assert_array_equal(ev.counters(), plain.counters())                           # the column sums, in the same bits
    np.testing.assert_array_equal(table.sum(axis=0), plain.counters())
    assert int(ev.table[len(want):].abs().sum()) == 0
    np.testing.assert_array_equal(ev.replicates(3, 5), C.eval_resample_numpy(table, 3, 5))
    np.testing.assert_array_equal(ev.replicates(3, 5)[0], plain.counters())


def test_hand_rows_are_all_reached():
    for (units, group, L), want in HAND_ROWS.items():
        assert rows_by_the_rule(units, group, L) == want
        ev = Stub(group)
        ev.resample(L, units)
        ev.run(units)
        assert ev.row_table()[1].tolist() == want


def test_resample_refuses_tables_it_cannot_hold():
    ev = Stub(1)
    with pytest.raises(ValueError, match="--block"):
        ev.resample(1, (1 << 20) + 1)                                  # more than 2^20 rows
    big = Stub(1)
    big.layout = C.AccLayout((("wide", (1 << 16,)),))
    with pytest.raises(ValueError, match="--block"):
        big.resample(1, 1 << 14)                                       # 2^14 rows of 2^16 words: 8 GiB
    with pytest.raises(ValueError):
        ev.resample(0, 10)
    assert ev.table is None
    ev.resample(4, 4)                                                  # told of 4 units, given 9
    with pytest.raises(RuntimeError, match="resample"):
        ev.run(9)


# ------------------------------------------------------------------------------------------------------------ 3. the interval rule
def test_interval_rule_on_hand_made_lists():
    ten = [7, 3, 10, 1, 5, 9, 2, 8, 6, 4]                                                   # sorted: 1 .. 10
    assert C.interval(ten, 10, 0.95) == [1.0, 10.0]                                          # floor(0.025 * 9) = 0, ceil(0.975 * 9) = 9
    assert C.interval(ten, 10, 0.5) == [3.0, 8.0]                                            # floor(0.25 * 9) = 2, ceil(0.75 * 9) = 7
    assert C.interval(range(41), 41, 0.95) == [1.0, 39.0]                                    # 0.025 * 40 = 1 and 0.975 * 40 = 39 exactly
    assert C.interval(range(401), 401, 0.95) == [10.0, 390.0]
    assert C.interval(range(400), 400, 0.95) == [9.0, 390.0]                                 # floor(9.975), ceil(389.025)
    assert C.interval(range(1000), 1000, 0.9) == [49.0, 950.0]                               # floor(49.95), ceil(949.05)
    assert C.interval(ten[:7], 10, 0.95) == [1.0, 10.0, 7]                                   # B / 2 <= n < B: [lo, hi, n]; 1 .. 10 without 4, 6, 8
    assert C.interval(ten[:5], 10, 0.95) == [1.0, 10.0, 5]                                   # n = B / 2 is enough
    assert C.interval(ten[:4], 10, 0.95) is None                                             # n < B / 2
    assert C.interval([], 10, 0.95) is None and C.interval([], 0, 0.95) is None
    assert C.interval([2.5], 1, 0.95) == [2.5, 2.5]


def test_interval_tree_has_the_summarys_shape_and_its_float_leaves_only():
    point = dict(frames=3, ok=True, name="x", ade=0.5, never=None, iou=[0.1, None], labelled=[1, 2], mixed=[0.5, 3], rows=[dict(a=1.0, n=2)])
    reps = [dict(point, ade=0.5 + b, never=None, iou=[0.1 * b, None if b % 4 else 1.0], rows=[dict(a=float(b), n=2)]) for b in range(1, 9)]
    ci = C.interval_tree(point, reps, 8, 0.95)
    assert ci == dict(ade=[1.5, 8.5], never=None, iou=[[0.1, 0.8], None], mixed={"0": [0.5, 0.5]}, rows=[dict(a=[1.0, 8.0])])
    reps[0]["iou"][1] = reps[1]["iou"][1] = 2.0                                              # defined in 4 of 8 replicates
    assert C.interval_tree(point, reps, 8, 0.95)["iou"][1] == [1.0, 2.0, 4]
    # a paired difference: replicate b against replicate b, over the leaves both sides have
    other = dict(ade=0.25, iou=[0.2], extra=1.0)
    others = [dict(ade=0.25 + b, iou=[0.1 * b], extra=1.0) for b in range(1, 9)]
    diff = C.interval_tree(point, reps, 8, 0.95, minus=(other, others))
    assert diff == dict(ade=[0.25, 0.25], iou={"0": [0.0, 0.0]})


def test_the_flags_are_run_clis_own_and_block_names_the_correlation_length():
    ap = argparse.ArgumentParser()
    C._resample_flags(ap, "frames")
    args = ap.parse_args([])
    assert (args.bootstrap, args.block, args.level, args.rows_out) == (0, 32, 0.95, None)
    assert "correlation length" in " ".join(ap.format_help().split())
    from lav_amd.train import evaluate_det, evaluate_distill
    assert evaluate_det.TOOL["contrasts"] == (("dense", "peaks"),) and evaluate_distill.TOOL["contrasts"] == (("student", "teacher"),)
    for tool in (evaluate_det.TOOL, evaluate_distill.TOOL):
        assert "--bootstrap" not in C.parser(tool).format_help()                            # parser(tool) is the tool's, as it was


# ------------------------------------------------------------------------------------------------------------ 4. coverage
COVERAGE_SEED = 20261021          # trial t draws its rows and its replicates from COVERAGE_SEED + t


def test_intervals_cover_a_known_mean():
    """Rows [count = 1, sum = x_r], x_r i.i.d. uniform on 0 .. 99 (mean 49.5), R = 100 blocks, B = 400 replicates, 200 trials: the 95 %
    interval of sum / count covers 49.5 in a share of the trials between 0.88 and 0.99 - nominal 0.95, binomial sd 0.016, and room below
    for the percentile bootstrap's known under-coverage at R = 100.  Observed with these seeds: see DESIGN 4.7n."""
    R, B, trials, mean = 100, 400, 200, 49.5
    covered = 0
    for t in range(trials):
        rows = np.stack([np.ones(R, np.int64), np.random.default_rng(COVERAGE_SEED + t).integers(0, 100, R)], axis=1)
        out = C.eval_resample_numpy(rows, B, COVERAGE_SEED + t)
        assert (out[:, 0] == R).all()
        lo, hi = C.interval((out[1:, 1] / out[1:, 0]).tolist(), B, 0.95)
        covered += lo <= mean <= hi
    share = covered / trials
    print(f"coverage: {covered} of {trials} = {share}")
    assert 0.88 <= share <= 0.99, share
