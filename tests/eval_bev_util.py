"""Seeded builders of small batches for the teacher-evaluation tests (tests/test_eval_bev_host.py, tests/test_gpu_eval_bev.py).

A scene is a dict of eval_plans' positional arguments after the accumulator (NumPy arrays; the three `other_*` are None for K = 0).
Coordinates are small multiples of 2^-20 or of 1/4, so that every distance the hand-derived tests name is exact in float32."""
from __future__ import annotations

import numpy as np

ARGS = ("ego_plan", "ego_cast", "ego_cmds", "ego_locs", "cmds", "bras", "other_cast", "other_cmds", "other_locs")
Q = 1 << 20
T, I = 20, 5


def positional(s):
    return [s[k] for k in ARGS]


def blank(B=1, K=0, T=T, I=I, cmd=2):
    """Every stage of every frame and every mode of every forecast ON its target; the command scores point at the command (ego) and
    fall from mode 0 (others); nobody brakes."""
    t = np.arange(T + 1, dtype=np.float32)
    ego_locs = np.tile(np.stack([0.25 * t, -0.5 * t], axis=-1)[None], (B, 1, 1)).astype(np.float32)
    target = ego_locs[:, 1:]
    ego_cmds = np.zeros((B, 6), np.float32)
    ego_cmds[:, cmd] = 1.0
    s = dict(ego_plan=np.tile(target[:, None, None], (1, I, 6, 1, 1)), ego_cast=np.tile(target[:, None], (1, 6, 1, 1)), ego_cmds=ego_cmds,
             ego_locs=ego_locs, cmds=np.full(B, cmd, np.int32), bras=np.zeros(B, np.uint8), other_cast=None, other_cmds=None, other_locs=None)
    if K:
        s["other_locs"] = np.tile(np.stack([-0.25 * t[1:], 0.75 * t[1:]], axis=-1)[None], (K, 1, 1)).astype(np.float32)
        s["other_cast"] = np.tile(s["other_locs"][:, None], (1, 6, 1, 1))
        s["other_cmds"] = np.tile(np.arange(6, 0, -1, dtype=np.float32) / 8, (K, 1))
    return s


def scene_345():
    """One frame, one forecast: every stage and every mode 3 m right and 4 m ahead of its target at every step - 5 m, held for T steps."""
    s = blank(1, 1)
    for k in ("ego_plan", "ego_cast", "other_cast"):
        s[k] = s[k] + np.array([3.0, 4.0], np.float32)
    return s


def scene_ties():
    """Targets at the origin; the cast 1.5 quanta and every plan stage 2.5 quanta from it along x: both round to 2 (ties to even).  The
    forecast's modes are 0.5, 1.5, 2.5, 3.5, 4.5 and 5.5 quanta off: 0, 2, 2, 4, 4, 6."""
    s = blank(1, 1)
    s["ego_locs"][:] = 0
    s["other_locs"][:] = 0
    for k in ("ego_plan", "ego_cast", "other_cast"):
        s[k][:] = 0
    s["ego_cast"][..., 0] = 1.5 / Q
    s["ego_plan"][..., 0] = 2.5 / Q
    for m in range(6):
        s["other_cast"][0, m, :, 0] = (m + 0.5) / Q
    return s


def scene_identical_modes():
    """Two forecasts.  0: modes 1 and 3 identical and nearest (0.25 m off), the scores' maximum on mode 3 - the min mode is 1, the FIRST.
    1: every mode 1 m off but mode 4 (0.5 m), the scores' maximum twice (modes 2 and 5) - the top mode is 2, the FIRST."""
    s = blank(1, 2)
    s["other_cast"][:, :, :, 1] += 1.0
    s["other_cast"][0, 1] = s["other_cast"][0, 3] = s["other_locs"][0] + np.array([0.25, 0.0], np.float32)
    s["other_cmds"][0] = (0.1, 0.2, 0.3, 0.9, 0.4, 0.5)
    s["other_cast"][1, 4] = s["other_locs"][1] + np.array([0.0, 0.5], np.float32)
    s["other_cmds"][1] = (0.1, 0.2, 0.7, 0.3, 0.4, 0.7)
    return s


def scene_nan_scores():
    """A NaN among the command scores counts as the maximum: frame 0 (command 2) has it at 4, frame 1 (command 1) at 1 behind a larger
    finite score; the forecast has two, at 3 and 5 - the first wins."""
    s = blank(2, 1)
    s["cmds"][:] = (2, 1)
    s["ego_cmds"][0] = (0.1, 0.2, 0.9, 0.3, np.nan, 0.4)
    s["ego_cmds"][1] = (0.99, np.nan, 0.1, 0.1, 0.1, 0.1)
    s["other_cmds"][0] = (0.9, 0.1, 0.1, np.nan, 0.1, np.nan)
    return s


def scene_nan_stage():
    """Two frames of command 3, the second braking.  Frame 0: a NaN at the last waypoint of plan iteration 1 (stage 2) only.  Frame 1: an
    Inf in the cast (stage 0) only - and in a command that is not the frame's, which nobody reads.  One forecast with a NaN in mode 5."""
    s = blank(2, 2, cmd=3)
    s["bras"][1] = 1
    s["ego_plan"][0, 1, 3, -1, 0] = np.nan
    s["ego_cast"][1, 3, 0, 1] = np.inf
    s["ego_plan"][1, :, 0, :, :] = np.nan
    s["other_cast"][1, 5, 7, 0] = np.nan
    return s


def scene_bad_cmds():
    """Three frames: commands 6, -1 and 0.  The first two touch `frames` and `bad_cmd` only, whatever their tensors hold."""
    s = blank(3, 0, cmd=0)
    s["cmds"][:] = (6, -1, 0)
    s["ego_plan"][:2] += 9.0
    s["ego_cmds"][:2] = np.nan
    return s


def random_batch(seed, B=5, K=7, T=T, I=I):
    """A seeded batch with everything in it: commands mostly valid, a few not; some frames brake; a stage or a mode with a NaN or an Inf
    now and then; forecasts with identical modes and tied scores."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32)
    ego_locs = f32(np.cumsum(rng.normal(0, 1, (B, T + 1, 2)), axis=1))
    s = dict(ego_plan=f32(ego_locs[:, None, None, 1:] + rng.normal(0, 2, (B, I, 6, T, 2))), ego_cast=f32(ego_locs[:, None, 1:] + rng.normal(0, 3, (B, 6, T, 2))),
             ego_cmds=f32(rng.random((B, 6))), ego_locs=ego_locs, cmds=rng.integers(0, 6, B).astype(np.int32), bras=(rng.random(B) < 0.3).astype(np.uint8),
             other_cast=None, other_cmds=None, other_locs=None)
    for b in range(B):
        r = rng.random()
        if r < 0.1:
            s["cmds"][b] = rng.choice([-1, 6, 1 << 20, -(1 << 31)])
        elif r < 0.25:
            s["ego_plan"][b, rng.integers(I), s["cmds"][b], rng.integers(T), rng.integers(2)] = rng.choice([np.nan, np.inf, -np.inf])
        elif r < 0.35:
            s["ego_cast"][b, s["cmds"][b], rng.integers(T), rng.integers(2)] = rng.choice([np.nan, np.inf])
        if rng.random() < 0.2:
            s["ego_cmds"][b, rng.integers(6)] = np.nan
        if rng.random() < 0.2:
            s["ego_cmds"][b, rng.integers(6)] = s["ego_cmds"][b].max()
    if K:
        s["other_locs"] = f32(np.cumsum(rng.normal(0, 1, (K, T, 2)), axis=1))
        s["other_cast"] = f32(s["other_locs"][:, None] + rng.normal(0, 2, (K, 6, T, 2)))
        s["other_cmds"] = f32(rng.random((K, 6)))
        for k in range(K):
            r = rng.random()
            if r < 0.15:
                s["other_cast"][k, rng.integers(6), rng.integers(T), rng.integers(2)] = rng.choice([np.nan, np.inf])
            elif r < 0.4:
                a, b = rng.choice(6, 2, replace=False)
                s["other_cast"][k, a] = s["other_cast"][k, b]
            if rng.random() < 0.2:
                s["other_cmds"][k, rng.integers(6)] = np.nan
            if rng.random() < 0.2:
                s["other_cmds"][k, rng.integers(6)] = s["other_cmds"][k].max()
    return s


def concat(a, b):
    """The batch of a's frames and forecasts followed by b's."""
    out = {k: np.concatenate([a[k], b[k]]) for k in ARGS[:6]}
    for k in ARGS[6:]:
        parts = [x[k] for x in (a, b) if x[k] is not None]
        out[k] = np.concatenate(parts) if parts else None
    return out


def take(s, frames, forecasts):
    """The sub-batch of the given frames and forecasts (index lists), in that order."""
    out = {k: s[k][list(frames)] for k in ARGS[:6]}
    for k in ARGS[6:]:
        out[k] = s[k][list(forecasts)] if s[k] is not None and len(forecasts) else None
    return out


SCENES = dict(on_target=lambda: blank(3, 2), offset_345=scene_345, ties=scene_ties, identical_modes=scene_identical_modes,
              nan_scores=scene_nan_scores, nan_stage=scene_nan_stage, bad_cmds=scene_bad_cmds)
