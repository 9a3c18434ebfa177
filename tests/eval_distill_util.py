"""Seeded builders of small student / teacher batches for the distillation-evaluation tests (tests/test_eval_distill_host.py,
tests/test_gpu_eval_distill.py).

A scene is a dict of eval_distill's positional arguments after the accumulator (NumPy arrays; the five forecast tensors are None for
K = 0), made of two eval_bev_util scenes - the student's and the teacher's outputs - over the same ego_locs, cmds and other_locs.
Coordinates are small multiples of 2^-20 or of 1/4, so that every distance the hand-derived tests name is exact in float32."""
from __future__ import annotations

import numpy as np

from tests import eval_bev_util as B

ARGS = ("s_ego_plan", "s_ego_cast", "s_ego_cmds", "t_ego_plan", "t_ego_cast", "t_ego_cmds", "ego_locs", "cmds", "s_other_cast", "s_other_cmds",
        "t_other_cast", "t_other_cmds", "other_locs")
FRAME_ARGS, FORECAST_ARGS = ARGS[:8], ARGS[8:]
Q = 1 << 20
T, I = B.T, B.I


def positional(s):
    return [s[k] for k in ARGS]


def pair(student, teacher):
    """The scene of two eval_bev_util scenes; the targets and commands are the student scene's."""
    copy = lambda a: None if a is None else a.copy()
    s = {("s_" + k): copy(student[k]) for k in ("ego_plan", "ego_cast", "ego_cmds", "other_cast", "other_cmds")}
    s.update({("t_" + k): copy(teacher[k]) for k in ("ego_plan", "ego_cast", "ego_cmds", "other_cast", "other_cmds")})
    s.update(ego_locs=student["ego_locs"].copy(), cmds=student["cmds"].copy(), other_locs=copy(student["other_locs"]))
    return s


def blank(Bn=1, K=0, T=T, I=I, cmd=2):
    """Both arms ON their targets in every stage and mode, with the same scores (eval_bev_util.blank twice)."""
    return pair(B.blank(Bn, K, T, I, cmd), B.blank(Bn, K, T, I, cmd))


def at_origin(Bn=1, K=0, T=T, I=I, cmd=2):
    """blank with every target and every waypoint at the origin, so that offsets of a few quanta are exact."""
    s = blank(Bn, K, T, I, cmd)
    for k in ARGS:
        if s[k] is not None and k not in ("cmds", "s_ego_cmds", "t_ego_cmds", "s_other_cmds", "t_other_cmds"):
            s[k][:] = 0
    return s


def scene_identical():
    """Three frames and two forecasts, the student's outputs the teacher's, 3 m right and 4 m ahead of every target."""
    s = blank(3, 2)
    for k in ("ego_plan", "ego_cast", "other_cast"):
        s["s_" + k] += np.array([3.0, 4.0], np.float32)
        s["t_" + k] += np.array([3.0, 4.0], np.float32)
    return s


def scene_one_quantum():
    """Two frames of command 2 at the origin.  Frame 0: at its last waypoint the student's commanded mode is 1 quantum and the
    teacher's 2 quanta off, in every stage - the student is closer by one quantum, the gap is one quantum.  Frame 1: the teacher's is on
    target and the student's 1 quantum off in the cast only - the teacher is closer there, the plan stages tie.  One forecast: the student's
    mode 4 is 1 quantum off at every step, its other modes and all of the teacher's 3 quanta - the student's min mode is closer by 2 T."""
    s = at_origin(2, 1)
    s["s_ego_cast"][0, 2, -1, 0] = s["s_ego_plan"][0, :, 2, -1, 0] = 1.0 / Q
    s["t_ego_cast"][0, 2, -1, 0] = s["t_ego_plan"][0, :, 2, -1, 0] = 2.0 / Q
    s["s_ego_cast"][1, 2, -1, 1] = -1.0 / Q
    s["s_other_cast"][0, :, :, 0] = s["t_other_cast"][0, :, :, 0] = 3.0 / Q
    s["s_other_cast"][0, 4, :, 0] = 1.0 / Q
    return s


def scene_nonfinite():
    """Two frames of command 3, three forecasts.  Frame 0: a NaN at the last waypoint of the STUDENT's plan iteration 1 (stage 2), mode 3
    - that (stage, mode) gap is non-finite and stage 2 is unjudged.  Frame 1: an Inf in the TEACHER's cast, mode 0 - not the frame's
    command: a non-finite gap at stage 0, and stage 0 is still judged.  Forecast 1: a NaN in mode 5 of the teacher only.  Forecast 2: an
    infinite score in mode 1 of the student only."""
    s = blank(2, 3, cmd=3)
    s["s_ego_plan"][0, 1, 3, -1, 0] = np.nan
    s["t_ego_cast"][1, 0, 0, 1] = np.inf
    s["t_other_cast"][1, 5, 7, 0] = np.nan
    s["s_other_cmds"][2, 1] = np.inf
    return s


def scene_nan_scores():
    """Two frames.  Frame 0 (command 2): the student's scores have a NaN at mode 4 - its first maximum - and the teacher's none (top 2);
    the gap of mode 4 is non-finite.  Frame 1 (command 1): both have a NaN at mode 1 behind a larger finite score."""
    s = blank(2, 0)
    s["cmds"][:] = (2, 1)
    s["s_ego_cmds"][0] = (0.25, 0.25, 0.75, 0.25, np.nan, 0.5)
    s["t_ego_cmds"][0] = (0.25, 0.25, 0.75, 0.25, 0.25, 0.5)
    s["s_ego_cmds"][1] = s["t_ego_cmds"][1] = (0.75, np.nan, 0.25, 0.25, 0.25, 0.25)
    return s


def scene_bad_cmds():
    """Three frames: commands 6, -1 and 0.  The first two touch `frames` and `bad_cmd` only, whatever their tensors hold."""
    s = blank(3, 0, cmd=0)
    s["cmds"][:] = (6, -1, 0)
    s["s_ego_plan"][:2] += 9.0
    s["t_ego_cmds"][:2] = np.nan
    return s


def scene_ties():
    """One frame, two forecasts, at the origin.  The frame: the teacher's scores tie at modes 1 and 3 (top 1, the FIRST), the student's
    at 3 and 5 (top 3).  Forecast 0: the student's modes 1 and 3 are nearest and identical (min mode 1, the first), the teacher's modes
    3 and 4 (min mode 3) - the same sum, a tie - and the two arms' min modes differ.  Forecast 1: both arms' scores tie at modes 2 and 5
    (top 2), every mode 8 quanta off but the student's mode 2 (4 quanta): by top mode the student is closer, by min mode too."""
    s = at_origin(1, 2)
    s["t_ego_cmds"][0] = (0.25, 0.75, 0.5, 0.75, 0.25, 0.25)
    s["s_ego_cmds"][0] = (0.25, 0.25, 0.5, 0.75, 0.25, 0.75)
    s["s_other_cast"][:, :, :, 0] = s["t_other_cast"][:, :, :, 0] = 8.0 / Q
    s["s_other_cast"][0, 1, :, 0] = s["s_other_cast"][0, 3, :, 0] = 2.0 / Q
    s["t_other_cast"][0, 3, :, 0] = s["t_other_cast"][0, 4, :, 0] = 2.0 / Q
    s["s_other_cmds"][1] = s["t_other_cmds"][1] = (0.25, 0.25, 0.75, 0.5, 0.25, 0.75)
    s["s_other_cast"][1, 2, :, 0] = 4.0 / Q
    return s


def scene_single_waypoint():
    """T = 1, no forecasts: the sum is the final distance.  The student 1.5 quanta from the teacher (2, ties to even) in mode 0 of the cast."""
    s = at_origin(1, 0, T=1)
    s["s_ego_cast"][0, 0, 0, 0] = 1.5 / Q
    return s


def random_batch(seed, Bn=5, K=7, T=T, I=I):
    """A seeded batch with everything in it: two eval_bev_util.random_batch draws (bad commands, NaNs and infinities, identical modes,
    tied and NaN scores) over the student's targets; now and then a stage or a forecast of the teacher is the student's (ties, zero
    gaps) or a few quanta from it."""
    rng = np.random.default_rng(seed + 77)
    student, teacher = B.random_batch(seed, B=Bn, K=K, T=T, I=I), B.random_batch(seed + 1000, B=Bn, K=K, T=T, I=I)
    shift = (student["ego_locs"] - teacher["ego_locs"])[:, 1:]                  # the teacher's draw, moved onto the student's targets
    teacher["ego_plan"] += shift[:, None, None]
    teacher["ego_cast"] += shift[:, None]
    if K:
        teacher["other_cast"] += (student["other_locs"] - teacher["other_locs"])[:, None]
    s = pair(student, teacher)
    for b in range(Bn):
        r = rng.random()
        if r < 0.2:
            s["t_ego_cast"][b], s["t_ego_plan"][b] = s["s_ego_cast"][b], s["s_ego_plan"][b]
        elif r < 0.4:
            s["t_ego_cast"][b] = s["s_ego_cast"][b] + np.float32(rng.integers(-3, 4) / Q)
        if rng.random() < 0.3:
            s["t_ego_cmds"][b] = s["s_ego_cmds"][b]
    for k in range(K):
        r = rng.random()
        if r < 0.2:
            s["t_other_cast"][k] = s["s_other_cast"][k]
        elif r < 0.4:
            s["t_other_cast"][k] = s["s_other_cast"][k][::-1]
        if rng.random() < 0.3:
            s["t_other_cmds"][k] = s["s_other_cmds"][k]
    return s


def concat(a, b):
    """The batch of a's frames and forecasts followed by b's."""
    out = {k: np.concatenate([a[k], b[k]]) for k in FRAME_ARGS}
    for k in FORECAST_ARGS:
        parts = [x[k] for x in (a, b) if x[k] is not None]
        out[k] = np.concatenate(parts) if parts else None
    return out


def student_of(s):
    """eval_plans' positional arguments for the student arm of a scene (nobody brakes)."""
    return [s["s_ego_plan"], s["s_ego_cast"], s["s_ego_cmds"], s["ego_locs"], s["cmds"], np.zeros(len(s["cmds"]), np.uint8), s["s_other_cast"],
            s["s_other_cmds"], s["other_locs"]]


SCENES = dict(identical=scene_identical, one_quantum=scene_one_quantum, nonfinite=scene_nonfinite, nan_scores=scene_nan_scores,
              bad_cmds=scene_bad_cmds, ties=scene_ties, single_waypoint=scene_single_waypoint, on_target=lambda: blank(3, 2))
