"""Resumable training state (--state-dir / --resume of the four trainers) and the decision that ends an unhealthy run.

A state file holds what a run needs to go on as if it had never stopped: the models the trainer saves, the optimiser's and the
scheduler's state_dicts, the iteration counters (`global_it` drives other_weight_schedule and the log cadence), every Augmenter's count,
every rank's random generators, and the arguments that define the run - a resume under other ones is refused.  State is taken at
epoch boundaries only: inside an epoch of a shuffled loader there is no position to come back to."""
from __future__ import annotations

import os
import random
import re

import numpy as np
import torch
import torch.distributed as dist

FORMAT = 1
KEEP = 2                    # state files kept in --state-dir
_SHARED = ("batch_size", "seed", "lr", "synthetic", "steps_per_epoch", "augment", "fused_optim", "max_grad_norm", "ema")
_OWN = {"bev": ("perceive_only", "motion_only", "max_points", "bev_on_device", "deterministic"), "seg": (), "bra": ()}
_OWN["lidar"] = _OWN["bev"]


def defining_args(what, args, world):
    """The arguments that define a run: global batch, world size, seed, lr, the data switches, the optimiser's, the trainer's own."""
    out = dict(what=what, world=int(world))
    for k in _SHARED + _OWN[what]:
        out[k] = getattr(args, k, None)
    return out


def _module(trainer, name):
    return getattr(trainer, {"bev": "bev_planner", "lidar": "lidar_model", "uniplanner": "uniplanner", "seg": "seg_model", "bra": "bra_model"}[name])


def _saves(trainer, what):
    return {"bev": ("bev",), "lidar": ("lidar", "uniplanner"), "seg": ("seg",), "bra": ("bra",)}[what]


def _rng_state(device):
    out = dict(torch=torch.get_rng_state(), numpy=np.random.get_state(), random=random.getstate())
    if torch.device(device).type == "cuda":
        out["cuda"] = torch.cuda.get_rng_state(device)
    return out


def _set_rng_state(st, device):
    torch.set_rng_state(st["torch"])
    np.random.set_state(st["numpy"])
    random.setstate(st["random"])
    if torch.device(device).type == "cuda" and "cuda" in st:
        torch.cuda.set_rng_state(st["cuda"], device)


def capture(trainer, what, args, epoch, global_it, augmenters, rank, world):
    """The state after `epoch` epochs (1-based: the run goes on with epoch + 1) as a dict of tensors and plain values.  With world > 1
    EVERY rank calls this (the ranks' generator states are gathered with all_gather_object); the models, the optimiser and the counters
    are rank 0's, which data parallel keeps equal on all of them."""
    rng = _rng_state(trainer.device)
    if world > 1:
        every = [None] * world
        dist.all_gather_object(every, rng)
        rng = every
    else:
        rng = [rng]
    sched = getattr(trainer, f"{what}_scheduler", None)
    return dict(format=FORMAT, what=what, epoch=int(epoch), global_it=int(global_it), steps=int(trainer.steps),
                models={name: trainer.state_dict(name) for name in _saves(trainer, what)},
                optimizer=getattr(trainer, f"{what}_optim").state_dict(), scheduler=None if sched is None else sched.state_dict(),
                augmenters=[int(a.count) for a in augmenters or ()], args=defining_args(what, args, world), rng=rng)


def restore(state, trainer, what, args, augmenters, rank, world):
    """capture's inverse, on every rank: returns (epoch, global_it).  A state of another format or trainer, or one whose defining
    arguments differ from this run's, ends the run with a SystemExit that names the key and both values."""
    if state.get("format") != FORMAT:
        raise SystemExit(f"--resume: state format {state.get('format')!r}, this build reads {FORMAT}")
    mine = defining_args(what, args, world)
    for k, v in mine.items():
        if state["args"].get(k) != v:
            raise SystemExit(f"--resume: the state was written with {k} = {state['args'].get(k)!r}, this run has {k} = {v!r}")
    for name, sd in state["models"].items():
        _module(trainer, name).load_state_dict(sd)
    getattr(trainer, f"{what}_optim").load_state_dict(state["optimizer"])
    sched = getattr(trainer, f"{what}_scheduler", None)
    if sched is not None:
        sched.load_state_dict(state["scheduler"])
    trainer.steps = int(state["steps"])
    augmenters = list(augmenters or ())
    if len(augmenters) != len(state["augmenters"]):
        raise SystemExit(f"--resume: the state holds {len(state['augmenters'])} augmenter counts, this run has {len(augmenters)} augmenters")
    for a, n in zip(augmenters, state["augmenters"]):
        a.count = int(n)
    _set_rng_state(state["rng"][rank], trainer.device)
    return int(state["epoch"]), int(state["global_it"])


def state_files(state_dir):
    """[(epoch, path)] of DIR/state_{epoch}.th, oldest first."""
    if not state_dir or not os.path.isdir(state_dir):
        return []
    found = []
    for f in os.listdir(state_dir):
        m = re.fullmatch(r"state_(\d+)\.th", f)
        if m:
            found.append((int(m.group(1)), os.path.join(state_dir, f)))
    return sorted(found)


def newest(state_dir):
    files = state_files(state_dir)
    return files[-1][1] if files else None


def write(state, state_dir):
    """DIR/state_{epoch}.th through a temporary file and os.replace (a killed job never leaves half a file); keeps the KEEP newest."""
    os.makedirs(state_dir, exist_ok=True)
    path = os.path.join(state_dir, f"state_{state['epoch']}.th")
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        torch.save(state, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)
    for _, old in state_files(state_dir)[:-KEEP]:
        os.remove(old)
    return path


def load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def _blamed(records):
    return ", ".join(f"{r['name']} ({r['nonfinite']}" + (f" at iteration {r['global_it']})" if r.get("global_it") is not None else ")") for r in records)


def check_health(health, skipped_at_last_log, max_skipped_steps, state_dir, blame=None):
    """What the trainers' main asks on every log iteration: ends the run (SystemExit, a non-zero exit) when a watched buffer holds a
    value that is not finite, or when more than max_skipped_steps steps were skipped since the last log iteration; the message names the
    newest state file to --resume from, or says that there is none.  Otherwise returns the skipped count to remember.
    blame (--tensor-stats): ([tensors], [watched buffers]) of records name, nonfinite, global_it - the messages then name them."""
    why = None
    if health["watch_nonfinite"]:
        why = f"{health['watch_nonfinite']} values of the watched buffers (BatchNorm running statistics) are not finite"
        if blame is not None and blame[1]:
            why += f": {_blamed(blame[1])}"
    elif health["skipped"] - skipped_at_last_log > max_skipped_steps:
        why = (f"{health['skipped'] - skipped_at_last_log} optimiser steps were skipped for gradients that are not finite since the last log "
               f"iteration (--max-skipped-steps {max_skipped_steps})")
        if blame is not None and blame[0]:
            why += f": {_blamed(blame[0])}"
    if why is None:
        return health["skipped"]
    last = newest(state_dir)
    raise SystemExit(f"training stopped: {why}; " + (f"--resume {last} continues from the newest state file" if last else
                                                     "there is no state file to --resume from (run with --state-dir)"))
