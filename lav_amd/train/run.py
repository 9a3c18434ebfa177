"""Command-line driver shared by train_bev_v2.py / train_full_v2.py / train_seg.py / train_bra_v2.py and bench.py's training modes."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import time
from typing import Callable, Optional

import torch
import torch.distributed as dist

from . import log_view, state as run_state, tensor_stats
from .brake import BRA_LABELS, BrakeTrainer
from .lav import LAV, TrainConfig
from .optim import ema_state_dict
from .synthetic import synthetic_bev_batch, synthetic_bra_batch, synthetic_lidar_batch, synthetic_seg_batch


def setup_distributed():
    """(rank, world, device).  One process per GPU; RCCL ("nccl") on GPUs, gloo otherwise.  LAV_DIST_BACKEND=gloo forces
    gloo with HIP tensors (gradients hop through the host) and lets ranks share a GPU (local rank modulo the device count):
    how the data-parallel step over the HIP autograd functions is exercised on a one-GPU box (tests/test_gpu_train.py)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    cuda = torch.cuda.is_available()
    backend = os.environ.get("LAV_DIST_BACKEND") or ("nccl" if cuda else "gloo")
    if cuda:
        if backend == "gloo":
            local %= torch.cuda.device_count()
        torch.cuda.set_device(local)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(backend)
    return rank, world, torch.device("cuda", local) if cuda else torch.device("cpu")


def train_loop(what, global_batch, steps, warmup, cfg=None, max_points=None, log=None, profile_steps=0, device=None, wrap=None):
    """Runs warmup + steps optimisation steps on a fixed synthetic shard per rank; returns (seconds for `steps`, last info).
    profile_steps > 0: that many EXTRA steps after the timed region with the library's HIP-event timers armed; their per-kernel
    times and the algorithmic work lav_amd.ops counted over the same steps come back in info["hand_kernels"]."""
    rank, world, dev0 = setup_distributed()
    device = device if device is not None else dev0    # device=cpu: the same trainer on torch CPU ops (bench.py's cpu_baseline)
    cfg = cfg or TrainConfig()
    if global_batch % world:
        raise SystemExit(f"global batch {global_batch} is not divisible by {world} ranks")
    per_rank = global_batch // world
    torch.manual_seed(cfg.seed + rank)
    lav = LAV(cfg, device, what=what)
    if what == "bev":
        batch = synthetic_bev_batch(per_rank, seed=cfg.seed + 100 * rank, device=device)
        step = lambda: lav.train_bev(*batch, other_weight=cfg.other_weight)
    else:
        batch = synthetic_lidar_batch(per_rank, seed=cfg.seed + 100 * rank, max_points=max_points or cfg.max_lidar_points, device=device)
        step = lambda: lav.train_lidar(*batch)

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    if wrap is not None:      # a context manager factory over the trainer (bench.py's CPU leg swaps the teacher's kernels for torch ops)
        with wrap(lav):       # (host work: no device sync, no all-reduce of the time)
            return _run_steps(step, steps, warmup, rank, log) + ((rank, world),)
    dt, info = _run_steps(step, steps, warmup, rank, log, sync)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if profile_steps > 0 and device.type == "cuda":   # every rank steps (the gradient exchange needs them all)
        import ctypes
        from .. import _lib, ops
        lib = _lib.load()
        lib.lav_profile_enable(4096)
        lib.lav_profile_reset()
        for k in ops.train_work:
            ops.train_work[k] = 0
        for _ in range(profile_steps):
            step()
        torch.cuda.synchronize()
        kernels = {}
        for name in ("crop_rotate_backward", "crop_rotate", "gru_seq_forward", "gru_seq_backward", "gru_plan", "scatter_max", "pillar_decorate",
                     "bn_train_fwd", "bn_train_bwd", "conv_wgrad", "conv2d"):
            ms, n = ctypes.c_double(), ctypes.c_int()
            lib.lav_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(n))
            if n.value:
                kernels[name] = dict(calls_per_step=n.value / profile_steps, ms_per_call=ms.value / n.value, ms_per_step=ms.value / profile_steps)
        lib.lav_profile_enable(0)
        info = dict(info, hand_kernels=dict(kernels=kernels, work_per_step={k: v / profile_steps for k, v in ops.train_work.items()}))
    if world > 1:
        dist.barrier()
    return dt, info, (rank, world)


def _run_steps(step, steps, warmup, rank, log, sync=lambda: None):
    """train_loop's warm-up and timed loop: (seconds for `steps`, last info); `sync` brackets the timed region."""
    info = None
    for _ in range(warmup):
        info = step()
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        info = step()
        if log and rank == 0:
            log(i, info)
    sync()
    return time.perf_counter() - t0, info


def load_config(path, **overrides) -> TrainConfig:
    """TrainConfig from the reference's YAML (config_v2.yaml): every key that TrainConfig has is taken from the file,
    the others (data paths, controller gains ...) are not part of the training step.  `distill` is read by
    lav_final_v2.py:244 but absent from config_v2.yaml (team_code_v2/config.yaml:11 says True): injected as True."""
    import yaml
    fields = {f.name for f in dataclasses.fields(TrainConfig)}
    vals = {}
    if path:
        with open(path, "r") as f:
            raw = yaml.safe_load(f) or {}
        vals = {k: v for k, v in raw.items() if k in fields}
    vals.setdefault("distill", True)
    vals.update({k: v for k, v in overrides.items() if v is not None})
    return TrainConfig(**vals)


def resolve_checkpoints(what, args):
    """Which checkpoints a run starts from.  Command-line paths win; otherwise a run on recorded routes follows the reference's
    rules for the *_model_dir keys of config_v2.yaml (lav/lav_final_v2.py:42-72): the privileged teacher `bev_model_dir` is
    ALWAYS loaded by train_full_v2, `lidar_model_dir` unless --perceive-only, `uniplanner_dir` unless --perceive-only or
    --motion-only; train_bev_v2 starts from scratch.  A missing file is an error there, never a silent fall back to seeded random
    weights (that is what --synthetic runs use, explicitly)."""
    paths = dict(lidar=args.lidar, bev=args.bev, uniplanner=args.uniplanner)
    if args.synthetic or not args.config_path or what != "lidar":
        return paths
    from .eval_common import config_checkpoint
    wanted = dict(bev="bev_model_dir")
    if not args.perceive_only:
        wanted["lidar"] = "lidar_model_dir"
        if not args.motion_only:
            wanted["uniplanner"] = "uniplanner_dir"
    for name, key in wanted.items():
        if not paths[name]:
            paths[name] = config_checkpoint(args.config_path, key, name, None, False, "to train seeded random weights on synthetic batches",
                                            why=": train_full_v2 loads it (lav/lav_final_v2.py:42-72)")
    return paths


def set_deterministic(on: bool = True):
    """Run-to-run bit reproducibility of a training step.  liblav_amd's kernels (pillar front end, scatter-max, crop gather,
    GRU tape, BatchNorm) reduce in a fixed order; what differs between two runs of the default configuration is torch's own
    atomics-based backward kernels and MIOpen's algorithm choice (tools/determinism_probe.py: already the forward loss of step 0
    differs by 3e-7, 181 of 189 parameter gradients after it).  With these switches two runs agree bit for bit."""
    torch.backends.cudnn.deterministic = bool(on)
    if on:
        torch.backends.cudnn.benchmark = False
    # Round 6: reproducible from PROCESS to process too.  With benchmark off torch still lets MIOpen "find" - time the applicable solvers and
    # keep the fastest -, so which (deterministic) solver a layer gets is a measurement, and two processes on one box disagreed about once in
    # three starts (tools/determinism_xproc.py: the first difference at step 0, 1 or 2; inside a process 24 of 24 repeats of step 0 agree).
    # MIOpen's immediate mode takes the solver from its database / heuristic instead of a timing.
    mi = getattr(torch.backends, "miopen", None)
    if mi is not None and hasattr(mi, "immediate"):
        mi.immediate = bool(on)
    torch.use_deterministic_algorithms(bool(on), warn_only=True)


def other_weight_schedule(it, beta=0.8):
    """lav/train_bev_v2.py:38-39"""
    return 1 - beta ** (it / 4000)


def _augmenters(args, rank, world, streams):
    """--augment PROB > 0: one lav_amd.data.augment.Augmenter per image stream (stream tags 0, 1, ...), every rank with its own sample
    ids; None for 0 (nothing changes: no uint8 upload, no launch)."""
    if not 0.0 <= args.augment <= 1.0:
        raise SystemExit(f"--augment {args.augment}: a probability")
    if args.augment == 0.0:
        return None
    from ..data.augment import Augmenter
    return [Augmenter(args.augment, seed=args.seed, rank=rank, world=world, stream_tag=t) for t in range(streams)]


def _as_u8_hwc(rgb):
    """(B, H, W, 3) uint8 of a batch of images, whatever dtype they arrive in (the loaders and the synthetic batches yield uint8)."""
    return rgb if rgb.dtype == torch.uint8 else rgb.round().clamp(0, 255).to(torch.uint8)


@dataclasses.dataclass
class _Trainer:
    """What one of the four command lines has of its own; main() is everything else.  The trainer object `build` returns names its
    optimiser {what}_optim, its per-epoch scheduler {what}_scheduler if it has one, and saves state_dict(name) as {name}_{epoch}.th."""
    num_epoch: int                  # defaults of --num-epoch, --batch-size, --config-path (None: a run on recorded routes must name one)
    batch_size: int
    config_path: Optional[str]
    config_help: str
    flags: dict                     # its own flags: {the shared flag they follow in --help: [(flag, add_argument keywords), ...]}
    build: Callable                 # (args, cfg, device, rank) -> the trainer object, from the checkpoints the flags name
    loader: str                     # lav_amd.data.get_data_loader's name, and what it counts
    unit: str
    synthetic: Callable             # (args, cfg, per_rank, seed, device) -> one seeded batch
    stepper: Callable               # (trainer, args, rank, world, device, loader) -> step(batch, global_it) -> info; called once, after the loader
    log: Callable                   # info -> what a log line shows of it
    saves: tuple
    replicas: tuple                 # the trainer's modules whose parameters the replica checksum covers; (): no check, no summary field
    overrides: Callable = lambda args: {}       # TrainConfig keys taken from the command line besides lr and seed
    loader_kwargs: Callable = lambda args: {}
    guard_dt: bool = True


def _lav(what):
    """lav/train_bev_v2.py:42-63 ("bev") / lav/train_full_v2.py:48-70 ("lidar"), same flags and defaults, over the 'temporal_bev' /
    'temporal_lidar_painted' loaders.  What this build adds: --lidar / --bev / --uniplanner (checkpoints to start from), --max-points,
    --log-every, --deterministic, --bev-on-device (the loaders hand over the decoded map planes and their warps, lav_bev_stack_u8
    renders the batch's BEV stacks behind the upload)."""
    bev = what == "bev"

    def build(args, cfg, device, rank):
        ck = {k: torch.load(v, map_location="cpu") for k, v in resolve_checkpoints(what, args).items() if v}
        torch.manual_seed(cfg.seed + rank)      # (kept as found: seeded per rank BEFORE the trainer is built; seg / bra seed after the loader)
        return LAV(cfg, device, what=what, checkpoints=ck)

    def stepper(lav, args, rank, world, device, loader):
        stacker, bev_at = None, 0 if bev else 5      # where the sample tuples hold `bev`
        if loader is not None and args.bev_on_device:
            from ..data.bev_stack import BevStacker
            stacker = BevStacker()

        def step(batch, it):
            if stacker is not None:      # the planes go up as uint8 (the bytes `bev` itself would take) and are rendered there
                batch = list(batch)
                batch[bev_at] = stacker(batch[bev_at], device=device)
            return lav.train_bev(*batch, other_weight=other_weight_schedule(it)) if bev else lav.train_lidar(*batch)
        return step

    def synthetic(args, cfg, per_rank, seed, device):
        if bev:
            return synthetic_bev_batch(per_rank, seed=seed, device=device)
        return synthetic_lidar_batch(per_rank, seed=seed, max_points=args.max_points or cfg.max_lidar_points, device=device)

    flags = {
        "--device": [("--perceive-only", dict(action="store_true")), ("--motion-only", dict(action="store_true"))],
        "--lr": [("--weight-decay", dict(type=float, default=2e-4, help="accepted for command-line compatibility; the reference never passes it to Adam"))],
        "--save-dir": [
            ("--lidar", dict(default=None, help="lidar_*.th to start from")),
            ("--bev", dict(default=None, help="bev_*.th to start from / the teacher of train_full_v2")),
            ("--uniplanner", dict(default=None, help="uniplanner_*.th to start from")),
            ("--max-points", dict(type=int, default=None)),
            ("--log-every", dict(type=int, default=None, help="steps between the eval-mode log inference (default: --num-per-log)")),
            ("--deterministic", dict(action="store_true", help="bit-reproducible steps: deterministic torch / MIOpen algorithms "
                                     "(liblav_amd's own kernels always are); slower convolution gradients")),
            ("--bev-on-device", dict(action="store_true",
                                     help="recorded routes only: the loaders return the decoded map planes with their warp coefficients "
                                          "(lav_amd.data.bev_stack) and the batch's BEV stacks are rendered after the uint8 upload, bit-identical to the "
                                          "loaders' own; no effect with --synthetic"))]}
    return _Trainer(
        num_epoch=160 if bev else 64, batch_size=256 if bev else 32, config_path=None,
        config_help="the reference's config_v2.yaml (training keys are read from it)", flags=flags, build=build,
        loader="temporal_bev" if bev else "temporal_lidar_painted", unit="frames", synthetic=synthetic, stepper=stepper,
        log=lambda info: {k: round(v, 4) for k, v in info.items() if isinstance(v, float)},
        saves=("bev",) if bev else ("lidar", "uniplanner"), replicas=("bev_planner",) if bev else ("lidar_model", "uniplanner"),
        overrides=lambda args: dict(perceive_only=args.perceive_only, motion_only=args.motion_only,
                                    log_every=args.log_every if args.log_every is not None else args.num_per_log),
        loader_kwargs=lambda args: dict(bev_on_device=args.bev_on_device),
        guard_dt=False)     # (kept as found: these two divide by the bare elapsed time, seg / bra by max(dt, 1e-9))


def _camera_stepper(images, train):
    """seg / bra: --augment's Augmenters over a batch's first `images` tensors (one stream tag each), then train(trainer)(*batch)."""
    def stepper(trainer, args, rank, world, device, loader):
        torch.manual_seed(args.seed)        # (kept as found: after the trainer and the loader, the same seed on every rank)
        aug = _augmenters(args, rank, world, images)

        def step(batch, it):
            if aug is not None:      # uploaded as uint8 and augmented there; the train step converts them as ever
                batch = [a(_as_u8_hwc(x).to(device)) for a, x in zip(aug, batch)] + list(batch[images:])
            return train(trainer)(*batch)
        step.augmenters = aug or ()       # (--state-dir saves their counts)
        return step
    return stepper


_AUGMENT = ("--augment", dict(type=float, default=0.0, metavar="PROB",
                              help="image augmentation (lav_amd.data.augment): each of the seven ops with this probability, on the device, after a "
                                   "uint8 upload; the reference trains with 0.5 (augment(0.5)).  Default 0: no augmentation"))

# lav/train_seg.py, same flags and defaults (--config-path defaults to the v2 agent's config, the consumer of the segmenter): the camera
# images of the 'seg' loader or synthetic 288 x 256 ones, seg_{epoch}.th with RGBSegmentationModel's keys (the agent's `seg_model_dir`).
# What this build adds: --seg (a checkpoint to start from), --augment PROB (the reference's augment(0.5) of every camera image).
_SEG = _Trainer(
    num_epoch=1, batch_size=256, config_path="config_v2.yaml", config_help="the reference's config_v2.yaml (seg_channels, data_dir)",
    flags={"--save-dir": [("--seg", dict(default=None, help="seg_*.th to start from")), _AUGMENT]},
    build=lambda args, cfg, device, rank: LAV(cfg, device, what="seg", checkpoints={"seg": torch.load(args.seg, map_location="cpu")} if args.seg else {}),
    loader="seg", unit="camera images", stepper=_camera_stepper(1, lambda lav: lav.train_seg), saves=("seg",),
    synthetic=lambda args, cfg, per_rank, seed, device: synthetic_seg_batch(per_rank, seed=seed, num_classes=len(cfg.seg_channels) + 1, device=device),
    log=lambda info: dict(loss=round(info["loss"], 4)),
    replicas=())        # (kept as found: no replica checksum, no replicas_in_sync in the summary)

# lav/train_bra_v2.py, same flags and defaults: the 'bra' loader (the three front cameras side by side, the telephoto camera, their labels,
# the brake flag) or synthetic 288 x 768 + 192 x 480 images, bra_{epoch}.th with RGBBrakePredictionModel([4, 10, 18])'s keys (the agent's
# `bra_model_dir`).  What this build adds: --bra (a checkpoint to start from), --augment PROB (the wide and the telephoto image).
_BRA = _Trainer(
    num_epoch=10, batch_size=52, config_path="config_v2.yaml", config_help="the reference's config_v2.yaml (data_dir, camera_yaws, crop_tel_bottom)",
    flags={"--save-dir": [("--bra", dict(default=None, help="bra_*.th to start from")), _AUGMENT]},
    build=lambda args, cfg, device, rank: BrakeTrainer(cfg, device, checkpoints={"bra": torch.load(args.bra, map_location="cpu")} if args.bra else {}),
    loader="bra", unit="frames", stepper=_camera_stepper(2, lambda trainer: trainer.train_bra), saves=("bra",),
    synthetic=lambda args, cfg, per_rank, seed, device: synthetic_bra_batch(per_rank, seed=seed, num_classes=len(BRA_LABELS) + 1, device=device),
    log=lambda info: dict(loss=round(info["loss"], 4), bra=info["bra"], pred_bra=round(info["pred_bra"], 4)), replicas=("bra_model",))


def _val_tool(what):
    """The evaluation tool of a trainer's own checkpoints (eval_common.run_cli's description)."""
    if what in ("seg", "bra"):
        from .evaluate_camera import _WHAT
        return _WHAT[what]
    if what == "bev":
        from .evaluate_bev import TOOL
        return TOOL
    from .evaluate import TOOL
    return TOOL


def _val_argv(tool, args, paths):
    """The tool's command line over --val-data-dir: the files just written, the tool's own defaults (the frame's precision) otherwise."""
    argv = ["--config-path", args.config_path, "--data-dir", args.val_data_dir, "--num-workers", str(max(0, min(args.num_workers, 4)))]
    for name, path in paths.items():
        argv += [f"--{name}", path]
    if args.val_max > 0:
        argv += [f"--max-{tool['unit']}", str(args.val_max)]
    return argv


def _process_settings():
    """What a validation must hand back as it found it, besides the generators: backend flags, default dtype, the precision stack."""
    from .. import ops
    mi = getattr(torch.backends, "miopen", None)
    return dict(cudnn=(torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic, torch.backends.cudnn.allow_tf32, torch.backends.cudnn.enabled),
                matmul=torch.backends.cuda.matmul.allow_tf32, miopen=getattr(mi, "immediate", None), dtype=torch.get_default_dtype(),
                deterministic=(torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()),
                grad=torch.is_grad_enabled(), precision=tuple(getattr(ops._precision_stack, "v", None) or ()))


def validate(what, args, trainer, device, epoch, global_it, files):
    """--val-data-dir, rank 0, right behind an epoch's checkpoint files: each of `files` = (weights, {name: path}) through the trainer's
    own evaluation tool (eval_common.run_cli, in this process, on inference modules it builds from the files), the tool's JSON line
    plus epoch / global_it / weights / buffers / checkpoints appended to SAVE_DIR/val.jsonl, one digest line printed.  The run goes on in
    the bits it would have had: every generator lav_amd.train.state covers is put back (run_cli seeds torch), and a setting or a trainer
    module's mode that an evaluation left changed ends the run."""
    from .eval_common import run_cli
    tool = _val_tool(what)

    def modes():        # every nn.Module the trainer object holds, whatever it is called
        return {f"{name}.{sub}": m.training for name, top in vars(trainer).items() if isinstance(top, torch.nn.Module)
                for sub, m in top.named_modules()}

    was = modes()
    before, rng = _process_settings(), run_state._rng_state(device)
    try:
        for weights, paths in files:
            for line in run_cli(tool, _val_argv(tool, args, paths), optional=("bev",) if what == "lidar" else (), echo=False):
                line = dict(line, epoch=epoch, global_it=global_it, weights=weights, buffers="live", checkpoints=[paths[k] for k in sorted(paths)])
                with open(os.path.join(args.save_dir, "val.jsonl"), "a") as f:
                    f.write(json.dumps(line) + "\n")
                rate = next((v for k, v in line.items() if k.endswith("_per_s")), None)
                shown = {k: v for k, v in (line.get("summary") or {}).items() if isinstance(v, (int, float)) or v is None}
                print(f"val epoch {epoch} it {global_it} weights: {weights} (buffers: live) {line['precision']} {line['data']}, {rate} {tool['unit']}/s: "
                      + json.dumps(shown), flush=True)
    finally:
        run_state._set_rng_state(rng, device)
    after, now = _process_settings(), modes()
    if after != before or now != was:
        moved = sorted(k for k in set(was) | set(now) if was.get(k) != now.get(k))
        raise SystemExit(f"--val-data-dir: the evaluation left the process changed: settings {before} -> {after}; "
                         f"modules whose mode moved: {[(k, was.get(k), now.get(k)) for k in moved[:8]]} ({len(moved)})")


def main(what):
    """The command line of train_bev_v2.py ("bev"), train_full_v2.py ("lidar"), train_seg.py ("seg") and train_bra_v2.py ("bra"), from
    the parser to the teardown: the recorded routes under the config's `data_dir` are read by lav_amd.data (every rank its own shard of
    each epoch), one optimiser step per batch, checkpoints every --num-per-save epochs, one JSON summary line.  What this build adds to
    the reference's flags: --synthetic / --steps-per-epoch (seeded synthetic batches instead of a data set), --save-dir, and what the
    trainer's description (_lav, _SEG, _BRA) names, --log-dir (a picture of sample 0 per logged iteration), --fused-optim /
    --max-grad-norm / --max-skipped-steps (lav_amd.train.optim.FusedAdam: a step with a NaN / Inf gradient is skipped, a run that keeps
    skipping ends), --state-dir / --resume (lav_amd.train.state: everything a run needs to go on from an epoch boundary), --ema DECAY (a
    moving average of the weights inside the fused step, saved as {name}_ema_{epoch}.th beside {name}_{epoch}.th; buffers: live) and
    --val-data-dir / --val-max (each file just written through the trainer's own evaluation tool, into SAVE_DIR/val.jsonl) and
    --tensor-stats N (lav_amd.train.tensor_stats: per-tensor gradient, weight and update statistics of every N-th step and the tensors
    behind every skipped one, into SAVE_DIR/tensor_stats.jsonl).  Without these flags nothing changes, files written included."""
    t = {"seg": _SEG, "bra": _BRA}.get(what) or _lav(what)
    ap = argparse.ArgumentParser()
    for flag, kw in (
            ("--config-path", dict(default=t.config_path, help=t.config_help)),
            ("--device", dict(default="cuda", choices=["cuda", "cpu"])),
            ("--num-epoch", dict(type=int, default=t.num_epoch)),
            ("--num-per-log", dict(type=int, default=100, help="log per iter")),
            ("--num-per-save", dict(type=int, default=1, help="save per epoch")),
            ("--batch-size", dict(type=int, default=t.batch_size, help="GLOBAL batch, split over the ranks")),
            ("--lr", dict(type=float, default=3e-4)),
            ("--num-workers", dict(type=int, default=16, help="DataLoader workers (recorded routes only)")),
            ("--seed", dict(type=int, default=2021)),
            ("--synthetic", dict(action="store_true", help="seeded synthetic batches instead of the config's data_dir")),
            ("--steps-per-epoch", dict(type=int, default=20, help="iterations that make one epoch of synthetic data")),
            ("--save-dir", dict(default="checkpoints")),
            ("--log-dir", dict(default=None, metavar="DIR",
                               help="write the reference's visual log of sample 0 (lav/utils/logger.py) as DIR/{what}_{iteration:07d}.png at every "
                                    "--num-per-log-th iteration, composed on the device (lav_amd.train.log_view).  Default: none, nothing changes")),
            ("--fused-optim", dict(action="store_true",
                                   help="lav_amd.train.optim.FusedAdam where torch.optim.Adam stands: one read of all gradients decides whether the step "
                                        "is applied (a NaN / Inf in any gradient skips it: parameters and moments keep every bit), one launch updates all "
                                        "parameters; the log lines gain grad_norm and skipped_steps")),
            ("--max-grad-norm", dict(type=float, default=None, metavar="X", help="clip the global gradient norm to X inside the fused step "
                                                                                 "(clip_grad_norm_'s factor); implies --fused-optim")),
            ("--max-skipped-steps", dict(type=int, default=10, metavar="N",
                                         help="--fused-optim: end the run (non-zero exit) when more than N steps were skipped between two log "
                                              "iterations, or when a BatchNorm running statistic is not finite")),
            ("--tensor-stats", dict(type=int, default=None, metavar="N",
                                    help="where a run goes wrong: behind every N-th optimiser step one more pass over g, p, m, v "
                                         "(lav_optim_tensor_stats) leaves per tensor the gradient's norm, largest element, zeros, values that are "
                                         "not finite and a 64-bin histogram of its exponents, the weight's norm and the norm of the update just "
                                         "applied; rank 0 appends them to SAVE_DIR/tensor_stats.jsonl (read it with python -m "
                                         "lav_amd.train.tensor_stats) and prints a digest at log iterations.  Every skipped step is written with "
                                         "the tensors that caused it, and the health stop names them.  The run's bits do not change; implies "
                                         "--fused-optim")),
            ("--ema", dict(type=float, default=None, metavar="DECAY",
                           help="keep an exponential moving average of the trained weights inside the fused step (e += (1 - d) (p - e), d = "
                                "min(DECAY, (1 + k) / (10 + k)) at the parameter's step count k; a skipped step leaves it alone) and write it as "
                                "{name}_ema_{epoch}.th wherever {name}_{epoch}.th is written: the same keys, frozen parameters and every buffer "
                                "(BatchNorm running statistics) at their live values - buffers: live.  0 < DECAY < 1; implies --fused-optim")),
            ("--val-data-dir", dict(default=None, metavar="DIR",
                                    help="held-out routes: right after an epoch's checkpoint files are written, rank 0 evaluates them (the _ema_ "
                                         "files too) with the trainer's own tool (eval_seg / eval_bra_v2 / eval_bev_v2 / eval_full_v2) at the frame's "
                                         "precision, appends each JSON line with epoch, global_it, weights (raw | ema), buffers and checkpoints to "
                                         "SAVE_DIR/val.jsonl and prints a digest; the run's bits do not change.  Needs a GPU and --config-path (the "
                                         "loaders' keys).  The other ranks wait for rank 0's verdict at one collective: keep --val-max below the "
                                         "process group's timeout")),
            ("--val-max", dict(type=int, default=1000, metavar="N", help="--val-data-dir: units (frames / images) per evaluation; 0: all")),
            ("--state-dir", dict(default=None, metavar="DIR",
                                 help="whenever checkpoints are written, also write DIR/state_{epoch}.th: models, optimiser, scheduler, iteration "
                                      "counters, augmenter counts, random generators of every rank (the two newest are kept).  State is taken at epoch "
                                      "boundaries only: resuming inside an epoch of a shuffled loader is out of scope")),
            ("--resume", dict(default=None, metavar="PATH",
                              help="continue from a state file at its epoch + 1, with its iteration count; 'auto': the newest of --state-dir, or a "
                                   "fresh start when there is none (a job script that is simply re-submitted).  Other defining arguments "
                                   "(batch size, seed, lr ...) than the state's are refused"))):
        for f, k in [(flag, kw)] + t.flags.get(flag, []):
            ap.add_argument(f, **k)
    args = ap.parse_args()
    if getattr(args, "deterministic", False):
        set_deterministic(True)
    if args.max_grad_norm is not None:
        if not args.max_grad_norm > 0:
            raise SystemExit(f"--max-grad-norm {args.max_grad_norm}: a positive norm")
        args.fused_optim = True
    if args.ema is not None:
        if not 0.0 < args.ema < 1.0:
            raise SystemExit(f"--ema {args.ema}: a decay, 0 < DECAY < 1")
        args.fused_optim = True
    if args.tensor_stats is not None:
        if args.tensor_stats < 1:
            raise SystemExit(f"--tensor-stats {args.tensor_stats}: every N-th iteration, N >= 1")
        args.fused_optim = True
    if args.val_data_dir is not None:
        if args.device == "cpu":
            ap.error("--val-data-dir with --device cpu: the models have no CPU inference path")
        if args.val_max < 0:
            ap.error(f"--val-max {args.val_max}")
        if not (args.config_path and os.path.isfile(args.config_path)):
            ap.error("--val-data-dir reads the loaders' keys from --config-path (with --synthetic too)")
    if args.resume == "auto" and not args.state_dir:
        raise SystemExit("--resume auto looks into --state-dir")
    # without a default (bev / lidar) the file named must exist, open() says so; a default that is not there (seg / bra) is no config
    named = t.config_path is None
    have_cfg = bool(args.config_path) and (named or os.path.isfile(args.config_path))
    if not args.synthetic and not have_cfg:
        raise SystemExit("recorded routes are read from the data_dir of --config-path ("
                         + ("" if named else f"{args.config_path} not found; ") + "or pass --synthetic)")
    rank, world, device = setup_distributed()
    if args.device == "cpu":
        device = torch.device("cpu")
    cfg = load_config(args.config_path if have_cfg else None, lr=args.lr, seed=args.seed, fused_optim=args.fused_optim,
                      max_grad_norm=args.max_grad_norm, ema_decay=args.ema, tensor_stats=args.tensor_stats, **t.overrides(args))
    if args.batch_size % world:
        raise SystemExit(f"global batch {args.batch_size} is not divisible by {world} ranks")
    per_rank = args.batch_size // world
    trainer = t.build(args, cfg, device, rank)
    loader = None
    if not args.synthetic:
        from ..data import get_data_loader
        loader = get_data_loader(t.loader, args, rank=rank, world=world, **t.loader_kwargs(args))
        if len(loader) == 0:
            raise SystemExit(f"{args.config_path}: data_dir holds fewer {t.unit} than one batch of {args.batch_size}")
    if args.val_data_dir is not None:       # before the first step: a directory without routes ends the run here
        from .eval_common import held_out_units
        if not torch.cuda.is_available():
            raise SystemExit("--val-data-dir: no GPU visible; the models have no CPU inference path")
        tool = _val_tool(what)
        rng = run_state._rng_state(device)      # (the loaders seed NumPy where they list their routes)
        units = held_out_units(tool, args.config_path, args.val_data_dir)
        run_state._set_rng_state(rng, device)
        if units == 0:
            raise SystemExit(f"--val-data-dir {args.val_data_dir}: no recorded {tool['unit']} there")
    step = t.stepper(trainer, args, rank, world, device, loader)
    scheduler = getattr(trainer, f"{what}_scheduler", None)

    def batches(epoch):
        if loader is not None:
            if world > 1:
                loader.sampler.set_epoch(epoch)
            yield from loader
            return
        for it in range(args.steps_per_epoch):
            yield t.synthetic(args, cfg, per_rank, cfg.seed + 1000003 * epoch + 1009 * it + 100 * rank, device)

    # --log-dir, rank 0: the logged steps also return their "view"; its frame is composed where the tensors are and handed to the writer,
    # which encodes it when the next one arrives (and at the end) - the step never waits for its own picture
    writer = log_view.FrameWriter(args.log_dir, what) if args.log_dir and rank == 0 else None
    global_it, first_epoch = 0, 0
    resume = run_state.newest(args.state_dir) if args.resume == "auto" else args.resume      # (auto without a file: a fresh start)
    if resume:
        first_epoch, global_it = run_state.restore(run_state.load(resume), trainer, what, args, getattr(step, "augmenters", ()), rank, world)
        if rank == 0:
            print(f"resumed from {resume}: epoch {first_epoch}, iteration {global_it}", flush=True)
    optimizer = getattr(trainer, f"{what}_optim")
    skipped_seen = health = None
    if args.fused_optim:
        skipped_seen = optimizer.health()["skipped"]
    # --tensor-stats: every rank's optimiser carries the names and records who made a step skip (its own health stop names them); the
    # per-tensor rows and the file are rank 0's - under data parallel all ranks see the same all-reduced gradients
    stats_log = tensor_stats.TensorStatsLog(args.save_dir, args.tensor_stats, global_it) if args.tensor_stats and rank == 0 else None
    it_first = global_it
    t0, it0 = time.perf_counter(), global_it
    val_failed = None
    for epoch in range(first_epoch, args.num_epoch):
        for batch in batches(epoch):
            drawn = writer is not None and global_it % args.num_per_log == 0
            trainer.log_view = drawn
            info = step(batch, global_it)
            if drawn:
                trainer.log_view = False
                writer.add(log_view.render(log_view.build_frame(what, info.pop("view"), cfg)), global_it)
            if stats_log is not None:
                stats_log.after_step(optimizer, global_it)
            if global_it % args.num_per_log == 0:
                shown = t.log(info) if rank == 0 else None
                if args.fused_optim:
                    # every rank reads its own words and takes the decision alone: under data parallel all of them stepped on the same
                    # all-reduced gradients, so they all see the same counts - no collective is needed to agree on the end of the run
                    health = optimizer.health()
                    if rank == 0:
                        shown = dict(shown, grad_norm=round(health["grad_norm"], 4), skipped_steps=health["skipped"])
                if rank == 0:
                    print(global_it, shown, flush=True)
                if args.tensor_stats:
                    blame = optimizer.blame()
                    if stats_log is not None:
                        digest = stats_log.digest()
                        if digest is not None:
                            print(digest, flush=True)
                        blame = stats_log.blamed(blame)
                    else:
                        blame = tuple([dict(r, global_it=it_first + r["step"] - 1) for r in recs] for recs in blame)
                    if health["watch_nonfinite"] and not blame[1]:     # (a step that was applied records none: look once, the run ends here)
                        blame = (blame[0], optimizer.watched_nonfinite())
                    skipped_seen = run_state.check_health(health, skipped_seen, args.max_skipped_steps, args.state_dir, blame)
                elif args.fused_optim:
                    skipped_seen = run_state.check_health(health, skipped_seen, args.max_skipped_steps, args.state_dir)
            global_it += 1
        if scheduler is not None:
            scheduler.step()       # once per epoch (train_full_v2.py:33)
        if (epoch + 1) % args.num_per_save == 0 and rank == 0:
            os.makedirs(args.save_dir, exist_ok=True)
            written = {"raw": {}, "ema": {}}
            for name in t.saves:
                path = os.path.join(args.save_dir, f"{name}_{epoch + 1}.th")
                torch.save(trainer.state_dict(name), path)
                print(f"saved to {path}", flush=True)
                written["raw"][name] = path
            if args.ema is not None:
                for name in t.saves:
                    path = os.path.join(args.save_dir, f"{name}_ema_{epoch + 1}.th")
                    torch.save(ema_state_dict(run_state._module(trainer, name), optimizer), path)
                    print(f"saved to {path}", flush=True)
                    written["ema"][name] = path
            if args.val_data_dir is not None:
                try:
                    validate(what, args, trainer, device, epoch + 1, global_it, [(w, paths) for w, paths in written.items() if paths])
                except (SystemExit, Exception) as e:      # (told to the other ranks first: they all end with it, none waits for a timeout)
                    val_failed = f"validation after epoch {epoch + 1} failed: {e!r}" if not isinstance(e, SystemExit) else str(e.code)
        if (epoch + 1) % args.num_per_save == 0 and args.val_data_dir is not None:
            if world > 1:       # rank 0 validates, the others wait here for its verdict
                verdict = [val_failed]
                dist.broadcast_object_list(verdict, src=0)
                val_failed = verdict[0]
            if val_failed is not None:
                raise SystemExit(val_failed)
        if (epoch + 1) % args.num_per_save == 0 and args.state_dir:     # every rank: the ranks' generator states are gathered
            st = run_state.capture(trainer, what, args, epoch + 1, global_it, getattr(step, "augmenters", ()), rank, world)
            if rank == 0:
                print(f"state in {run_state.write(st, args.state_dir)}", flush=True)
    if writer is not None:
        writer.close()
    if stats_log is not None:
        stats_log.blamed(optimizer.blame())
        stats_log.close()
    if device.type == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    summary = dict(what=what, samples_per_s=round(args.batch_size * (global_it - it0) / (max(dt, 1e-9) if t.guard_dt else dt), 2), n_gpus=world)
    if t.replicas:
        summary["replicas_in_sync"] = None
        if world > 1:   # data parallel keeps the replicas identical: compare a checksum of every trained parameter across the ranks
            # (BatchNorm's running statistics are per-rank by design - DDP re-broadcasts rank 0's before each forward - and are left out)
            mine = torch.stack([p_.detach().double().sum() for m in t.replicas for p_ in getattr(trainer, m).parameters() if p_.requires_grad]).to(device)
            every = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(every, mine)
            summary["replicas_in_sync"] = all(torch.equal(every[0], e) for e in every[1:])
    summary.update(global_batch=args.batch_size, steps=global_it, epochs=args.num_epoch,
                   data="synthetic batches" if loader is None else f"{len(loader.dataset)} recorded {t.unit}",
                   lr=getattr(trainer, f"{what}_optim").param_groups[0]["lr"])
    if scheduler is not None:
        summary["scheduler_epochs"] = scheduler.last_epoch
    if args.fused_optim:
        health = optimizer.health()
        summary.update(fused_optim=True, skipped_steps=health["skipped"], last_grad_norm=health["grad_norm"])
    if args.ema is not None:
        summary["ema_decay"] = args.ema
    if rank == 0:
        print(json.dumps(summary))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
