"""Worker of tests/test_ema_host.py::test_eval_tools_build_without_a_collective_inside_a_process_group: two gloo ranks, of which rank 0
alone builds the evaluation tools' models - what the trainers' --val-data-dir does behind a save."""
import argparse
import datetime
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=90))
rank = dist.get_rank()
from lav_amd.train import TrainConfig, evaluate, evaluate_bev  # noqa: E402
from lav_amd.train.lav import LAV  # noqa: E402

DDP = torch.nn.parallel.DistributedDataParallel
cfg, cpu = TrainConfig(), torch.device("cpu")
if rank == 0:
    for build, args in ((evaluate_bev._build, argparse.Namespace(bev=None)),
                        (evaluate._build, argparse.Namespace(lidar=None, uniplanner=None, bev=None))):
        lav = build(args, cfg, cpu)
        wrapped = [k for k, v in vars(lav).items() if isinstance(v, DDP)]
        assert not wrapped, f"{build.__module__}: {wrapped} are DistributedDataParallel"
# had rank 0 issued a collective of its own (DistributedDataParallel's constructor is one), this all-reduce would meet it on rank 1
# and not add up
t = torch.tensor([rank + 1.0], dtype=torch.float64)
dist.all_reduce(t)
assert t.item() == 3.0, t
trainer = LAV(cfg, cpu, what="bev")         # every rank: the trainers' own build still wraps
assert isinstance(trainer.bev_ddp, DDP)
dist.barrier()
if rank == 0:
    print("VAL_WORKER_OK")
dist.destroy_process_group()
