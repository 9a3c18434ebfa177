"""BEVPlanner (privileged teacher) with the reference's constructor and state_dict keys
(lav/models/bev_planner_v2.py:7-71).  It rides inside UniPlanner checkpoints (`bev_planner.*`), so it must
exist for drop-in loading; its cast/plan decoders run on the same HIP GRU kernels.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import planner_common
from .planner_common import BatchInference, PlannerBase, sample_others  # noqa: F401  (BatchInference: infer_batch's result, read here too)
from .resnet import resnet18


class BEVPlanner(PlannerBase):
    def __init__(self, pixels_per_meter=2, crop_size=64, x_offset=0, y_offset=0.75, feature_x_jitter=1,
                 feature_angle_jitter=10, num_plan=10, k=16, num_out_feature=64, num_cmds=6, max_num_cars=5,
                 num_plan_iter=1, num_frame_stack=0):
        super().__init__()
        self.num_cmds, self.num_plan, self.num_plan_iter = num_cmds, num_plan, num_plan_iter
        self.max_num_cars, self.num_out_feature = max_num_cars, num_out_feature
        self.pixels_per_meter, self.crop_size = pixels_per_meter, crop_size
        self.feature_x_jitter = feature_x_jitter
        self.feature_angle_jitter = np.deg2rad(feature_angle_jitter)
        self.offset_x = nn.Parameter(torch.tensor(x_offset).float(), requires_grad=False)
        self.offset_y = nn.Parameter(torch.tensor(y_offset).float(), requires_grad=False)
        self.bev_conv_emb = nn.Sequential(resnet18(num_channels=3 + 2 * (num_frame_stack + 1)),
                                          nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten())
        self.plan_gru = nn.GRU(4, 512, batch_first=True)
        self.plan_mlp = nn.Linear(512, 2)
        self.cast_grus = nn.ModuleList([nn.GRU(512, 64, batch_first=True) for _ in range(num_cmds)])
        self.cast_mlps = nn.ModuleList([nn.Linear(64, 2) for _ in range(num_cmds)])
        self.cast_cmd_pred = nn.Sequential(nn.Linear(512, num_cmds), nn.Sigmoid())

    def _cast_modules(self):
        return self.cast_grus, self.cast_mlps

    @torch.no_grad()
    def infer(self, bev, nxps):
        """bev_planner_v2.py:46-70."""
        crop = self.crop_feature(bev, bev.new_zeros((1, 2)), bev.new_zeros((1,)), self.pixels_per_meter, self.crop_size * 2)
        embd = self.bev_conv_emb(crop)
        cast = self.cast(embd)
        plan = self.plan(embd, nxps, cast_locs=cast, pixels_per_meter=self.pixels_per_meter, crop_size=self.crop_size * 2)
        return plan, cast, self.cast_cmd_pred(embd)

    @torch.no_grad()
    def infer_batch(self, bev, ego_locs, locs, oris, nxps, typs, others="ahead"):
        """The teacher over a loader batch with no random draw (eval_bev_v2.py): forecasts for EVERY vehicle among locs[:, 1:] -
        others="ahead": those that pass filter_cars, what the teacher was trained on; "all": all of them; no cap at max_num_cars - from
        its un-jittered crop, and cast, command scores and every refinement of the plan from the B ego crops.  forward's eval-mode
        arithmetic: crop_rotate_indexed -> bev_conv_emb -> cast / cast_cmd_pred -> plan (all six commands), other_locs as forward
        computes them with zero jitter (torch ops, float32, the vehicle's own frame).  Arguments as forward's, in HBM.  Returns
        BatchInference: other_locs (K, T, 2), other_cast (K, 6, T, 2), other_cmds (K, 6), ego_plan (B, I, 6, T, 2), ego_cast
        (B, 6, T, 2), ego_cmds (B, 6), sample (K,) and actor (K,) int32; K = 0 gives empty tensors on the device.  Eval mode only (the
        module has no HIP train-mode decoders); the convolutions follow ops.precision; the global generators are not touched."""
        return planner_common.infer_batch(self, self.bev_conv_emb, bev, ego_locs, locs, oris, nxps, typs, others, self.pixels_per_meter, self.crop_size * 2)

    def forward(self, bev, ego_locs, locs, oris, nxps, typs):
        """Training forward of the privileged planner (bev_planner_v2.py:72-174): forecasts for up to `max_num_cars`
        jittered crops around other vehicles and the ego plan from the un-jittered ego crop.
        bev (B,9,320,320), ego_locs (B,T+1,2), locs (B,N+1,T+1,2), oris (B,N+1), nxps (B,2), typs (B,N+1)."""
        pick, N = sample_others(self, ego_locs, locs, oris, typs)
        ppm, crop = self.pixels_per_meter, self.crop_size * 2
        if pick is not None:
            other_embd = self.bev_conv_emb(self.crop_feature(bev, pick["crop_locs"], pick["crop_oris"], ppm, crop, map_index=pick["sample"]))
            other_locs = pick["other_locs"]
            other_cast_cmds = self.cast_cmd_pred(other_embd)
        else:
            z = dict(dtype=bev.dtype, device=bev.device)
            other_locs = torch.zeros((N, self.num_plan, 2), **z)
            other_cast_locs = torch.zeros((N, self.num_cmds, self.num_plan, 2), **z)
            other_cast_cmds = torch.zeros((N, self.num_cmds), **z)
            other_embd = None
        B = bev.size(0)
        ego_embd = self.bev_conv_emb(self.crop_feature(bev, bev.new_zeros((B, 2)), bev.new_zeros((B,)), ppm, crop,
                                                       map_index=torch.arange(B, dtype=torch.int32, device=bev.device)))
        if other_embd is not None:     # one cast() over others + ego: same arithmetic, half the GRU launches
            both = self.cast(torch.cat([other_embd, ego_embd]))
            other_cast_locs, ego_cast_locs = both[:other_embd.size(0)], both[other_embd.size(0):]
        else:
            ego_cast_locs = self.cast(ego_embd)
        ego_plan_locs = self.plan(ego_embd, nxps, cast_locs=ego_cast_locs, pixels_per_meter=ppm, crop_size=crop)
        return other_locs, other_cast_locs, other_cast_cmds, ego_plan_locs, ego_cast_locs, self.cast_cmd_pred(ego_embd)
