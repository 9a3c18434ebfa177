"""Pieces shared by UniPlanner and BEVPlanner: the GRU decoders on liblav_amd and the rotated crop."""
from __future__ import annotations

import collections

import torch
import torch.nn.functional as F

from . import ops
from .engine import Engine


def _hip_train(what: str) -> bool:
    """Diagnosis knob (tools/curve_bisect.py): LAV_TRAIN_<what>=torch runs that piece of the TRAINING graph on torch's own ops
    (nn.GRU = MIOpen's RNN, affine_grid + grid_sample) instead of liblav_amd's autograd functions - to tell a kernel's effect on a
    training run apart from everything else.  Inference never consults it."""
    import os
    return os.environ.get("LAV_TRAIN_" + what, "hip") != "torch"


def stack_cast_weights(grus, mlps, device):
    """6 x nn.GRU(512,64) + 6 x nn.Linear(64,2) -> the stacked arrays lav_gru_cast takes."""
    g = lambda mods, n: torch.stack([getattr(m, n).detach() for m in mods]).float().contiguous().to(device)
    return dict(w_ih=g(grus, "weight_ih_l0"), w_hh=g(grus, "weight_hh_l0"), b_ih=g(grus, "bias_ih_l0"), b_hh=g(grus, "bias_hh_l0"),
                mlp_w=g(mlps, "weight"), mlp_b=g(mlps, "bias"))


def plan_weights(gru, mlp, device):
    """The same arrays for the one plan GRU and its Linear, as lav_gru_plan takes them."""
    return {k: v[0] for k, v in stack_cast_weights([gru], [mlp], device).items()}


def crop_feature(features, rel_locs, rel_oris, pixels_per_meter, crop_size, offset_x, offset_y):
    """Rotated crop of the feature map around each actor (team_code_v2/model_inference.py:204-238 /
    uniplanner.py:310-352): theta = k*R(ori) with the (offset_x, offset_y) pivot, bilinear, zeros outside,
    align_corners=True - one liblav_amd kernel instead of affine_grid + grid_sample.  A feature map that was
    `expand`ed over the batch (stride 0) is passed once and shared by all crops."""
    if features.dim() == 4 and features.shape[0] > 1 and features.stride(0) == 0:
        features = features[:1]
    return ops.crop_rotate(features, rel_locs, rel_oris, pixels_per_meter, crop_size, offset_x, offset_y)


def crop_feature_torch(features, rel_locs, rel_oris, pixels_per_meter, crop_size, offset_x, offset_y):
    """The same crop with torch's affine_grid/grid_sample (kept for training mode, which needs autograd)."""
    B, C, H, W = features.shape
    rel_locs = rel_locs.view(-1, 2) * pixels_per_meter
    rel_locs = torch.stack([rel_locs[:, 0] / (H / 2), rel_locs[:, 1] / (W / 2)], dim=-1)
    cos, sin = torch.cos(rel_oris), torch.sin(rel_oris)
    k = crop_size / H
    rot_x = -k * offset_x * cos + k * offset_y * sin + offset_x
    rot_y = -k * offset_x * sin - k * offset_y * cos + offset_y
    theta = torch.stack([torch.stack([k * cos, k * -sin, rot_x + rel_locs[..., 0]], dim=-1),
                         torch.stack([k * sin, k * cos, rot_y + rel_locs[..., 1]], dim=-1)], dim=-2)
    grid = F.affine_grid(theta, (B, C, crop_size, crop_size), align_corners=True)
    return F.grid_sample(features, grid, align_corners=True)


def transform_points(locs, oris):
    """model_inference.py:240-251: rotate (.., T, 2) waypoints by -ori (row-vector convention)."""
    cos, sin = torch.cos(oris), torch.sin(oris)
    R = torch.stack([torch.stack([cos, sin], dim=-1), torch.stack([-sin, cos], dim=-1)], dim=-2)
    return locs @ R


def filter_cars(ego_locs, locs, typs):
    """Vehicles ahead of the ego vehicle only (bev_planner_v2.py:279-283; -y is forward)."""
    return typs & ((locs[:, :, 0] - ego_locs[:, 0:1])[..., 1] < 0)


def random_sample(binaries, size):
    """Keep at most `size` set entries per row, chosen uniformly (bev_planner_v2.py:286-299; same RNG calls)."""
    cut = torch.zeros_like(binaries)
    counts = binaries.sum(1).tolist()      # (ONE device->host copy for the rows' counts; the reference pays a sync per row)
    if max(counts, default=0) <= size:
        return binaries.clone()
    for i in range(binaries.size(0)):
        if counts[i] <= size:
            cut[i] = binaries[i]
        else:
            nz = torch.nonzero(binaries[i]).squeeze(1)
            nz = nz[torch.multinomial(torch.ones_like(nz).float(), size)]
            cut[i, nz] = binaries[i, nz]
    return cut


def select_others(ego_locs, locs, typs, ahead=True):
    """The selection half of sample_others, no random draw: which of locs[:, 1:] are vehicles (typs == 1) and, with `ahead`, pass
    filter_cars.  (B, N) bool."""
    vehicles = typs[:, 1:] == 1          # 1 = vehicle
    return filter_cars(ego_locs, locs[:, 1:], vehicles) if ahead else vehicles


def picked_others(ego_locs, locs, oris, picked, jitter):
    """The geometry of the picked vehicles (`picked`: (B, N) bool over locs[:, 1:]): their crops in the ego frame and their future in
    their own.  jitter(K, device) -> ((K, 2), (K,)) is called once, after the gathers - where sample_others has always drawn -, and
    zeros there give the un-jittered quantities by the same arithmetic."""
    ego_oris = oris[:, :1]
    locs, oris = locs[:, 1:], oris[:, 1:]
    flat_locs = (locs[:, :, 1:] - locs[:, :, :1])[picked]
    rel_loc0 = (locs[:, :, 0] - ego_locs[:, None, 0])[picked]
    rel_ori0 = (oris - ego_oris)[picked]
    locs_jitter, oris_jitter = jitter(flat_locs.size(0), locs.device)
    other_locs = transform_points(flat_locs - locs_jitter[:, None], -rel_ori0 - oris_jitter)
    where = torch.nonzero(picked)         # which sample's maps each picked vehicle is cropped from, and which of its actors it is
    return dict(typs=picked, sample=where[:, 0].int(), actor=where[:, 1].int(), crop_locs=rel_loc0 + locs_jitter,
                crop_oris=rel_ori0 + oris_jitter, other_locs=other_locs)


def sample_others(self, ego_locs, locs, oris, typs):
    """Shared front half of BEVPlanner.forward / UniPlanner.forward (bev_planner_v2.py:74-101, uniplanner.py:58-86):
    pick the vehicles to train on and draw their crop jitter.  Returns None when no vehicle qualifies."""
    typs = select_others(ego_locs, locs, typs)
    if int(typs.float().sum()) == 0:
        return None, locs.size(1) - 1
    typs = random_sample(typs, size=self.max_num_cars)

    def jitter(K, device):
        locs_jitter = (torch.rand((K, 2)) * 2 - 1).float().to(device) * self.feature_x_jitter
        locs_jitter[:, 1] = 0
        oris_jitter = (torch.rand((K,)) * 2 - 1).float().to(device) * self.feature_angle_jitter
        return locs_jitter, oris_jitter
    return picked_others(ego_locs, locs, oris, typs, jitter), locs.size(1) - 1


# infer_batch's result: forward's six outputs, then the (sample, actor) index of every forecast (actor counts locs[:, 1:])
BatchInference = collections.namedtuple("BatchInference", "other_locs other_cast other_cmds ego_plan ego_cast ego_cmds sample actor")


def infer_batch(planner, embed, maps, ego_locs, locs, oris, nxps, typs, others, map_ppm, map_crop):
    """What BEVPlanner.infer_batch and UniPlanner.infer_batch share: a loader batch through `planner` with no random draw.  The picks
    are select_others + picked_others with zero jitter (every vehicle among locs[:, 1:] that qualifies, no cap at max_num_cars); `embed`
    (the planner's crop embedder) reads map_crop-pixel crops of `maps` at map_ppm pixels per metre, the others' first and then the B
    ego crops, as the forwards launch them; one cast() over others + ego, cast_cmd_pred, and plan for all six commands and every
    refinement.  Returns BatchInference; K = 0 gives empty tensors on the device.  Eval mode only, `maps` in HBM; the global generators
    are not touched."""
    name = type(planner).__name__
    if planner.training:
        raise RuntimeError(f"{name}.infer_batch runs the eval-mode kernels: call .eval() first")
    if others not in ("ahead", "all"):
        raise ValueError(f"infer_batch: others={others!r} (ahead or all)")
    if not maps.is_cuda:
        raise RuntimeError(f"{name}.infer_batch: the batch must be in HBM; lav_amd has no CPU inference path")
    ppm, crop, B = planner.pixels_per_meter, planner.crop_size * 2, maps.size(0)
    z = dict(dtype=maps.dtype, device=maps.device)
    picked = select_others(ego_locs, locs, typs, ahead=others == "ahead")
    pick = picked_others(ego_locs, locs, oris, picked, lambda K, device: (torch.zeros((K, 2), **z), torch.zeros((K,), **z)))
    K = pick["sample"].size(0)
    other_embd = None      # (the launches in forward's order: the others' crops, then the ego's)
    if K:
        other_embd = embed(ops.crop_rotate_indexed(maps, pick["sample"], pick["crop_locs"], pick["crop_oris"], map_ppm, map_crop, *planner.offsets()))
        other_cmds = planner.cast_cmd_pred(other_embd)
    ego_embd = embed(ops.crop_rotate_indexed(maps, torch.arange(B, dtype=torch.int32, device=maps.device), maps.new_zeros((B, 2)),
                                             maps.new_zeros((B,)), map_ppm, map_crop, *planner.offsets()))
    if K:
        both = planner.cast(torch.cat([other_embd, ego_embd]), mode="ego")      # (one cast() over others + ego, as forward)
        other_cast, ego_cast = both[:K], both[K:]
    else:
        ego_cast = planner.cast(ego_embd, mode="ego")
        other_cast, other_cmds = torch.zeros((0, planner.num_cmds, planner.num_plan, 2), **z), torch.zeros((0, planner.num_cmds), **z)
    ego_plan = planner.plan(ego_embd, nxps, cast_locs=ego_cast, pixels_per_meter=ppm, crop_size=crop)
    return BatchInference(pick["other_locs"], other_cast, other_cmds, ego_plan, ego_cast, planner.cast_cmd_pred(ego_embd), pick["sample"], pick["actor"])


class PlannerBase(Engine):
    """What UniPlanner and BEVPlanner share: the conv engines' cache (Engine), cast()/plan() on the HIP GRU kernels, the cached crop
    offsets and the rotated crop.  Expects self.num_plan, self.num_plan_iter, self.num_cmds, self.plan_gru, self.plan_mlp,
    self.offset_x / offset_y and a _cast_modules() -> (grus, mlps) hook."""

    def _dec(self, device):
        d = getattr(self, "_dec_cache", None)
        if d is None or d["device"] != device:
            grus, mlps = self._cast_modules()
            d = dict(device=device, cast=stack_cast_weights(grus, mlps, device), plan=plan_weights(self.plan_gru, self.plan_mlp, device))
            object.__setattr__(self, "_dec_cache", d)
        return d

    def _drop(self):
        super()._drop()
        object.__setattr__(self, "_dec_cache", None)
        object.__setattr__(self, "_offsets", None)

    def _mark_stale(self):
        """Parameters may have changed in place (train()/eval() toggle, load_state_dict): the conv engines re-pack themselves at
        their next use; the stacked decoder weights and the cached offsets are plain copies, so they are dropped and rebuilt."""
        super()._mark_stale()
        object.__setattr__(self, "_dec_cache", None)
        object.__setattr__(self, "_offsets", None)

    def offsets(self):
        """(offset_x, offset_y) as host floats, read from the parameters once (no device->host sync per frame;
        keeps the forward HIP-graph capturable)."""
        if getattr(self, "_offsets", None) is None:
            object.__setattr__(self, "_offsets", (float(self.offset_x), float(self.offset_y)))
        return self._offsets

    def crop_feature(self, features, rel_locs, rel_oris, pixels_per_meter=4, crop_size=96, map_index=None, amax=None):
        """map_index (int32, per crop): take crop i from features[map_index[i]] instead of features[i] - the training
        forwards crop several vehicles out of each sample's map without materialising one copy of the map per vehicle.
        amax (eval, no map_index): the ops.Amax of the feature map - a bilinear crop never exceeds the map's largest magnitude, so
        the crops carry it on to the stem convolution (LAV_CONV_F16X3's scale, lav_conv2d_amax)."""
        ox, oy = self.offsets()
        if map_index is not None and features.is_cuda and (_hip_train("CROP") or not self.training):   # HIP forward + backward (autograd.Function)
            return ops.crop_rotate_indexed(features, map_index, rel_locs, rel_oris, pixels_per_meter, crop_size, ox, oy)
        if map_index is not None:
            features = features[map_index.long()]
        if self.training:   # autograd path (affine_grid + grid_sample)
            return crop_feature_torch(features, rel_locs, rel_oris, pixels_per_meter, crop_size, ox, oy)
        crops = crop_feature(features, rel_locs, rel_oris, pixels_per_meter, crop_size, ox, oy)
        return ops.tag_amax(crops, amax) if map_index is None else crops

    def cast(self, embd, mode="ego"):
        """(B,512) -> (B, num_cmds, num_plan, 2).  Both modes use the *_ego GRUs, as the reference does
        (uniplanner.py:296-300)."""
        if self.training:
            return self._cast_torch(embd)
        w = self._dec(embd.device)["cast"]
        return ops.gru_cast(embd, w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"], w["mlp_w"], w["mlp_b"], self.num_plan)

    def plan(self, embd, nxp, cast_locs=None, pixels_per_meter=4, crop_size=96, cmd: int = -1, impl: str = "auto"):
        """(B,512),(B,2),(B,num_cmds,T,2) -> (B, num_plan_iter, num_cmds, T, 2)  (uniplanner.py:255-286).
        cmd >= 0 evaluates only that command branch and returns (B, iters, 1, T, 2).  impl: see ops.gru_plan."""
        if cast_locs is None:
            cast_locs = self.cast(embd)
        if self.training:
            return self._plan_torch(embd, nxp, cast_locs.detach(), pixels_per_meter, crop_size, cmd)
        w = self._dec(embd.device)["plan"]
        return ops.gru_plan(embd, nxp, cast_locs.detach(), w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"], w["mlp_w"],
                            w["mlp_b"], self.num_plan_iter, cmd, pixels_per_meter, crop_size, impl=impl)

    # ---- train mode: the same decoders as differentiable torch ops (uniplanner.py:255-308) ----------------------
    def _cast_torch(self, embd):
        """Six independent GRU(512 -> 64) decoders on the same input == ONE GRU(512 -> 384) whose recurrent matrix is
        block diagonal (gate-major stacking [r | z | n], each 6 x 64 rows).  The combined weights are assembled from the
        six modules' parameters with differentiable torch ops on every call, so gradients reach the original tensors;
        MIOpen then runs one RNN call instead of six (each ~2 ms forward + backward at these sizes)."""
        grus, mlps = self._cast_modules()
        nc, H = len(grus), grus[0].hidden_size
        gate = lambda name, g: torch.cat([getattr(m, name).view(3, H, -1)[g] for m in grus], dim=0)
        w_ih = torch.cat([gate("weight_ih_l0", g) for g in range(3)], dim=0)                                   # (3*nc*H, 512)
        w_hh = torch.cat([torch.block_diag(*[m.weight_hh_l0.view(3, H, H)[g] for m in grus]) for g in range(3)], dim=0)
        b_ih = torch.cat([torch.cat([m.bias_ih_l0.view(3, H)[g] for m in grus]) for g in range(3)])
        b_hh = torch.cat([torch.cat([m.bias_hh_l0.view(3, H)[g] for m in grus]) for g in range(3)])
        B = embd.size(0)
        u = embd[:, None].expand(-1, self.num_plan, -1).contiguous()
        h0 = embd.new_zeros((1, B, nc * H))
        if embd.is_cuda and _hip_train("GRU"):   # liblav_amd's sequence GRU: the input is the same at every step, so it is projected once
            out = ops.gru_seq(F.linear(embd, w_ih, b_ih), h0[0], w_hh, b_hh, self.num_plan)                       # (B, T, nc*H)
        else:
            out, _ = torch._VF.gru(u, h0, [w_ih, w_hh, b_ih, b_hh], True, 1, 0.0, self.training, False, True)
        out = out.view(B, self.num_plan, nc, H)
        w = torch.stack([m.weight for m in mlps])                                                               # (nc, 2, H)
        b = torch.stack([m.bias for m in mlps])                                                                 # (nc, 2)
        step = torch.einsum("btch,cdh->bctd", out, w) + b[None, :, None, :]
        return torch.cumsum(step, dim=2)

    def _plan_torch(self, embd, nxp, plan_loc, pixels_per_meter, crop_size, cmd=-1):
        """The reference loops over the six command branches (uniplanner.py:264-275); they share the GRU and never interact,
        so they are run as ONE batched GRU call per refinement iteration (sequences ordered branch-major) - MIOpen's RNN
        costs ~2 ms per call forward + backward whatever the batch, which made 30 calls the bulk of a training step."""
        B, T = embd.size(0), self.num_plan
        if cmd >= 0:
            plan_loc = plan_loc[:, cmd:cmd + 1]
        nb = plan_loc.size(1)
        u0 = (nxp * pixels_per_meter / crop_size * 2 - 1)[:, None].expand(-1, T, -1).repeat(nb, 1, 1)        # (nb*B, T, 2)
        h0 = embd.repeat(nb, 1)[None].contiguous()                                                            # (1, nb*B, 512)
        outs = []
        for _ in range(self.num_plan_iter):
            u = torch.cat([u0, plan_loc.transpose(0, 1).reshape(nb * B, T, 2)], dim=2)
            if u.is_cuda and _hip_train("GRU"):
                g = self.plan_gru
                hseq = ops.gru_seq(F.linear(u, g.weight_ih_l0, g.bias_ih_l0), h0[0], g.weight_hh_l0, g.bias_hh_l0, T)
            else:
                hseq = self.plan_gru(u, h0)[0]
            step = torch.cumsum(self.plan_mlp(hseq), dim=1)                                                   # (nb*B, T, 2)
            plan_loc = step.view(nb, B, T, 2).transpose(0, 1) + plan_loc
            outs.append(plan_loc)
        return torch.stack(outs, dim=1)
