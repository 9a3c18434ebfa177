"""The brake-net trainer (lav/lav_privileged_v2.py:30, 46, 186-216 `LAV.train_bra`, driven by lav/train_bra_v2.py) with one process
per GPU: RGBBrakePredictionModel([4, 10, 18]), Adam over all of it, one step per batch of (wide image, tele image, their labels,
brake flag).  The loss is the reference's

    BCE(pred_bra, bra) + 1/2 CE(up4(seg_head(x1)), sem1) + 1/2 CE(up4(seg_head(x2)), sem2)

The step composes the model's pieces itself (lav_amd.rgb's forwards are the frame graphs' and stay as they are):
    trunk      normalize -> ResNet-18 on hipnn.conv_module + bn_act (ResNet.forward_train), the seg head's BatchNorm + ReLU on bn_act
    attention  hipnn.attn_pool_train (lav_attn_train_*: the K/V projection folded around the single query)
    seg loss   hipnn.seg_cross_entropy_up (lav_seg_xent_up_forward: the x4 upsampling folded into the loss)
Which of them run on liblav_amd by default is hipnn.brake_piece_on's measured table; LAV_TRAIN_CONV=torch gives the
all-torch step.  On a CPU tensor every piece is the reference's torch ops."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .. import synth
from .lav import _ddp
from .optim import make_adam

BRA_LABELS = [4, 10, 18]        # lav_privileged_v2.py:30 (hard-coded there; not config_v2's seg_channels)
SEG_SCALE = 4                   # the seg head's logits are at stride 4 of the image (F.interpolate(scale_factor=4))


class _BrakeStep(nn.Module):
    """The train-mode forward of RGBBrakePredictionModel(mask=True) up to the seg head's stride-4 logits, behind ONE forward so
    that DistributedDataParallel sees the whole autograd graph."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def _trunk(self, rgb):
        from .hipnn import brake_piece_on
        m = self.model
        x = m.normalize(rgb / 255.)
        if x.is_cuda and brake_piece_on("trunk"):
            return m.conv_backbone.forward_train(x)
        return m.conv_backbone(x)        # (_ResNet18's train-mode forward: torch ops)

    def _seg_head(self, x):
        from .hipnn import bn_act, brake_piece_on
        up = self.model.seg_head.upconv      # [ConvTranspose2d, BatchNorm2d, ReLU] x 3, Conv2d(64, K, 1)
        if not (x.is_cuda and brake_piece_on("trunk")):
            return up(x)
        for j in range(0, len(up) - 1, 3):   # (the transposed convolutions stay on torch / MIOpen, as in train_full)
            x = bn_act(up[j + 1], up[j](x), relu_post=True)
        return up[len(up) - 1](x)

    def _attn(self, attn, x):
        from .hipnn import attn_pool_train, brake_piece_on
        return attn_pool_train(attn, x) if x.is_cuda and brake_piece_on("attn") else attn(x)

    def forward(self, rgb1, rgb2):
        m = self.model
        x1, x2 = self._trunk(rgb1), self._trunk(rgb2)
        pred = m.classifier(torch.cat([self._attn(m.attn1, x1), self._attn(m.attn2, x2)], dim=1))[:, 0]
        return pred, self._seg_head(x1), self._seg_head(x2)


def seg_loss_up(logits, labels):
    """F.cross_entropy(F.interpolate(logits, scale_factor=4), labels): hipnn.seg_cross_entropy_up where the "xent" piece is on, the
    torch ops otherwise."""
    from .hipnn import brake_piece_on, seg_cross_entropy_up
    if logits.is_cuda and brake_piece_on("xent"):
        return seg_cross_entropy_up(logits, labels, SEG_SCALE)
    return F.cross_entropy(F.interpolate(logits, scale_factor=SEG_SCALE), labels.long())


class BrakeTrainer:
    def __init__(self, cfg, device, checkpoints=None):
        """cfg: a TrainConfig (lr, conv_precision).  checkpoints: optional dict with 'bra' (a state_dict of RGBBrakePredictionModel);
        without it the weights are synth.seeded_state_dict(model, prefix="bra.").  The reference starts the trunk from ImageNet
        (RGBBrakePredictionModel(..., pretrained=True) -> load_state_dict_from_url): that is a download, and does not exist here."""
        from ..rgb import RGBBrakePredictionModel
        self.cfg, self.device = cfg, torch.device(device)
        self.steps = 0
        self.log_view = False           # set by the driver around a step whose picture is wanted (--log-dir): train_bra then returns "view"
        ck = checkpoints or {}
        self.bra_model = RGBBrakePredictionModel(BRA_LABELS)
        self.bra_model.load_state_dict(ck.get("bra") or synth.seeded_state_dict(self.bra_model, prefix="bra."))
        self.bra_model.to(self.device).train()
        # ResNet.fc rides in the checkpoints but no forward uses it: without a gradient it would keep its DDP bucket from ever
        # becoming ready (Adam skips a parameter without a gradient either way: the steps are the reference's)
        for p in self.bra_model.conv_backbone.fc.parameters():
            p.requires_grad_(False)
        self.bra_optim = make_adam(self.bra_model.parameters(), cfg, [self.bra_model], saved={"bra": self.bra_model})     # lav_privileged_v2.py:46 (Adam), no scheduler
        self.bra_ddp = _ddp(_BrakeStep(self.bra_model), self.device)

    def state_dict(self, model_name="bra"):
        if model_name != "bra":
            raise ValueError(f"BrakeTrainer: no model {model_name!r} (bra)")
        return self.bra_model.state_dict()

    def train_bra(self, rgb1, rgb2, sem1, sem2, bra):
        """One Adam step on (B, H1, W1, 3) / (B, H2, W2, 3) uint8 RGB images (wide, tele), their (B, H, W) integer labels and the
        (B,) 0/1 brake flags.  Returns the reference's opt_info: loss, rgb1, rgb2 (sample 0, HWC uint8), bra, pred_bra,
        pred_sem1, pred_sem2 (the full-resolution argmax of sample 0)."""
        from .hipnn import use_precision
        d = self.device
        rgb1 = rgb1.float().permute(0, 3, 1, 2).to(d)
        rgb2 = rgb2.float().permute(0, 3, 1, 2).to(d)
        # uint8 labels stay uint8 for lav_seg_xent_up_forward (an eighth of int64's bytes); the torch path widens them itself
        sem1, sem2 = (s.to(d) if s.dtype == torch.uint8 else s.long().to(d) for s in (sem1, sem2))
        bra = bra.float().to(d)
        # f16x3 convolutions in the trunk: 48.6 ms per batch-52 step against 53.8 with bf16x6 (profiles/train_bra_probe.json)
        with use_precision(self.cfg.conv_precision or "f16x3"):
            pred_bra, logit1, logit2 = self.bra_ddp(rgb1, rgb2)
            loss = F.binary_cross_entropy(pred_bra, bra) + 1 / 2 * seg_loss_up(logit1, sem1) + 1 / 2 * seg_loss_up(logit2, sem2)
            self.bra_optim.zero_grad()
            loss.backward()
        self.bra_optim.step()
        self.steps += 1
        loss_v, bra_v, pred_v = torch.stack([loss.detach(), bra[0], pred_bra[0].detach()]).tolist()
        up = lambda a: a.repeat(SEG_SCALE, axis=0).repeat(SEG_SCALE, axis=1)   # nearest x4: the argmax of the upsampled logits
        info = dict(loss=loss_v, rgb1=rgb1[0].permute(1, 2, 0).byte().cpu().numpy(), rgb2=rgb2[0].permute(1, 2, 0).byte().cpu().numpy(),
                    bra=bra_v, pred_bra=pred_v, pred_sem1=up(logit1[0].detach().argmax(0).cpu().numpy()),
                    pred_sem2=up(logit2[0].detach().argmax(0).cpu().numpy()))
        if self.log_view:      # (lav_amd.train.log_view.bra_frame) the logits of sample 0 stay on the device, at the resolution the heads emit
            info["view"] = dict(rgb1=rgb1[0].permute(1, 2, 0).byte().contiguous(), rgb2=rgb2[0].permute(1, 2, 0).byte().contiguous(), bra=bra_v,
                                pred_bra=pred_v, pred_sem1=logit1[0].detach().float().contiguous(), pred_sem2=logit2[0].detach().float().contiguous())
        return info
