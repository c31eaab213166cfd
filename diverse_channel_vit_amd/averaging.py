"""Weight averaging for the arena-backed DiChaViT: SWA / SWAD and EMA of the weights as ONE launch over the parameter arena.

``AveragedModel`` mirrors ``torch.optim.swa_utils.AveragedModel`` wherever the reference trainer touches it (``train.swa`` /
``train.swad``: trainer.py:242-244 builds it, :810-812 updates it once per epoch, :957-959 after every optimizer step, :1334-1336 swaps
it in for the model): ``module`` is a deep copy, ``n_averaged`` a long buffer, ``forward`` runs the copy, and the state dict has torch's
layout (``n_averaged`` + ``module.*``), so a state dict written by either class loads into the other.

Every parameter of the model lives in one flat fp32 arena (DiChaViT._ensure_arena) and a deep copy has an arena of the same layout, so
``update_parameters`` is a single streaming pass ``avg <- lerp(avg, p, w)`` over two flat buffers (dcv_avg_update), with the count read
on the device: no host read and no host branch, legal inside a captured step (``GraphedTrainStep(..., averager=...)``) and identical
outside one.  torch's class walks ~150 parameter views through multi-tensor lerps, branches on the host on ``n_averaged`` and copies it
to the device on every update.

Works unchanged with: ``freeze_prefix(k)`` (the average of a parameter that never moves is that parameter, exactly: fma(w, 0, a) = a);
``DataParallel`` (every rank applies the same update to the same weights: no communication; the copy is detached from the reducer);
``torch.optim.swa_utils.SWALR(HipAdamW(...))`` (it only edits ``param_groups[i]["lr"]``, which HipAdamW re-reads every step, in
capturable mode too); ``torch.optim.swa_utils.update_bn`` (returns at once: the model has no BatchNorm)."""
from __future__ import annotations

import copy

import torch
from torch import nn

from . import hip


class AveragedModel(nn.Module):
    """avg="swa": the running equal-weight mean of the parameters seen by update_parameters (w = 1 / (n_averaged + 1));
    avg="ema": avg <- decay * avg + (1 - decay) * p.  In both, the first update copies the parameters.  ``decay`` may be changed between
    updates in eager mode (a captured step keeps the weight it was captured with)."""

    def __init__(self, model, avg: str = "swa", decay: float = 0.999):
        super().__init__()
        if avg not in ("swa", "ema"):
            raise ValueError(f"avg={avg!r}: expected 'swa' or 'ema'")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"decay={decay!r}: expected a value in [0, 1]")
        self.avg, self.decay = avg, float(decay)
        # the copy owns its parameters (Parameter.__deepcopy__ clones them) and rebuilds its own arena and operand copies on first use; the
        # source's device buffers and its DataParallel reducer are left out of the copy instead of being duplicated and then dropped
        skip = ("_dp", "_arena", "_grad_arena", "_grad_scratch", "_ops", "_side")
        memo = {id(v): None for v in (getattr(model, k, None) for k in skip) if v is not None}
        self.module = copy.deepcopy(model, memo)
        self.module._dp = None
        self.register_buffer("n_averaged", torch.tensor(0, dtype=torch.long))

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    @torch.no_grad()
    def update_parameters(self, model) -> None:
        """One dcv_avg_update over the whole arena (model -> self.module) with the count read from ``n_averaged`` on the device, then
        ``n_averaged += 1`` on the same stream."""
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("diverse_channel_vit_amd runs only on an MI355X: move the model to the GPU before averaging its weights "
                               "(there is no CPU fallback)")
        hip.load()
        mine = self.module
        if next(mine.parameters()).device != dev:
            mine.to(dev)
        if self.n_averaged.device != dev:
            self.n_averaged = self.n_averaged.to(dev)
        model._ensure_arena(dev)
        mine._ensure_arena(dev)
        src, dst = model._arena, mine._arena
        if src.numel() != dst.numel():
            raise ValueError(f"the averaged copy's arena holds {dst.numel()} floats, the model's {src.numel()}: they are not the same architecture")
        if list(model._all_off) != list(mine._all_off):
            k = next(i for i, (a, b) in enumerate(zip(model._all_off, mine._all_off)) if a != b)
            raise ValueError(f"parameter slot {k} starts at float {mine._all_off[k]} in the averaged copy's arena and at {model._all_off[k]} in the "
                             "model's: they are not the same architecture")
        hip.avg_update(dst, src, src.numel(), hip.AVG_SWA if self.avg == "swa" else hip.AVG_EMA,
                       ema_weight=0.0 if self.avg == "swa" else float(1.0 - self.decay), n_averaged_dev=self.n_averaged)
        self.n_averaged.add_(1)
