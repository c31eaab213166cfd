"""DINO self-distillation (Caron et al. 2021, "Emerging Properties in Self-Supervised Vision Transformers"): the multi-crop loss on the fused HIP
kernels of csrc/dino_loss.hip, the projection head, the teacher-temperature schedule and the teacher head's EMA.  The backbone's teacher is
``AveragedModel(model, avg="ema")``; the views come from ``DeviceAugment``; ``DiChaViT.forward_views`` runs them under one set of operand copies.

    loss = dino_loss(student_head(feats), teacher_head(teacher_feats), teacher_temp, n_views=V)
    loss.backward(); opt.step(); teacher.update_parameters(model); update_teacher_head(teacher_head, student_head, m); dino_loss.update_center()

The loss runs only on the GPU and only in fp32: there is no CPU fallback and no bf16 form."""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import hip


class _DINOLossFn(torch.autograd.Function):
    """student [V*B, K], teacher [2*B, K], center [K] -> loss [] (dcv_dino_loss_fwd), tsum [K] (not differentiable).  Backward: dcv_dino_loss_bwd with
    grad_output as its device scalar (first order only: create_graph=True raises); the teacher and the centre get no gradient.  Without a gradient to compute nothing is saved and no statistics
    are written."""

    @staticmethod
    def forward(ctx, student, teacher, center, V, student_temp, teacher_temp, save):
        B = student.shape[0] // V
        loss = torch.empty(1, dtype=torch.float32, device=student.device)
        tsum = torch.empty(student.shape[1], dtype=torch.float32, device=student.device)
        s_stats = torch.empty(V * B, 2, dtype=torch.float32, device=student.device) if save else None
        t_stats = torch.empty(2 * B, 3, dtype=torch.float32, device=student.device) if save else None
        hip.dino_loss_fwd(student, teacher, center, V, student_temp, teacher_temp, loss, s_stats, t_stats, tsum)
        if save:
            ctx.save_for_backward(student, teacher, center, s_stats, t_stats)
            ctx.cfg = (V, student_temp, teacher_temp)
        ctx.mark_non_differentiable(tsum)
        return loss.view(()), tsum

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, _dtsum):
        student, teacher, center, s_stats, t_stats = ctx.saved_tensors
        V, student_temp, teacher_temp = ctx.cfg
        dS = torch.empty_like(student)
        hip.dino_loss_bwd(student, teacher, center, V, student_temp, teacher_temp, s_stats, t_stats, dloss.reshape(1).float().contiguous(), dS)
        return dS, None, None, None, None, None, None


def center_update(center: torch.Tensor, tsum: torch.Tensor, rows: int, momentum: float) -> torch.Tensor:
    """DINOLoss.update_center's arithmetic: momentum * center + (1 - momentum) * tsum / rows, with tsum the column sums of the teacher logits over
    `rows` = 2 B world rows.  Plain torch on [K]; works on CPU tensors."""
    return center * momentum + tsum * ((1.0 - momentum) / rows)


class DINOLoss(nn.Module):
    """DINO's loss (facebookresearch DINO, DINOLoss) for V views of which the first two are the global crops:

        loss = dino_loss(student_logits [V*B, K], teacher_logits [2*B, K], teacher_temp, n_views=V)

    student_logits are view-major (the rows of view 0, then view 1, ...), as DiChaViT.forward_views and the head deliver them; teacher_logits are
    the teacher's logits of the two global crops and get no gradient.  Forward and backward are one fused pass each over the logits (csrc/
    dino_loss.hip): no softmax, log-softmax or pairwise product is materialised.  `center` [K] is a buffer; it moves only in update_center(),
    called after the optimiser step: center <- m center + (1 - m) tsum / (2 B world), with tsum the column sums of the teacher logits of the last
    forward (all_reduced first when torch.distributed is initialised).  GPU tensors, fp32 only."""

    def __init__(self, out_dim: int, student_temp: float = 0.1, center_momentum: float = 0.9):
        super().__init__()
        self.out_dim, self.student_temp, self.center_momentum = int(out_dim), float(student_temp), float(center_momentum)
        self.register_buffer("center", torch.zeros(self.out_dim))
        self._tsum = None
        self._rows = 0

    def forward(self, student_logits: torch.Tensor, teacher_logits: torch.Tensor, teacher_temp: float, n_views: int) -> torch.Tensor:
        for t, name in ((student_logits, "student_logits"), (teacher_logits, "teacher_logits")):
            if not t.is_cuda:
                raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
            if t.dtype != torch.float32:
                raise RuntimeError(f"{name}: expected {torch.float32}, got {t.dtype}")
        V = int(n_views)
        if student_logits.dim() != 2 or teacher_logits.dim() != 2 or student_logits.shape[1] != self.out_dim or teacher_logits.shape[1] != self.out_dim:
            raise ValueError(f"DINOLoss: expected [rows, {self.out_dim}] logits")
        if V < 2 or student_logits.shape[0] % V or student_logits.shape[0] // V * 2 != teacher_logits.shape[0]:
            raise ValueError("DINOLoss: student_logits holds n_views * B rows (n_views >= 2, the two global crops first), teacher_logits 2 * B")
        student = student_logits if student_logits.stride(1) == 1 else student_logits.contiguous()
        teacher = teacher_logits.detach()
        teacher = teacher if teacher.stride(1) == 1 else teacher.contiguous()
        with torch.autocast(device_type="cuda", enabled=False):
            loss, tsum = _DINOLossFn.apply(student, teacher, self.center, V, self.student_temp, float(teacher_temp),
                                           torch.is_grad_enabled() and student.requires_grad)  # under no_grad nothing is saved
        self._tsum, self._rows = tsum, teacher.shape[0]
        return loss

    @torch.no_grad()
    def update_center(self) -> None:
        if self._tsum is None:
            raise RuntimeError("DINOLoss.update_center: no forward since the last update")
        tsum, rows = self._tsum, self._rows
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(tsum)
            rows *= torch.distributed.get_world_size()
        self.center.copy_(center_update(self.center, tsum, rows, self.center_momentum))
        self._tsum = None


class DINOHead(nn.Module):
    """DINO's projection head: an MLP of `nlayers` Linear layers with GELU between them (in_dim -> hidden_dim -> ... -> bottleneck_dim), L2
    normalisation, and a weight-normalised Linear without bias to out_dim prototypes; norm_last_layer fills weight_g with 1 and freezes it.
    Linear weights are drawn as DINO draws them, trunc_normal_(std=0.02) with its cut at +-2; biases are 0.  Plain torch: the head runs on the
    vendor GEMM, as the classifier head does."""

    def __init__(self, in_dim: int, out_dim: int = 65536, hidden_dim: int = 2048, bottleneck_dim: int = 256, nlayers: int = 3,
                 norm_last_layer: bool = True):
        super().__init__()
        nlayers = max(int(nlayers), 1)
        if nlayers == 1:
            self.mlp = nn.Linear(in_dim, bottleneck_dim)
        else:
            layers = [nn.Linear(in_dim, hidden_dim), nn.GELU()]
            for _ in range(nlayers - 2):
                layers += [nn.Linear(hidden_dim, hidden_dim), nn.GELU()]
            layers.append(nn.Linear(hidden_dim, bottleneck_dim))
            self.mlp = nn.Sequential(*layers)
        for m in self.mlp.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)
        self.last_layer = nn.utils.weight_norm(nn.Linear(bottleneck_dim, out_dim, bias=False))
        self.last_layer.weight_g.data.fill_(1)
        if norm_last_layer:
            self.last_layer.weight_g.requires_grad = False

    def bottleneck(self, x: torch.Tensor) -> torch.Tensor:
        return F.normalize(self.mlp(x), dim=-1, p=2)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.last_layer(self.bottleneck(x))


def teacher_temp_schedule(warmup_teacher_temp: float, teacher_temp: float, warmup_epochs: int, epochs: int) -> List[float]:
    """DINO's teacher temperature, one value per epoch: linear from warmup_teacher_temp to teacher_temp over the first warmup_epochs epochs (both
    ends included), then constant."""
    w = min(int(warmup_epochs), int(epochs))
    warm = [warmup_teacher_temp + (teacher_temp - warmup_teacher_temp) * i / max(w - 1, 1) for i in range(w)]
    return warm + [float(teacher_temp)] * (int(epochs) - w)


@torch.no_grad()
def update_teacher_head(teacher_head: nn.Module, student_head: nn.Module, momentum: float) -> None:
    """teacher <- momentum * teacher + (1 - momentum) * student over the head's parameters, one foreach lerp.  The backbone's EMA stays
    AveragedModel.update_parameters."""
    tp, sp = list(teacher_head.parameters()), list(student_head.parameters())
    if len(tp) != len(sp):
        raise ValueError("update_teacher_head: the heads differ in their parameters")
    torch._foreach_lerp_(tp, [s.detach() for s in sp], 1.0 - float(momentum))
