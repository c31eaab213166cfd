"""DINO self-distillation (Caron et al. 2021, "Emerging Properties in Self-Supervised Vision Transformers"): the multi-crop loss on the fused HIP
kernels of csrc/dino_loss.hip, the projection head, the teacher-temperature schedule and the teacher head's EMA.  The backbone's teacher is
``AveragedModel(model, avg="ema")``; the views come from ``DeviceAugment``; ``DiChaViT.forward_views`` runs them under one set of operand copies.

    loss = dino_loss(student_head(feats), teacher_head(teacher_feats), teacher_temp, n_views=V)
    loss.backward(); opt.step(); teacher.update_parameters(model); update_teacher_head(teacher_head, student_head, m); dino_loss.update_center()

Masked patch-token distillation (iBOT, Zhou et al. 2022) adds the patch rows: ``model.add_mask_token()``, ``BlockMaskGenerator`` for the masks,
``forward_views(..., masks=, patch_views=)`` for the patch tokens, and ``IBOTPatchLoss`` on the fused kernels of csrc/ibot_loss.hip.

The losses run only on the GPU and only in fp32: there is no CPU fallback and no bf16 form."""
from __future__ import annotations

import math
import random
from typing import List, NamedTuple

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


class _IBOTLossFn(torch.autograd.Function):
    """student [R, K], teacher [R, K], center [K], weights [R] -> loss [] (dcv_ibot_loss_fwd), tsum [K] (not differentiable).  Backward:
    dcv_ibot_loss_bwd with grad_output as its device scalar (first order only); the teacher, the centre and the weights get no gradient.  Without
    a gradient to compute nothing is saved and no statistics are written."""

    @staticmethod
    def forward(ctx, student, teacher, center, weights, student_temp, teacher_temp, save):
        R, K = student.shape
        loss = torch.empty(1, dtype=torch.float32, device=student.device)
        tsum = torch.empty(K, dtype=torch.float32, device=student.device)
        s_stats = torch.empty(R, 3, dtype=torch.float32, device=student.device) if save else None
        t_stats = torch.empty(R, 4, dtype=torch.float32, device=student.device) if save else None
        hip.ibot_loss_fwd(student, teacher, center, weights, student_temp, teacher_temp, loss, s_stats, t_stats, tsum)
        if save:
            ctx.save_for_backward(student, teacher, center, weights, s_stats, t_stats)
            ctx.cfg = (student_temp, teacher_temp)
        ctx.mark_non_differentiable(tsum)
        return loss.view(()), tsum

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, _dtsum):
        student, teacher, center, weights, s_stats, t_stats = ctx.saved_tensors
        student_temp, teacher_temp = ctx.cfg
        dS = torch.empty_like(student)
        hip.ibot_loss_bwd(student, teacher, center, weights, student_temp, teacher_temp, s_stats, t_stats,
                          dloss.reshape(1).float().contiguous(), dS)
        return dS, None, None, None, None, None, None


class IBOTPatchLoss(nn.Module):
    """Masked patch-token distillation (iBOT, Zhou et al. 2022; the patch term of DINOv2) over the R masked tokens of a batch:

        loss = patch_loss(student_patch_logits [R, K], teacher_patch_logits [R, K], weights [R], teacher_temp)
             = sum_r weights[r] * sum_k -q_r[k] log p_r[k],   q_r = softmax((T_r - center) / teacher_temp),  p_r = softmax(S_r / student_temp)

    Row r of both logit matrices belongs to the same masked token (BlockMaskGenerator's `rows`, gathered from the student's and the teacher's
    patch tokens); `weights` carries the per-image mean and the batch mean (BlockMaskGenerator's `weights`).  The teacher logits get no gradient.
    Forward and backward are one fused pass each over the logits (csrc/ibot_loss.hip).  `center` [K] is a buffer; it moves only in
    update_center(): center <- m center + (1 - m) tsum / R, with tsum the unweighted column sums of the teacher logits of the last forward
    (tsum and R all_reduced first when torch.distributed is initialised).  GPU tensors, fp32 only."""

    def __init__(self, out_dim: int, student_temp: float = 0.1, center_momentum: float = 0.9):
        super().__init__()
        self.out_dim, self.student_temp, self.center_momentum = int(out_dim), float(student_temp), float(center_momentum)
        self.register_buffer("center", torch.zeros(self.out_dim))
        self._tsum = None
        self._rows = 0

    def forward(self, student_patch_logits: torch.Tensor, teacher_patch_logits: torch.Tensor, weights: torch.Tensor,
                teacher_temp: float) -> torch.Tensor:
        for t, name in ((student_patch_logits, "student_patch_logits"), (teacher_patch_logits, "teacher_patch_logits"), (weights, "weights")):
            if not t.is_cuda:
                raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
            if t.dtype != torch.float32:
                raise RuntimeError(f"{name}: expected {torch.float32}, got {t.dtype}")
        S, T = student_patch_logits, teacher_patch_logits
        if S.dim() != 2 or S.shape[1] != self.out_dim or T.shape != S.shape or S.shape[0] < 1:
            raise ValueError(f"IBOTPatchLoss: expected two [R, {self.out_dim}] logit matrices, R >= 1")
        if weights.numel() != S.shape[0]:
            raise ValueError("IBOTPatchLoss: weights holds one float per row")
        student = S if S.stride(1) == 1 else S.contiguous()
        teacher = T.detach()
        teacher = teacher if teacher.stride(1) == 1 else teacher.contiguous()
        with torch.autocast(device_type="cuda", enabled=False):
            loss, tsum = _IBOTLossFn.apply(student, teacher, self.center, weights.detach().contiguous(), self.student_temp, float(teacher_temp),
                                           torch.is_grad_enabled() and student.requires_grad)  # under no_grad nothing is saved
        self._tsum, self._rows = tsum, teacher.shape[0]
        return loss

    @torch.no_grad()
    def update_center(self) -> None:
        if self._tsum is None:
            raise RuntimeError("IBOTPatchLoss.update_center: no forward since the last update")
        tsum, rows = self._tsum, self._rows
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(tsum)
            n = torch.tensor([float(rows)], device=tsum.device)
            torch.distributed.all_reduce(n)  # the masked-token count differs from rank to rank
            self.center.copy_(self.center * self.center_momentum + tsum * ((1.0 - self.center_momentum) / n))
        else:
            self.center.copy_(center_update(self.center, tsum, rows, self.center_momentum))
        self._tsum = None


class MaskBatch(NamedTuple):
    """What BlockMaskGenerator returns: mask bool [B, C, gh, gw] (CPU); mask_dev uint8 [B, C * n]; rows int64 [R], the flat indices (b * C * n + t) of
    the masked tokens in (b, t) order; weights fp32 [R] = 1 / (max(m_b, 1) * B) with m_b the masked count of the row's image."""
    mask: torch.Tensor
    mask_dev: torch.Tensor
    rows: torch.Tensor
    weights: torch.Tensor


class BlockMaskGenerator:
    """Block-wise patch masks for masked-token distillation, drawn on the host from an own random.Random (it follows no outside RNG stream).

        gen = BlockMaskGenerator((14, 14), channels=8); m = gen(B)      # m.mask, m.mask_dev, m.rows, m.weights

    Per image: with probability mask_prob the image is masked.  The target count per gh x gw plane is round(u * gh * gw), u uniform in mask_ratio.
    A plane is filled by rectangles: aspect ratio log-uniform in [0.3, 1 / 0.3], area uniform between 1 and what the target still lacks (at least
    1), placement uniform; a rectangle's unmasked cells are added in row-major order only as far as the target still lacks, so a plane ends with
    exactly its target count; after 10 x target draws without completion the remainder is filled with uniformly chosen unmasked cells.
    per_channel=True: every channel plane gets its own draw with the image's ratio u (a masked token keeps its channel embedding and position, so
    the student knows which channel at which position it predicts); per_channel=False: one plane shared by all channels.  The uploads come from
    pinned memory (non_blocking): no device synchronisation.  device=None keeps everything on the CPU (tests)."""

    def __init__(self, grid, channels: int, mask_ratio=(0.1, 0.5), mask_prob: float = 0.5, per_channel: bool = True, seed: int = 0,
                 device="cuda"):
        self.gh, self.gw = (int(grid), int(grid)) if isinstance(grid, int) else (int(grid[0]), int(grid[1]))
        self.channels, self.per_channel = int(channels), bool(per_channel)
        self.lo, self.hi = float(mask_ratio[0]), float(mask_ratio[1])
        self.mask_prob = float(mask_prob)
        if self.gh < 1 or self.gw < 1 or self.channels < 1 or not 0.0 <= self.lo <= self.hi <= 1.0 or not 0.0 <= self.mask_prob <= 1.0:
            raise ValueError("BlockMaskGenerator: grid and channels >= 1, 0 <= mask_ratio[0] <= mask_ratio[1] <= 1, 0 <= mask_prob <= 1")
        self.rng = random.Random(seed)
        self.device = device

    def _plane(self, target: int) -> torch.Tensor:
        gh, gw, rng = self.gh, self.gw, self.rng
        plane = torch.zeros(gh, gw, dtype=torch.bool)
        count, log_lo, log_hi = 0, math.log(0.3), math.log(1.0 / 0.3)
        for _ in range(10 * target):
            if count >= target:
                break
            area = rng.uniform(1.0, float(max(target - count, 1)))
            aspect = math.exp(rng.uniform(log_lo, log_hi))
            h = min(max(int(round(math.sqrt(area * aspect))), 1), gh)
            w = min(max(int(round(math.sqrt(area / aspect))), 1), gw)
            top, left = rng.randint(0, gh - h), rng.randint(0, gw - w)
            for i in range(top, top + h):
                for j in range(left, left + w):
                    if count < target and not plane[i, j]:
                        plane[i, j] = True
                        count += 1
        if count < target:
            free = [k for k in range(gh * gw) if not plane[k // gw, k % gw]]
            for k in rng.sample(free, target - count):
                plane[k // gw, k % gw] = True
        return plane

    def __call__(self, B: int) -> MaskBatch:
        C, gh, gw = self.channels, self.gh, self.gw
        mask = torch.zeros(B, C, gh, gw, dtype=torch.bool)
        for b in range(B):
            if self.rng.random() >= self.mask_prob:
                continue
            target = int(round(self.rng.uniform(self.lo, self.hi) * gh * gw))
            if self.per_channel:
                for c in range(C):
                    mask[b, c] = self._plane(target)
            else:
                mask[b] = self._plane(target)
        flat = mask.view(B, C * gh * gw)
        rows = flat.flatten().nonzero().flatten()
        per_image = flat.sum(1).clamp(min=1).to(torch.float32)
        weights = (1.0 / (per_image * B))[rows // (C * gh * gw)]
        mask_u8 = flat.to(torch.uint8)
        if self.device is None:
            return MaskBatch(mask, mask_u8, rows, weights)
        up = lambda t: t.pin_memory().to(self.device, non_blocking=True)  # noqa: E731
        return MaskBatch(mask, up(mask_u8), up(rows), up(weights))


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
