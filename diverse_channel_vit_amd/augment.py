"""The CHAMMI train-time augmentation of the reference on the device (datasets/dataset_utils.py:234-243): TPSTransform(p), then
RandomResizedCrop(size, scale, ratio, antialias=True), then RandomHorizontalFlip — for a batch of equal-size raw images that already sits on
the GPU, in two launches (csrc/augment.hip).  Normalize stays where it is: in the tokeniser, through model.set_input_normalisation.

    aug = DeviceAugment(size=224, tps_prob=0.2)
    out = aug(x_uint8)                       # [B, C, W, W] uint8 / float32 on the GPU -> float32 [B, C, 224, 224], raw units
    logits = model(out, chunk)               # the model was given set_input_normalisation(mean, std)

The parameters are drawn on the host (torch's generator; the streams of `random` / numpy / torchvision that the reference consumes cannot be
matched and are not); the B small spline systems are solved there too, in float64 (tps_coefficients).  No CPU fallback for the image work."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import hip

__all__ = ["DeviceAugment", "AugmentParams", "tps_coefficients", "tps_control_points", "regular_grid"]


def regular_grid(width: int, points_per_dim: int = 3) -> torch.Tensor:
    """The reference's _get_regular_grid of a square image: points_per_dim^2 points on [0, width]^2, float64 [k, 2]."""
    g = torch.linspace(0, width, points_per_dim, dtype=torch.float64)
    return torch.stack([g.repeat_interleave(points_per_dim), g.repeat(points_per_dim)], dim=1)


def _corners(width) -> torch.Tensor:
    w = float(width)
    return torch.tensor([[0.0, 0.0], [0.0, w], [w, 0.0], [w, w]], dtype=torch.float64)


def tps_control_points(dst: torch.Tensor, width: int) -> torch.Tensor:
    """dst [B, k, 2] -> P float64 [B, k + 4, 2]: the displaced points followed by the four fixed corners (keep_corners of the reference)."""
    dst = torch.as_tensor(dst, dtype=torch.float64)
    return torch.cat([dst, _corners(width).expand(dst.shape[0], 4, 2)], dim=1)


def tps_coefficients(dst: torch.Tensor, src: torch.Tensor, width: int) -> torch.Tensor:
    """Coefficients of the reference's INVERSE warp (_make_warp(to_points, from_points, ...), tps_transform.py:124-134): the thin-plate spline
    through dst (+ corners) -> src (+ corners).  dst [B, k, 2], src [k, 2] or [B, k, 2]; returns float64 [B, 2, K + 3], K = k + 4: per output
    axis the K kernel weights, then (a1, ax, ay) — pinv(L) [src; 0] with L built from the dst points.  Host-side, B systems of K + 3 unknowns."""
    P = tps_control_points(dst, width)
    B, K, _ = P.shape
    src = torch.as_tensor(src, dtype=torch.float64)
    if src.dim() == 2:
        src = src.expand(B, *src.shape)
    r = (P[:, :, None, :] - P[:, None, :, :]).pow(2).sum(-1).sqrt()
    small = r < 1e-100
    U = torch.where(small, torch.zeros_like(r), r * r * torch.log(torch.where(small, torch.ones_like(r), r)))
    L = torch.zeros(B, K + 3, K + 3, dtype=torch.float64)
    L[:, :K, :K] = U
    L[:, :K, K] = 1.0
    L[:, :K, K + 1:] = P
    L[:, K, :K] = 1.0
    L[:, K + 1:, :K] = P.transpose(1, 2)
    V = torch.zeros(B, K + 3, 2, dtype=torch.float64)
    V[:, :K] = tps_control_points(src, width)
    return (torch.linalg.pinv(L) @ V).transpose(1, 2).contiguous()


@dataclass
class AugmentParams:
    """What DeviceAugment.sample draws, all on the host: tps / flip / fallback bool [B], dst float64 [B, k, 2] (displaced control points), src
    float64 [k, 2], box int32 [B, 4] rows (i, j, h, w).  fallback marks the boxes that come from the centre-crop rule."""
    tps: torch.Tensor
    dst: torch.Tensor
    src: torch.Tensor
    box: torch.Tensor
    flip: torch.Tensor
    fallback: torch.Tensor


class DeviceAugment:
    def __init__(self, size=224, tps_prob=0.2, tps_scale=0.1, scale=(0.8, 1.0), ratio=(0.9, 1.1), hflip=0.5, generator: Optional[torch.Generator] = None):
        if size < 1 or not 0.0 <= tps_prob <= 1.0 or not 0.0 <= hflip <= 1.0:
            raise ValueError("DeviceAugment: size >= 1, probabilities in [0, 1]")
        if not (0.0 < scale[0] <= scale[1]) or not (0.0 < ratio[0] <= ratio[1]):
            raise ValueError("DeviceAugment: scale and ratio are (min, max) ranges of positive numbers")
        self.size, self.tps_prob, self.tps_scale, self.scale, self.ratio, self.hflip = int(size), float(tps_prob), float(tps_scale), tuple(scale), tuple(ratio), float(hflip)
        self.generator = generator
        self._ws = None  # stage 1's output, reused from call to call

    # -- parameters -------------------------------------------------------------------------------------------------------------------
    def _rand(self, *shape):
        return torch.rand(*shape, dtype=torch.float64, generator=self.generator)

    def sample(self, B: int, H: int, W: int) -> AugmentParams:
        """Draws the parameters of one batch.  Crop boxes follow torchvision's RandomResizedCrop.get_params: up to 10 tries of area U(scale),
        aspect exp(U(log ratio)), w = round(sqrt(A r)), h = round(sqrt(A / r)), the first that fits wins and is placed uniformly; a sample with no
        fitting try gets the centre crop with the aspect clamped into `ratio`."""
        tps = self._rand(B) < self.tps_prob
        src = regular_grid(W)
        dst = src + (2.0 * self._rand(B, src.shape[0], 2) - 1.0) * (self.tps_scale * W)
        area = float(H * W) * (self.scale[0] + (self.scale[1] - self.scale[0]) * self._rand(B, 10))
        lr0, lr1 = math.log(self.ratio[0]), math.log(self.ratio[1])
        aspect = torch.exp(lr0 + (lr1 - lr0) * self._rand(B, 10))
        w = torch.round(torch.sqrt(area * aspect)).long()
        h = torch.round(torch.sqrt(area / aspect)).long()
        fits = (w > 0) & (w <= W) & (h > 0) & (h <= H)
        fallback = ~fits.any(dim=1)
        first = fits.float().argmax(dim=1, keepdim=True)
        w, h = w.gather(1, first)[:, 0], h.gather(1, first)[:, 0]
        i = torch.floor(self._rand(B) * (H - h + 1).clamp(min=1)).long()  # randint(0, H - h + 1); the clamp only serves rows the fallback replaces
        j = torch.floor(self._rand(B) * (W - w + 1).clamp(min=1)).long()
        in_ratio = W / H
        if in_ratio < self.ratio[0]:
            fw, fh = W, int(round(W / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            fh, fw = H, int(round(H * self.ratio[1]))
        else:
            fw, fh = W, H
        fb = torch.tensor([(H - fh) // 2, (W - fw) // 2, fh, fw])
        box = torch.where(fallback[:, None], fb[None, :], torch.stack([i, j, h, w], dim=1)).to(torch.int32)
        flip = self._rand(B) < self.hflip
        return AugmentParams(tps=tps, dst=dst, src=src, box=box, flip=flip, fallback=fallback)

    # -- the two launches -------------------------------------------------------------------------------------------------------------
    def apply(self, x: torch.Tensor, params: AugmentParams) -> torch.Tensor:
        """x [B, C, W, W] uint8 / float32 on the GPU -> float32 [B, C, size, size] in x's units."""
        B, C, H, W = hip._images(x, "DeviceAugment.apply: x")
        if H != W:
            raise ValueError(f"DeviceAugment.apply: square images only, got {H} x {W}")
        if not hip.TPS_MIN_W <= W <= hip.TPS_MAX_W:
            raise ValueError(f"DeviceAugment.apply: {hip.TPS_MIN_W} <= W <= {hip.TPS_MAX_W}, got {W}")
        if params.tps.shape != (B,) or params.flip.shape != (B,) or params.box.shape != (B, 4) or params.dst.dim() != 3 or params.dst.shape[0] != B:
            raise ValueError("DeviceAugment.apply: the parameters were drawn for another batch size")
        hip.check_crop_boxes(params.box, H, W, self.size)
        if not x.is_cuda:
            raise RuntimeError("DeviceAugment.apply: expected a GPU tensor (the HIP path has no CPU fallback)")
        dev = x.device
        x = x.contiguous()
        K = params.dst.shape[1] + 4
        tps = params.tps.bool()
        any_tps = bool(tps.any())
        # one upload of the float64 tables, one of the int32 ones
        f64 = torch.zeros(B * K * 2 + B * 2 * (K + 3), dtype=torch.float64)
        if any_tps:
            f64[:B * K * 2] = tps_control_points(params.dst, W).reshape(-1)
            coef = f64[B * K * 2:].view(B, 2, K + 3)
            coef[tps] = tps_coefficients(params.dst[tps], params.src, W)
        i32 = torch.cat([tps.to(torch.int32), params.flip.to(torch.int32), params.box.reshape(-1).to(torch.int32)])
        f64, i32 = f64.to(dev, non_blocking=True), i32.to(dev, non_blocking=True)
        ws = self._workspace(x)
        if any_tps:
            hip.tps_warp(x, f64[:B * K * 2].view(B, K, 2), f64[B * K * 2:].view(B, 2, K + 3), i32[:B], ws)
        out = torch.empty(B, C, self.size, self.size, dtype=torch.float32, device=dev)
        hip.crop_resize_flip(x, ws, i32[:B], i32[2 * B:].view(B, 4), i32[B:2 * B], out)
        return out

    def _workspace(self, x):
        n = x.numel()
        if self._ws is None or self._ws.device != x.device or self._ws.numel() < n:
            self._ws = torch.empty(n, dtype=torch.float32, device=x.device)
        return self._ws[:n].view(x.shape)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return self.apply(x, self.sample(x.shape[0], x.shape[2], x.shape[3]))

    def eval_transform(self, x: torch.Tensor) -> torch.Tensor:
        """The reference's eval transform for square images — Resize(size, antialias=True) + CenterCrop(size) — through the stage-2 kernel:
        the whole image resized to size x size, no warp, no flip."""
        B, C, H, W = hip._images(x, "DeviceAugment.eval_transform: x")
        if H != W:
            raise ValueError(f"DeviceAugment.eval_transform: square images only, got {H} x {W}")
        box = torch.tensor([[0, 0, H, W]], dtype=torch.int32).repeat(B, 1)
        hip.check_crop_boxes(box, H, W, self.size)
        if not x.is_cuda:
            raise RuntimeError("DeviceAugment.eval_transform: expected a GPU tensor (the HIP path has no CPU fallback)")
        out = torch.empty(B, C, self.size, self.size, dtype=torch.float32, device=x.device)
        zeros = torch.zeros(B, dtype=torch.int32, device=x.device)
        hip.crop_resize_flip(x.contiguous(), None, None, box.to(x.device), zeros, out)
        return out
