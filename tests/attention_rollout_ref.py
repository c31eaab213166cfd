"""Attention rollout in float64: the expected values of the get_attention_rollout tests (test_attention_rollout_cpu.py checks it on closed
forms, test_attention_rollout_gpu.py compares the kernel and the model against it, golden/make_golden_rollout.py rolls the reference's maps
with it)."""
import torch


def rollout(maps, start_layer=0, residual=0.5, start=None):
    """maps: one [B, H, N, N] attention map per block, block 0 first.  Returns float64 [B, N]:
        r = start^T . A~_{L-1} . A~_{L-2} ... A~_{start_layer},   A~_l = residual I + (1 - residual) mean_h maps[l]
    the LAST block applied first.  start: [B, N] (default: one-hot at token 0, CLS); start_layer < 0 counts from the end."""
    L = len(maps)
    B, _, N, _ = maps[0].shape
    if start is None:
        r = torch.zeros(B, N, dtype=torch.float64, device=maps[0].device)
        r[:, 0] = 1.0
    else:
        r = start.double().to(maps[0].device)
    for l in range(L - 1, start_layer % L - 1, -1):
        A = maps[l].double().mean(1)
        r = residual * r + (1.0 - residual) * torch.einsum("bq,bqk->bk", r, A)
    return r


def tv(a, b):
    """Mean over the batch of the total variation 1/2 sum_k |a - b| between the rows of two [B, N] tensors."""
    return 0.5 * (a.double() - b.double().to(a.device)).abs().sum(-1).mean().item()
