"""Gradient-weighted attention relevance (Chefer, Gur & Wolf 2021) in float64: the expected values of the get_attention_relevance tests
(test_attention_relevance_cpu.py checks it on closed forms and against the explicit R matrix, test_attention_relevance_gpu.py compares the
kernel and the model against it, golden/make_golden_relevance.py applies it to the reference's maps and their gradients)."""
import torch


def relevance(maps, grads, start_layer=0, start=None):
    """maps, grads: one [B, H, N, N] attention map per block and the gradient of the explained scalar with respect to it, block 0 first.
    Returns float64 [B, N]:
        r = start^T (I + A^_{L-1}) (I + A^_{L-2}) ... (I + A^_{start_layer}),   A^_l = mean_h relu(grads[l] . maps[l])
    the LAST block applied first — row `start` of R after R = I; R <- R + A^_l R for l = start_layer .. L - 1.  start: [B, N] (default: one-hot
    at token 0, CLS); start_layer < 0 counts from the end."""
    L = len(maps)
    B, _, N, _ = maps[0].shape
    if start is None:
        r = torch.zeros(B, N, dtype=torch.float64, device=maps[0].device)
        r[:, 0] = 1.0
    else:
        r = start.double().to(maps[0].device)
    for l in range(L - 1, start_layer % L - 1, -1):
        A = (grads[l].double() * maps[l].double()).clamp(min=0).mean(1)
        r = r + torch.einsum("bq,bqk->bk", r, A)
    return r


def relevance_step_ref(q, k, v, dO, w, nq, scale, magnitude=False):
    """One block from its operands, as dcv_attn_relevance_step states it: q, k, v, dO [B, H, N, 64] (the bf16 values, any float dtype),
    w [B, N] >= 0, query rows [0, nq).  Float64 [B, N]:
        out[b,k] = w[b,k] + 1 / H sum_h sum_{q < nq} w[b,q] P[b,h,q,k] max(G[b,h,q,k], 0),   P = softmax(q k^T scale),   G = dO v^T
    Rows of dO at or past nq, and rows whose weight is 0, are not read (they may hold NaN).  magnitude=True: also the companion
    mag[b,k] = w[b,k] + 1 / H sum sum w p sum_d |dO_qd v_kd|, which bounds every partial sum on either side of the relu's kink."""
    q, k, v, w = q.double(), k.double(), v.double(), w.double()
    H = q.shape[1]
    wq = w[:, :nq]
    live = (wq > 0)[:, None, :, None]
    g = torch.where(live, dO.double()[:, :, :nq], torch.zeros((), dtype=torch.float64, device=q.device))
    P = torch.softmax(q[:, :, :nq] @ k.transpose(-1, -2) * scale, dim=-1)
    G = g @ v.transpose(-1, -2)
    out = w + torch.einsum("bq,bhqk->bk", wq, P * G.clamp(min=0)) / H
    if not magnitude:
        return out
    return out, w + torch.einsum("bq,bhqk->bk", wq, P * (g.abs() @ v.abs().transpose(-1, -2))) / H


def normalised_patches(r):
    """r[:, 1:] / sum: the patch relevance as a distribution (float64)."""
    p = r.double()[:, 1:]
    return p / p.sum(-1, keepdim=True)


def tv(a, b):
    """Mean over the batch of the total variation 1/2 sum_k |a - b| between the rows of two [B, N] tensors."""
    return 0.5 * (a.double() - b.double().to(a.device)).abs().sum(-1).mean().item()
