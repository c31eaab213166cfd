"""The oracle of the iBOT patch-loss tests: the row-paired definition of masked patch-token distillation (Zhou et al. 2022, eq. 3, with DINO's
centring of the teacher), in torch with autograd, in float64 or float32; and the helpers of the exact one-hot case.  Written from the paper.

    S [R, K] student logits, T [R, K] teacher logits (row r of both the same masked token), c [K] centre, w [R] row weights
    q_r = softmax((T_r - c) / tt),  log p_r = log_softmax(S_r / ts)
    loss = sum_r w_r sum_k -q_r[k] log p_r[k]
"""
import torch


def paired(S, T, c, w, ts, tt, dtype=torch.float64, g=1.0):
    """-> (loss, dS): the definition and autograd's gradient of g * loss.  dtype: what everything is computed in (float64: the reference; float32:
    the plain restatement whose error sets the tests' bound)."""
    S = S.detach().cpu().to(dtype).requires_grad_(True)
    T, c, w = (t.detach().cpu().to(dtype) for t in (T, c, w))
    q = torch.softmax((T - c) / tt, dim=-1)
    logp = torch.log_softmax(S / ts, dim=-1)
    loss = (w * torch.sum(-q * logp, dim=-1)).sum()
    (g * loss).backward()
    return loss.detach(), S.grad


def closed_form(S, T, c, w, ts, tt, dtype=torch.float64):
    """-> (loss, dS) of the closed form the kernels compute: loss = sum_r w_r (lse(S_r / ts) - <q_r, S_r> / ts), dS = w_r (p_r - q_r) / ts.  No
    autograd."""
    S, T, c, w = (t.detach().cpu().to(dtype) for t in (S, T, c, w))
    q = torch.softmax((T - c) / tt, dim=-1)
    p = torch.softmax(S / ts, dim=-1)
    loss = (w * (torch.logsumexp(S / ts, dim=-1) - (q * S).sum(-1) / ts)).sum()
    return loss, w[:, None] * (p - q) / ts


def peaks(R, K, cols):
    """The fixed rule of the one-hot case: the peak column of teacher row r and of student row r, drawn from `cols` (0, K - 1 and the plan's seams)
    so that some rows' peaks coincide and some do not.  -> (teacher peaks [R], student peaks [R]) as int64 tensors."""
    n = len(cols)
    tp = torch.tensor([cols[r % n] for r in range(R)], dtype=torch.int64)
    sp = torch.tensor([cols[(r + (r // n) % 2 + (r % 3 == 0)) % n] for r in range(R)], dtype=torch.int64)
    return tp, sp


def one_hot_logits(pk, K, value=64.0):
    """rows with `value` at the peak column and 0 elsewhere: [R, K] float32"""
    out = torch.zeros(pk.shape[0], K, dtype=torch.float32)
    out.scatter_(-1, pk.unsqueeze(-1), value)
    return out


def one_hot_grad(tp, sp, w, K, ts, g=1.0):
    """dS of the one-hot case, predicted per element from the peak positions with both softmaxes exactly one-hot: g w_r ([k == sp_r] - [k == tp_r])
    / ts, in float32 (exact when g, w_r and ts are powers of two)."""
    R = sp.shape[0]
    d = torch.zeros(R, K, dtype=torch.float32)
    d.scatter_add_(-1, sp.unsqueeze(-1), torch.ones(R, 1))
    d.scatter_add_(-1, tp.unsqueeze(-1), -torch.ones(R, 1))
    return d * (g * w.float()[:, None] / ts)
