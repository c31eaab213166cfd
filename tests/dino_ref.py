"""The oracle of the DINO loss tests: the PAIRWISE definition of the multi-crop loss (Caron et al. 2021, Algorithm 1 and its multi-crop extension),
in torch with autograd, in float64 or float32; and the closed form the kernels compute, restated in torch.  Written from the paper.

    S [V, B, K] student logits, views 0 and 1 the global crops;  T [2, B, K] teacher logits of the global crops;  c [K] centre
    q_i = softmax((T_i - c) / tt),  log p_v = log_softmax(S_v / ts)
    loss = 1 / (2 V - 2) * sum_{i < 2} sum_{v != i} mean_b sum_k -q_i[b,k] log p_v[b,k]
"""
import torch


def pairwise(S, T, c, ts, tt, dtype=torch.float64):
    """-> (loss, dS): the loop over the teacher view iq and the student views v != iq, and autograd's gradient.  dtype: what everything is
    computed in (float64: the reference; float32: the plain restatement whose error sets the tests' bound)."""
    S = S.detach().cpu().to(dtype).requires_grad_(True)
    T, c = T.detach().cpu().to(dtype), c.detach().cpu().to(dtype)
    V = S.shape[0]
    q = torch.softmax((T - c) / tt, dim=-1)
    logp = torch.log_softmax(S / ts, dim=-1)
    total, terms = 0, 0
    for iq in range(2):
        for v in range(V):
            if v == iq:
                continue
            total = total + torch.sum(-q[iq] * logp[v], dim=-1).mean()
            terms += 1
    loss = total / terms
    loss.backward()
    return loss.detach(), S.grad


def closed_form(S, T, c, ts, tt, dtype=torch.float64):
    """-> (loss, dS) of the closed form: with n = 2 V - 2, m_v = 1 for v < 2 else 2, Q_v = sum_{i != v} q_i,
    loss = 1 / (n B) sum_v sum_b [m_v lse(S_v[b] / ts) - <Q_v[b], S_v[b]> / ts],  dS_v = (m_v p_v - Q_v) / (n B ts).  No autograd."""
    S, T, c = (t.detach().cpu().to(dtype) for t in (S, T, c))
    V, B, _ = S.shape
    n = 2 * V - 2
    q = torch.softmax((T - c) / tt, dim=-1)
    p = torch.softmax(S / ts, dim=-1)
    lse = torch.logsumexp(S / ts, dim=-1)
    loss, dS = 0, torch.empty_like(S)
    for v in range(V):
        m = 1 if v < 2 else 2
        Q = sum(q[i] for i in range(2) if i != v)
        loss = loss + (m * lse[v] - (Q * S[v]).sum(-1) / ts).sum()
        dS[v] = (m * p[v] - Q) / (n * B * ts)
    return loss / (n * B), dS


def peaks(V, B, K, cols):
    """The fixed rule of the one-hot case: the peak column of teacher row (i, b) and of student row (v, b), drawn from `cols` (a list of columns:
    0, K - 1 and the plan's seams) so that some teacher and student peaks coincide and some do not, and the two teachers of a batch row differ
    whenever cols has two entries.  -> (teacher peaks [2, B], student peaks [V, B]) as int64 tensors."""
    n = len(cols)
    tp = torch.tensor([[cols[(b + i) % n] for b in range(B)] for i in range(2)], dtype=torch.int64)
    sp = torch.tensor([[cols[(b + (v * v + v) // 2) % n] for b in range(B)] for v in range(V)], dtype=torch.int64)
    return tp, sp


def one_hot_logits(pk, K, value=64.0):
    """rows with `value` at the peak column and 0 elsewhere: [..., K] float32"""
    out = torch.zeros(*pk.shape, K, dtype=torch.float32)
    out.scatter_(-1, pk.unsqueeze(-1), value)
    return out


def one_hot_grad(tp, sp, K, ts):
    """dS of the one-hot case, predicted per element from the peak positions with both softmaxes exactly one-hot: (m_v [k == sp] - sum_{i != v}
    [k == tp_i]) / (n B ts), in float32 (exact when n B ts is a power of two)."""
    V, B = sp.shape
    n = 2 * V - 2
    d = torch.zeros(V, B, K, dtype=torch.float32)
    for v in range(V):
        d[v].scatter_add_(-1, sp[v].unsqueeze(-1), torch.full((B, 1), 1.0 if v < 2 else 2.0))
        for i in range(2):
            if i != v:
                d[v].scatter_add_(-1, tp[i].unsqueeze(-1), torch.full((B, 1), -1.0))
    return d / (n * B * ts)
