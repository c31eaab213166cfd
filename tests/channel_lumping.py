"""The float64 reference of get_channel_attention shared by its CPU and GPU tests: an attention map lumped to channel granularity by one-hot
matmuls.  Token 0 is CLS (segment 0), token 1 + c * n_p + i is patch i of channel c (segment 1 + c)."""
import torch


def segment_onehot(C, n_p, shift=0, device="cpu"):
    """[N, 1 + C] float64, row k = the one-hot segment of token k.  shift != 0 (the discrimination checks): the boundaries moved by `shift`
    tokens — token k takes the segment of token (k + shift) mod N."""
    N = 1 + C * n_p
    k = (torch.arange(N, device=device) + shift) % N
    seg = torch.where(k == 0, torch.zeros_like(k), 1 + (k - 1).clamp_min(0) // n_p)
    return torch.nn.functional.one_hot(seg, 1 + C).to(torch.float64)


def lump(P, C, n_p, shift=0):
    """P [..., N, N] -> (T [..., N, 1 + C], A [..., 1 + C, 1 + C]) in float64: T = the mass each query puts on each segment, A = its mean over
    the queries of each segment."""
    E = segment_onehot(C, n_p, shift, P.device)
    T = P.double() @ E
    A = (E / E.sum(0, keepdim=True)).transpose(0, 1) @ T
    return T, A


def mean_tv(A, B):
    """mean over rows of the total variation 1/2 sum_j |A - B|"""
    return 0.5 * (A.double() - B.double()).abs().sum(-1).mean().item()
