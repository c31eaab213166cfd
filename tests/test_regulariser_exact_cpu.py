"""The two regularisers of the train step on operands for which "bit for bit" is legitimate: the channel-diversity loss (ortho_fwd_partial, ortho_fwd_final,
ortho_bwd_kernel in csrc/tokenizer.hip) and the channel-proxy loss (proxy_loss_kernel in csrc/loss.hip).  This file holds what tests/test_regulariser_exact_gpu.py
shares with it and proves, without a GPU, that the comparison is sound:

* Dyadic ortho operands (ortho_operands): row t of Y holds k_t non-zero entries of +-m_t with (k_t, m_t) from ROW_KINDS, so |y_t| is 4, 2, 8 or 8, 1 / |y_t| is
  0.25, 0.5 or 0.125, every normalised entry is +-0.25 or +-0.5 and every normalised row has square norm exactly 1.  The norms differ from row to row (an inv_norm
  read from the wrong row changes bits) and coef differs from image to image (so does a row of another image).  One case has whole rows equal to 0: they are
  clamped (inv_norm = 1 / 1e-12f = 1e12f), add 0 to selfsq and have fh = 0.
* The closed-form expectation in float64 (ortho_expect) for S, selfsq, tot, inv_norm, (pos_sum, neg_sum) and dY.
* The two conditions under which torch.equal is the right assertion, asserted per case: (i) the float64 expectation is an fp32 number (the dY of a zero row
  is base * 1e12f rounded ONCE: one fp32 multiplication, which no order can change); (ii) an fp32 restatement of the kernels' formulas (ortho_restate) gives those
  bits in two association orders, with and without fused multiply-add: every intermediate is then representable, and neither the device's summation order nor
  -ffp-contract can matter.  For the non-negative sums this needs 64 max(sum S^2, sum tot^2) < 2^24, asserted; random signs keep the sums that small.
* Injected defects (DEFECTS): each is applied to the restatement and must be flagged by the exact rules; each is also evaluated on test_ortho_loss's own operands
  at that test's bounds, and OLD_BOUNDS_CATCH records, shape by shape, which of them those bounds catch.
* Two defects of the issue's list cannot change a bit on finite operands, which the tests below state instead of hiding: with C == 1, tot is bitwise S, so
  cb * (tot - s_c) is cb * 0 whatever cb holds (the guard matters for a non-finite coef only, which is how it is tested); and a row that is exactly 0 has
  fh = 0, so g . fh is 0 whether the clamp branch is taken or not (the branch is visible on a row of norm 3e-13, held against float64 autograd).
* Proxy operands, the float64 reference (models/loss_fn.py:7-21 under autograd, as in test_proxy_loss_kernel) and an fp32 restatement of proxy_loss_kernel,
  from which the GPU file takes its measured bound for saturated logits."""
import math
import os
import sys
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ORTHO_CHUNK = 28   # csrc/tokenizer.hip: tokens per workgroup, 4 waves x 7
ORTHO_MAX_D = 1024  # OV = 4 float4 per lane
ROW_KINDS = ((16, 1.0), (4, 1.0), (16, 2.0), (4, 4.0))  # (non-zero entries, magnitude): norms 4, 2, 8, 8
INV_CLAMP = float(np.float32(1.0) / np.float32(1e-12))  # what 1.f / fmaxf(0.f, 1e-12f) is in fp32
COEF_VALUES = (0.0, 1.0, -1.0, 0.5, -0.5, 0.25, -0.25, 0.125, -0.125)

OrthoCase = namedtuple("OrthoCase", "B C n D zero_rows covers")
ORTHO_CASES = [
    OrthoCase(2, 3, 1, 16, False, "n == 1: no same-channel pair"),
    OrthoCase(2, 1, 29, 4, False, "C == 1; nv = 1; a 28 + 1 split of ORTHO_CHUNK"),
    OrthoCase(2, 3, 27, 192, False, "nv = 48 < 64 lanes; n below a chunk and not a multiple of 4"),
    OrthoCase(3, 5, 30, 384, True, "second chunk with two idle waves; whole rows equal to 0"),
    OrthoCase(1, 18, 3, 768, False, "wave 3 idle"),
    OrthoCase(1, 2, 57, 1024, False, "OV limit"),
    OrthoCase(2, 8, 196, 384, False, "the workload's n, seven full chunks"),
]
ORTHO_IDS = [f"B{c.B}-C{c.C}-n{c.n}-D{c.D}" for c in ORTHO_CASES]


def ortho_regimes(c):
    """What a case exercises, from the launch code: grid (cdiv(n, 28), B C); wave w of chunk k takes tokens 28 k + w, + 4, ...; lane l holds float4 l + 64 i."""
    chunks = -(-c.n // ORTHO_CHUNK)
    last = c.n - (chunks - 1) * ORTHO_CHUNK
    return dict(n1=c.n == 1, c1=c.C == 1, nv=c.D // 4, chunks=chunks, last=last, idle_waves=max(0, 4 - last), full_chunks=c.n // ORTHO_CHUNK,
                zero_rows=c.zero_rows, n_mod4=c.n % 4)


# ---- dyadic ortho operands ----------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def ortho_operands(case):
    """Y fp32 [B, C n, D], coef fp32 [B, 2], kind int64 [B, C n] (index into ROW_KINDS, -1 for a zero row).  CPU tensors; treat as read-only."""
    B, C, n, D = case[:4]
    g = torch.Generator().manual_seed(20240 + 97 * ORTHO_CASES.index(case))
    R = B * C * n
    allowed = torch.tensor([0, 1, 2, 3] if D >= 16 else [1, 3])
    kind = allowed[torch.randint(0, allowed.numel(), (R,), generator=g)].tolist()
    inv_of = [0.25, 0.5, 0.125, 0.125]
    for r in range(1, R):  # no row has its neighbour's norm
        while inv_of[kind[r]] == inv_of[kind[r - 1]]:
            kind[r] = int(allowed[(allowed.tolist().index(kind[r]) + 1) % allowed.numel()])
    kind = torch.tensor(kind)
    kmax = 16 if D >= 16 else 4
    pos = torch.rand(R, D, generator=g).argsort(-1)[:, :kmax]  # kmax distinct columns per row
    k = torch.tensor([ROW_KINDS[i][0] for i in range(4)])[kind]
    m = torch.tensor([ROW_KINDS[i][1] for i in range(4)])[kind]
    sgn = torch.randint(0, 2, (R, kmax), generator=g).float() * 2 - 1
    val = sgn * m[:, None] * (torch.arange(kmax)[None, :] < k[:, None])
    Y = torch.zeros(R, D).scatter_(1, pos, val)
    if case.zero_rows:
        zero = torch.rand(R, generator=g) < 0.08
        zero[0] = True                 # the first token of a channel
        zero[n - 1] = True             # the last token of a channel: the ragged chunk
        zero[R - n + ORTHO_CHUNK - 1] = True  # the last token of a full chunk
        Y[zero] = 0
        kind = torch.where(zero, torch.tensor(-1), kind)
    coef = torch.stack([torch.tensor(COEF_VALUES)[torch.randperm(len(COEF_VALUES), generator=g)[:B]] for _ in range(2)], 1)  # pairwise different over b
    return Y.reshape(B, C * n, D), coef, kind.reshape(B, C * n)


def ortho_expect(Y, coef, case):
    """The closed form in float64: dict of S [B,C,D], selfsq [B,C], tot [B,D], inv_norm [B,Cn], stats [B,2], dY [B,Cn,D] and zero [B,Cn] (bool)."""
    B, C, n, D = case[:4]
    Y4 = Y.double().reshape(B, C, n, D)
    q = (Y4 * Y4).sum(-1)
    zero = q == 0
    inv = torch.where(zero, torch.tensor(INV_CLAMP, dtype=torch.float64), 1.0 / q.clamp_min(1e-300).sqrt())
    fh = Y4 * inv[..., None]
    S = fh.sum(2)
    selfsq = (q * inv * inv).sum(2)
    tot = S.sum(1)
    a, t2, sf = (S * S).sum((1, 2)), (tot * tot).sum(1), selfsq.sum(1)
    pos = torch.zeros_like(a) if n == 1 else a - sf
    neg = torch.zeros_like(a) if C == 1 else t2 - a
    ca = (2 * coef[:, 0].double())[:, None, None]
    cb = (2 * coef[:, 1].double() * (0.0 if C == 1 else 1.0))[:, None, None]
    base = ca * S + cb * (tot[:, None, :] - S)
    g = base[:, :, None, :] - ca[..., None] * fh
    dot = torch.where(zero, torch.zeros_like(q), (g * fh).sum(-1))
    dY = (g - fh * dot[..., None]) * inv[..., None]
    dY = torch.where(zero[..., None], dY.float().double(), dY)  # a zero row: base * 1e12f, one fp32 multiplication
    return dict(S=S, selfsq=selfsq, tot=tot, inv_norm=inv.reshape(B, C * n), stats=torch.stack([pos, neg], 1), dY=dY.reshape(B, C * n, D),
                zero=zero.reshape(B, C * n), sums=(float(a.max()), float(t2.max())))


# ---- fp32 restatement of the three kernels ------------------------------------------------------------------------------------------------------------------
def _mac(acc, a, b, fma):
    """acc + a * b in fp32: the product rounded and then added, or (fma) formed exactly in float64 and the sum rounded once."""
    return (acc.double() + a.double() * b.double()).float() if fma else acc + a * b


def _sum_last(x, order):
    L = x.shape[-1]
    if order == "seq":
        acc = torch.zeros_like(x[..., 0])
        for i in range(L):
            acc = acc + x[..., i]
        return acc
    P = 1 << max(0, (L - 1).bit_length())
    x = F.pad(x, (0, P - L))
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def _dot_last(a, b, order, fma):
    """sum over the last axis of a * b in fp32.  order 'seq': one accumulator from the first element on; 'tree': halving, from the far ends inwards."""
    a, b = torch.broadcast_tensors(a, b)
    if order == "seq":
        acc = torch.zeros_like(a[..., 0])
        for i in range(a.shape[-1]):
            acc = _mac(acc, a[..., i], b[..., i], fma)
        return acc
    if fma and a.shape[-1] >= 2:
        L = a.shape[-1] // 2 * 2
        pairs = _mac(a[..., 1:L:2] * b[..., 1:L:2], a[..., 0:L:2], b[..., 0:L:2], True)
        return _sum_last(torch.cat([pairs, (a[..., L:] * b[..., L:])], -1), order)
    return _sum_last(a * b, order)


DEFECTS = ("ssq_drop", "dot_drop_col", "inv_neighbour", "coef_prev_image", "tot_prev_image", "cb_at_c1", "clamp_projected")


def ortho_restate(Y, coef, case, order="seq", fma=False, defect=None):
    """ortho_fwd_partial + ortho_fwd_final + ortho_bwd_kernel in fp32 torch, term for term.  defect: one of DEFECTS (None: the kernels as written)."""
    B, C, n, D = case[:4]
    Y4 = Y.float().reshape(B, C, n, D)
    q = _dot_last(Y4, Y4, order, fma)
    inv = 1.0 / torch.maximum(q.sqrt(), torch.tensor(1e-12, dtype=torch.float32))
    selfsq = _sum_last(q * inv * inv, order)
    S = _dot_last(Y4.transpose(2, 3), inv[:, :, None, :], order, fma)
    cs = range(C) if order == "seq" else range(C - 1, -1, -1)
    tot, ssq_d = torch.zeros(B, D), torch.zeros(B, D)
    drop = None
    if defect == "ssq_drop":
        i = int((S[0] != 0).flatten().nonzero()[0])  # the first element of image 0 that has something to lose
        drop = (i // D, i % D)
    for c in cs:
        s = S[:, c]
        add = _mac(ssq_d, s, s, fma)
        if drop is not None and c == drop[0]:
            add[0, drop[1]] = ssq_d[0, drop[1]]
        ssq_d = add
        tot = tot + s
    a, t2, sf = _sum_last(ssq_d, order), _dot_last(tot, tot, order, fma), _sum_last(selfsq, order)
    pos = torch.zeros(B) if n == 1 else a - sf
    neg = torch.zeros(B) if C == 1 else t2 - a
    # backward
    cf = coef.float().roll(1, 0) if defect == "coef_prev_image" else coef.float()
    tt = (tot.roll(1, 0) if defect == "tot_prev_image" else tot)[:, None, :]
    ca = (2 * cf[:, 0])[:, None, None]
    cb = (torch.zeros(B) if C == 1 and defect != "cb_at_c1" else 2 * cf[:, 1])[:, None, None]
    base = _mac(ca * S, cb.expand_as(S), tt - S, fma)
    binv = inv.reshape(-1).roll(1).reshape(B, C, n) if defect == "inv_neighbour" else inv
    clamped = binv >= torch.tensor(1e12, dtype=torch.float32)
    fh = Y4 * binv[..., None]
    g = _mac(base[:, :, None, :].expand_as(fh), (-ca[..., None]).expand_as(fh), fh, fma)
    gd, fd = g, fh
    if defect == "dot_drop_col":
        col = int((Y4 != 0).sum((0, 1, 2)).argmax())  # the column most rows use
        keep = torch.arange(D) != col
        gd, fd = g[..., keep], fh[..., keep]
    dot = _dot_last(gd, fd, order, fma)
    if defect != "clamp_projected":
        dot = torch.where(clamped, torch.zeros_like(dot), dot)
    dY = _mac(g, -fh, dot[..., None].expand_as(fh), fma) * binv[..., None]
    return dict(S=S, selfsq=selfsq, tot=tot, inv_norm=inv.reshape(B, C * n), stats=torch.stack([pos, neg], 1), dY=dY.reshape(B, C * n, D))


# ---- the exact rules ----------------------------------------------------------------------------------------------------------------------------------------
ORTHO_OUTPUTS = ("inv_norm", "S", "selfsq", "tot", "stats", "dY")


def _candidates(diff, terms, name_of):
    """terms whose single value explains got - want: lost (term == -diff) or added twice (term == diff); in the manner of test_stream_kernels_gpu._explain_terms."""
    lost, twice = (terms == -diff).nonzero().flatten(), (terms == diff).nonzero().flatten()
    return (f"explained by ONE LOST term at {[name_of(int(i)) for i in lost[:4]]} ({lost.numel()} candidates) or ONE DOUBLED term at "
            f"{[name_of(int(i)) for i in twice[:4]]} ({twice.numel()} candidates)")


def ortho_mismatches(got, want, Y, case):
    """Rule (i) and the comparison itself.  got: fp32 CPU tensors by name; want: ortho_expect's float64.  Returns one line per output that differs, naming the
    image, channel, token and column of the first differing element and, for the sums, the terms whose loss or doubling would explain the difference."""
    B, C, n, D = case[:4]
    out = []
    fh = None
    for name in ORTHO_OUTPUTS:
        g, w64 = got[name].detach().cpu(), want[name]
        w = w64.float()
        assert torch.equal(w.double(), w64), f"{name}: the expectation itself is not an fp32 number (test bug)"
        assert g.dtype == torch.float32 and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
        if torch.equal(g, w):
            continue
        bad = (g != w) | g.isnan()
        i = int(bad.flatten().nonzero()[0])
        gv, wv = g.flatten()[i].item(), w.flatten()[i].item()
        if fh is None:
            fh = Y.double().reshape(B, C, n, D) * want["inv_norm"].reshape(B, C, n, 1)
        if name == "inv_norm":
            where = f"image {i // (C * n)} channel {i % (C * n) // n} token {i % n}"
        elif name == "S":
            b, c, d = i // (C * D), i // D % C, i % D
            where = f"image {b} channel {c} column {d}; " + _candidates(gv - wv, fh[b, c, :, d], lambda t: f"token {t} (chunk {t // ORTHO_CHUNK}, wave {t % ORTHO_CHUNK % 4})")
        elif name == "selfsq":
            where = f"image {i // C} channel {i % C}"
        elif name == "tot":
            b, d = i // D, i % D
            where = f"image {b} column {d}; " + _candidates(gv - wv, want["S"][b, :, d], lambda c: f"channel {c}")
        elif name == "stats":
            b = i // 2
            sq = (want["S"][b] ** 2).flatten()
            where = (f"image {b} {'pos_sum' if i % 2 == 0 else 'neg_sum'}; in S^2 " + _candidates((gv - wv) * (1 if i % 2 == 0 else -1), sq, lambda j: f"(channel {j // D}, column {j % D})")
                     + "; in tot^2 " + _candidates(gv - wv, want["tot"][b] ** 2, lambda d: f"column {d}"))
        else:
            b, t, d = i // (C * n * D), i // D % (C * n), i % D
            where = f"image {b} channel {t // n} token {t % n} column {d}" + (" (a zero row: base * inv_norm)" if bool(want["zero"][b, t]) else "")
        out.append(f"{name}: {int(bad.sum())}/{bad.numel()} elements differ; first at {where}: got {gv!r}, want {wv!r}")
    return out


# ---- test_ortho_loss's own operands and bounds --------------------------------------------------------------------------------------------------------------
def old_ortho_cases():
    """The parametrisation of tests/test_kernels_gpu.py::test_ortho_loss, read from the test itself."""
    import test_kernels_gpu as old
    marks = [m for m in old.test_ortho_loss.pytestmark if m.name == "parametrize" and m.args[0] == "B,C,n,D"]
    assert len(marks) == 1
    return [tuple(c) for c in marks[0].args[1]]


def old_ortho_operands(B, C, n, D):
    """Y = _f(B, T, D, seed=3) + 0.3 and coef = _f(B, 2, seed=9) of test_ortho_loss (its generator is the CPU's)."""
    Y = torch.randn(B, C * n, D, generator=torch.Generator().manual_seed(3)) + 0.3
    coef = torch.randn(B, 2, generator=torch.Generator().manual_seed(9))
    return Y, coef


def ortho_reference64(Y, coef, C, n):
    """float64 autograd through F.normalize, as test_ortho_loss writes it: pos_sum, neg_sum [B] and dY."""
    B, T, D = Y.shape
    Yr = Y.double().detach().clone().requires_grad_(True)
    f = F.normalize(Yr, dim=-1).reshape(B, C, n, D)
    s = f.sum(2)
    pos_sum = ((s * s).sum(-1) - (f * f).sum(-1).sum(-1)).sum(-1)
    neg_sum = (s.sum(1) ** 2).sum(-1) - (s * s).sum(-1).sum(-1)
    loss = (coef[:, 0].double().to(Y.device) * pos_sum).sum() + ((coef[:, 1].double().to(Y.device) * neg_sum).sum() if C > 1 else 0)
    loss.backward()
    return pos_sum.detach(), neg_sum.detach(), Yr.grad


def _outside(got, ref64, rtol, atol):
    return bool((~((got.double() - ref64).abs() <= atol + rtol * ref64.abs())).any())


def old_bounds_findings(got, pos_sum, neg_sum, grad, C, rows=None):
    """The three assertions of test_ortho_loss on a result: names of those that fail.  rows: a boolean [B, T] mask to hold dY on those rows only, with
    their own max |grad| (the rows under the clamp are 1e12 times larger than the rest)."""
    bad = []
    if _outside(got["stats"][:, 0], pos_sum, 1e-4, 1e-3 * max(1.0, pos_sum.abs().max().item())):
        bad.append("pos_sum")
    if C > 1:
        if _outside(got["stats"][:, 1], neg_sum, 1e-4, 1e-3 * max(1.0, neg_sum.abs().max().item())):
            bad.append("neg_sum")
    elif not bool((got["stats"][:, 1] == 0).all()):
        bad.append("neg_sum")
    for tag, m in ((("dY", None),) if rows is None else (("dY clamped rows", rows), ("dY other rows", ~rows))):
        g, r = (got["dY"], grad) if m is None else (got["dY"][m], grad[m])
        if r.numel() and _outside(g, r, 1e-3, 1e-4 * r.abs().max().item() + 1e-6):
            bad.append(tag)
    return bad


def clamp_operands(device="cpu"):
    """randn + 0.3 at (2, 3, 30, 384) with a few rows scaled to norm 3e-13 and a few set to 0: Y, coef, the mask of the rows under the clamp."""
    B, C, n, D = 2, 3, 30, 384
    g = torch.Generator().manual_seed(77)
    Y = torch.randn(B, C * n, D, generator=g) + 0.3
    tiny = [(0, 0), (0, 29), (0, 58), (1, 31), (1, 89)]   # first token, last token of a chunk's tail, mid-channel, last row
    zero = [(0, 1), (0, 28), (1, 0), (1, 60)]
    for b, t in tiny:
        Y[b, t] *= 3e-13 / Y[b, t].double().norm().item()
    for b, t in zero:
        Y[b, t] = 0
    mask = torch.zeros(B, C * n, dtype=torch.bool)
    for b, t in tiny + zero:
        mask[b, t] = True
    coef = torch.randn(B, 2, generator=g)
    return (B, C, n, D), Y.to(device), coef.to(device), mask.to(device)


# ---- the proxy loss -----------------------------------------------------------------------------------------------------------------------------------------
PROXY_SHAPES = [(1, 1), (3, 4), (5, 100), (8, 1000), (16, 1024), (17, 60), (32, 512)]
PROXY_KINDS = ("random", "zero row", "parallel")
PROXY_STRUCTURED = ("p = e", "p = e[perm]", "e = -p")
PROXY_SCALE = float(np.sqrt(1.0 / 0.07))      # the workload's temperature, as in test_proxy_loss_kernel
PROXY_SCALE_SAT = float(np.sqrt(1.0 / 0.005))  # logits down to -4 / 0.005 = -800
PROXY_SAT_CASES = [(C, D, kind) for C, D in ((8, 384), (5, 100)) for kind in ("random", "parallel", "p = e[perm]", "e = -p")]
PROXY_SAT_FACTOR = 4.0


def _randn_cpu(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def proxy_operands(C, D, kind):
    """e, p fp32 [C, D] on the CPU: the three kinds of test_proxy_loss_kernel (same seeds and scales) and the three structured ones."""
    e, p = _randn_cpu(C, D, seed=3, scale=0.5), _randn_cpu(C, D, seed=4, scale=0.125)
    if kind == "zero row":
        e[0].zero_()
    elif kind == "parallel":
        p = (e * 0.3 + 1e-3 * _randn_cpu(C, D, seed=5)).contiguous()
    elif kind == "p = e":
        p = e.clone()
    elif kind == "p = e[perm]":
        p = e[proxy_perm(C)].contiguous()
    elif kind == "e = -p":
        e = -p
    else:
        assert kind == "random", kind
    return e, p


def proxy_perm(C):
    """a permutation without a fixed point (and not an involution for C > 2, so that L[i][j] and L[j][i] differ)"""
    return torch.arange(1, C + 1) % C


def proxy_reference(e, p, scale):
    """float64 autograd on the reference's formula (models/loss_fn.py:7-21): loss, d_emb, d_proxies."""
    C = e.shape[0]
    e64, p64 = e.double().detach().clone().requires_grad_(True), p.double().detach().clone().requires_grad_(True)
    a, b = scale * F.normalize(e64, p=2, dim=-1), scale * F.normalize(p64, p=2, dim=-1)
    ref = F.cross_entropy(-((a[:, None, :] - b[None, :, :]) ** 2).sum(-1), torch.eye(C, device=e.device, dtype=torch.float64))
    ref.backward()
    return ref.detach(), e64.grad, p64.grad


def proxy_restate(e, p, scale):
    """proxy_loss_kernel in fp32 torch, step for step (torch's own summation order, expf and logf): loss [1], d_emb, d_proxies."""
    C = e.shape[0]
    e, p, sc = e.float(), p.float(), torch.tensor(scale, dtype=torch.float32)
    eps = torch.tensor(1e-12, dtype=torch.float32)
    ne, npx = torch.maximum((e * e).sum(-1).sqrt(), eps), torch.maximum((p * p).sum(-1).sqrt(), eps)
    en, pn = e / ne[:, None], p / npx[:, None]
    diff = sc * en[:, None, :] - sc * pn[None, :, :]   # [i, j, d]
    L = -(diff * diff).sum(-1)
    m = L.max(-1, keepdim=True).values
    lse = m + (L - m).exp().sum(-1, keepdim=True).log()
    loss = (lse[:, 0] - L.diagonal()).sum() / C
    W = ((L - lse).exp() - torch.eye(C)) / C
    dn_e = sc * (W[:, :, None] * -2.0 * diff).sum(1)
    dn_p = sc * (W[:, :, None] * 2.0 * diff).sum(0)
    de = (dn_e - en * (en * dn_e).sum(-1, keepdim=True)) / ne[:, None]
    dp = (dn_p - pn * (pn * dn_p).sum(-1, keepdim=True)) / npx[:, None]
    return loss.reshape(1), de, dp


def proxy_errors(got, ref):
    """(loss, d_emb, d_proxies) errors as multiples of test_proxy_loss_kernel's bounds: |loss - ref| over 2e-6 max(1, |ref|), max |grad - ref| over
    2e-5 max |ref grad| + 1e-9.  At most 1 inside those bounds; a NaN stays a NaN."""
    loss, de, dp = got
    rl, rde, rdp = ref
    out = [abs(float(loss.double().reshape(-1)[0]) - float(rl)) / (2e-6 * max(1.0, abs(float(rl))))]
    for g, r in ((de, rde), (dp, rdp)):
        out.append(float((g.double().cpu() - r.cpu()).abs().max()) / (2e-5 * float(r.abs().max()) + 1e-9) if r.numel() else 0.0)
    return out


@lru_cache(maxsize=None)
def proxy_saturation_bound():
    """The worst error of the fp32 restatement against float64 over PROXY_SAT_CASES at PROXY_SCALE_SAT, per quantity, in proxy_errors' units (multiples of
    the bounds at the workload's scale)."""
    worst = [0.0, 0.0, 0.0]
    for C, D, kind in PROXY_SAT_CASES:
        e, p = proxy_operands(C, D, kind)
        err = proxy_errors(proxy_restate(e, p, PROXY_SCALE_SAT), proxy_reference(e, p, PROXY_SCALE_SAT))
        worst = [max(a, b) for a, b in zip(worst, err)]
    return tuple(worst)


def proxy_exact_operands(C=8, D=384):
    """Dyadic rows of norm 4 on pairwise disjoint supports (16 entries of +-1 each), e[0] = 0: with scale = 2 every logit of row 0 is exactly -4, its softmax is one
    number u for all classes, and d_emb[0][d] = 2 w_j s / 1e-12f for the one proxy j whose support holds d (s its sign there), exactly 0 where no proxy has an entry."""
    assert 2 * 16 * C <= D
    g = torch.Generator().manual_seed(5150)
    cols = torch.randperm(D, generator=g)[:32 * C].reshape(2, C, 16)
    e, p = torch.zeros(C, D), torch.zeros(C, D)
    e.scatter_(1, cols[0], torch.randint(0, 2, (C, 16), generator=g).float() * 2 - 1)
    p.scatter_(1, cols[1], torch.randint(0, 2, (C, 16), generator=g).float() * 2 - 1)
    e[0] = 0
    return e, p


def proxy_exact_findings(de0, p):
    """What is exact about d_emb[0] for proxy_exact_operands: see there.  The magnitudes are u / C / 1e-12f * 2 with u = expf(-logf(C)): lse = -4 + logf(C) rounds
    by half an ulp of 4 (1.2e-7 absolute), logf and expf by at most 2 ulps each (1.2e-7 absolute at 0.69 .. 2.1, 2.4e-7 relative), the two divisions by half an
    ulp each: below 8 ulps (9.6e-7 relative) of the float64 value for C <= 8."""
    C, D = p.shape
    de0 = de0.detach().cpu()
    out = []
    used = p != 0
    if not bool((de0[~used.any(0)] == 0).all()):
        out.append("a column in no proxy's support is not exactly 0")
    mags = []
    for j in range(C):
        v = de0[used[j]]
        s = torch.sign(p[j][used[j]]) * (-1.0 if j == 0 else 1.0)  # w_0 = (u - 1) / C < 0
        if not bool((v == v[0].abs() * s).all()):
            out.append(f"proxy {j}: its 16 columns do not hold one magnitude with the signs of the proxy's entries: {v.tolist()}")
        mags.append(float(v[0].abs()))
    if len(set(mags[1:])) > 1:
        out.append(f"the wrong classes 1.. do not share one magnitude: {mags[1:]}")
    u = 1.0 / C
    for j, want in ((0, 2 * (1 - u) / C / float(np.float32(1e-12))), (1, 2 * u / C / float(np.float32(1e-12)))):
        if j < C and not abs(mags[j] - want) <= 8 * 2.0 ** -23 * want:
            out.append(f"proxy {j}: magnitude {mags[j]!r}, want {want!r} within 8 ulps")
    return out


# =============================================================================================================================================================
# The CPU tests
# =============================================================================================================================================================
def test_case_table_covers_the_regimes():
    """Removing a row of ORTHO_CASES fails one of these."""
    r = [ortho_regimes(c) for c in ORTHO_CASES]
    assert any(x["n1"] for x in r), "n == 1"
    assert any(x["c1"] and x["nv"] == 1 and x["chunks"] == 2 and x["last"] == 1 for x in r), "C == 1, nv == 1, a 28 + 1 split"
    assert any(x["nv"] < 64 and x["nv"] > 1 and x["chunks"] == 1 and x["n_mod4"] != 0 and not x["n1"] for x in r), "nv below a wave, n below a chunk, n % 4 != 0"
    assert any(x["chunks"] == 2 and x["idle_waves"] == 2 for x in r), "a second chunk with two idle waves"
    assert any(x["chunks"] == 1 and x["idle_waves"] == 1 for x in r), "wave 3 idle"
    assert any(x["nv"] == ORTHO_MAX_D // 4 for x in r), "the OV limit"
    assert any(x["full_chunks"] == 7 and x["last"] == ORTHO_CHUNK for x in r) and any(c[:4] == (2, 8, 196, 384) for c in ORTHO_CASES), "the workload's n"
    assert sum(x["zero_rows"] for x in r) == 1, "exactly one case with whole rows equal to 0"
    assert any(c.B >= 2 for c in ORTHO_CASES if c.zero_rows)
    assert all(c.D % 4 == 0 and c.D <= ORTHO_MAX_D for c in ORTHO_CASES)
    assert INV_CLAMP == float(np.float32(1e12))  # the clamped inv_norm is the number ortho_bwd_kernel compares with


@pytest.mark.parametrize("case", ORTHO_CASES, ids=ORTHO_IDS)
def test_operands_are_what_the_docstring_says(case):
    B, C, n, D = case[:4]
    Y, coef, kind = ortho_operands(case)
    nz, mag = (Y != 0).sum(-1), Y.abs().amax(-1)
    for i, (k, m) in enumerate(ROW_KINDS):
        assert bool(((nz == k) & (mag == m))[kind == i].all())
    assert bool((Y[kind == -1] == 0).all()) and bool(((Y == 0) | (Y.abs() == mag[..., None])).all())
    assert (int((kind == -1).sum()) > 2) == case.zero_rows
    if D < 16:
        assert set(kind.flatten().tolist()) <= {1, 3}
    inv = ortho_expect(Y, coef, case)["inv_norm"]
    assert set(inv.flatten().tolist()) <= {0.25, 0.5, 0.125, INV_CLAMP}
    if not case.zero_rows:  # norms differ from row to row: a neighbour's inv_norm is another number
        assert bool((inv.flatten()[1:] != inv.flatten()[:-1]).all())
    assert set(coef.flatten().tolist()) <= set(COEF_VALUES)
    for j in range(2):
        assert len(set(coef[:, j].tolist())) == B  # pairwise different over the images


@pytest.mark.parametrize("case", ORTHO_CASES, ids=ORTHO_IDS)
def test_ortho_expectation_is_order_free(case):
    """Conditions (i) and (ii) of the module docstring for this case."""
    Y, coef, _ = ortho_operands(case)
    want = ortho_expect(Y, coef, case)
    assert 64 * max(want["sums"]) < 2 ** 24, want["sums"]
    if case.n == 1:
        assert bool((want["stats"][:, 0] == 0).all())
    if case.C == 1:
        assert bool((want["stats"][:, 1] == 0).all())
    if case.zero_rows:
        assert bool((want["inv_norm"][want["zero"]] == INV_CLAMP).all()) and bool((want["selfsq"].sum(1) < case.C * case.n).any())
        assert bool((want["dY"][want["zero"]] != 0).any())
    else:
        assert bool((want["selfsq"] == case.n).all())
    for order in ("seq", "tree"):
        for fma in (False, True):
            found = ortho_mismatches(ortho_restate(Y, coef, case, order, fma), want, Y, case)
            assert not found, f"order {order}, fma {fma}:\n" + "\n".join(found)


def _flagged(defect):
    """{case id: names of the outputs the exact rules flag} for one defect over the table."""
    out = {}
    for case, cid in zip(ORTHO_CASES, ORTHO_IDS):
        Y, coef, _ = ortho_operands(case)
        found = ortho_mismatches(ortho_restate(Y, coef, case, "tree", False, defect), ortho_expect(Y, coef, case), Y, case)
        if found:
            out[cid] = sorted(f.split(":")[0] for f in found)
    return out


def test_injected_defects_are_flagged_by_the_exact_rules():
    f = {d: _flagged(d) for d in DEFECTS}
    for d, v in f.items():
        print(d, v)
    assert set(f["ssq_drop"]) == set(ORTHO_IDS) and all(v == ["stats"] for v in f["ssq_drop"].values())
    assert set(f["dot_drop_col"]) == set(ORTHO_IDS) and all(v == ["dY"] for v in f["dot_drop_col"].values())
    assert set(f["inv_neighbour"]) == set(ORTHO_IDS) and all(v == ["dY"] for v in f["inv_neighbour"].values())
    multi = {cid for c, cid in zip(ORTHO_CASES, ORTHO_IDS) if c.B > 1}
    assert set(f["coef_prev_image"]) == multi and set(f["tot_prev_image"]) == {cid for c, cid in zip(ORTHO_CASES, ORTHO_IDS) if c.B > 1 and c.C > 1}
    # the two that no finite operand can show (module docstring): bit-identical on the whole table ...
    assert f["cb_at_c1"] == {} and f["clamp_projected"] == {}


def test_the_c1_guard_shows_on_a_non_finite_coef_only():
    """... cb_at_c1: with C == 1, tot is bitwise S and cb multiplies an exact 0; the guard decides between 0 and NaN when coef[:, 1] is not finite."""
    case = next(c for c in ORTHO_CASES if c.C == 1)
    Y, coef, _ = ortho_operands(case)
    coef = coef.clone()
    coef[:, 1] = float("inf")
    want = ortho_expect(Y, torch.stack([coef[:, 0], torch.zeros(case.B)], 1), case)
    assert not ortho_mismatches(ortho_restate(Y, coef, case, "tree", False), want, Y, case)
    found = ortho_mismatches(ortho_restate(Y, coef, case, "tree", False, "cb_at_c1"), want, Y, case)
    assert [f.split(":")[0] for f in found] == ["dY"]


def test_the_clamp_branch_shows_on_rows_of_norm_3e_13():
    """... clamp_projected: a row that is exactly 0 has fh = 0 and g . fh = 0 either way; on rows of norm 3e-13 (fh of norm 0.3) the projection takes 9 % of g
    along fh, which test_ortho_loss's bounds applied to the clamped rows alone flag — and which they miss when all rows share one max |grad|."""
    case, Y, coef, mask = clamp_operands()
    B, C, n, D = case
    ref = ortho_reference64(Y, coef, C, n)
    full = OrthoCase(B, C, n, D, True, "")
    good = ortho_restate(Y, coef, full, "tree", False)
    assert bool((good["inv_norm"][mask] == INV_CLAMP).all()) and bool((good["inv_norm"][~mask] < 1).all())
    assert old_bounds_findings(good, *ref, C, rows=mask) == []
    bad = ortho_restate(Y, coef, full, "tree", False, "clamp_projected")
    assert old_bounds_findings(bad, *ref, C, rows=mask) == ["dY clamped rows"]


OLD_SHAPES = ((3, 5, 16, 384), (2, 1, 9, 192), (2, 8, 196, 384), (2, 18, 16, 384))
#: defect -> per shape of OLD_SHAPES, the assertions of test_ortho_loss that fail on that test's own operands with the defect in the fp32 restatement ("-": the
#: test's bounds let the defect through at that shape).  Recorded from this test's own computation; nothing here was tuned.
OLD_BOUNDS_CATCH = {
    "ssq_drop":        ["-", "pos_sum", "-", "-"],   # one S^2 of 3072 at the headline shape: 8 in 2.5e4, bound 25
    "dot_drop_col":    ["dY", "dY", "dY", "dY"],     # randn + 0.3 rows all lean on the mean direction: every column carries a visible share of g . fh
    "inv_neighbour":   ["dY", "dY", "dY", "dY"],
    "coef_prev_image": ["dY", "dY", "dY", "dY"],
    "tot_prev_image":  ["dY", "-", "dY", "dY"],      # C == 1 multiplies tot - s_c = 0
    "cb_at_c1":        ["-", "-", "-", "-"],         # cannot show on finite operands (module docstring)
    "clamp_projected": ["-", "-", "-", "-"],         # no row of that test is under the clamp
}


def test_what_the_older_bounds_let_through():
    """Each defect on test_ortho_loss's operands against its three assertions; the outcome is recorded in OLD_BOUNDS_CATCH (and in the pull request that added
    this file).  Without a defect the restatement passes them."""
    shapes = old_ortho_cases()
    assert shapes == list(OLD_SHAPES)
    got = {d: [] for d in DEFECTS}
    for B, C, n, D in shapes:
        Y, coef = old_ortho_operands(B, C, n, D)
        ref = ortho_reference64(Y, coef, C, n)
        case = OrthoCase(B, C, n, D, False, "")
        assert old_bounds_findings(ortho_restate(Y, coef, case, "tree", False), *ref, C) == []
        for d in DEFECTS:
            got[d].append("+".join(old_bounds_findings(ortho_restate(Y, coef, case, "tree", False, d), *ref, C)) or "-")
    for d in DEFECTS:
        print(f"{d:16s}", got[d])
    assert got == OLD_BOUNDS_CATCH


def test_single_patch_defect_in_fp32():
    """The defect the fix removes, restated: at n == 1 on randn + 0.3 the two evaluations of the same number differ by rounding, and 1 / pos_cnt = 1e6 makes that
    a positive-pair term of order 0.1 .. 1 where the reference has exactly 0.  The fixed rule (pos_sum = 0 at n == 1) is what ortho_restate and ortho_expect use."""
    B, C, n, D = 4, 8, 1, 384
    worst = 0.0
    for seed in range(8):
        Y = torch.randn(B, C, D, generator=torch.Generator().manual_seed(seed)) + 0.3
        q = (Y * Y).sum(-1)
        inv = 1.0 / q.sqrt()
        a = ((Y * inv[..., None]) ** 2).sum((1, 2))
        sf = (q * inv * inv).sum(1)
        worst = max(worst, float((a - sf).abs().max()))
    assert 0 < worst < 1e-5  # not 0, and nothing but rounding
    assert worst / 1e-6 > 0.1  # ... which pos_cnt = 1e-6 turns into a term the loss can see


def test_proxy_restatement_and_shapes():
    """The fp32 restatement of proxy_loss_kernel stays within test_proxy_loss_kernel's bounds of float64 at the workload's scale on every shape and kind the GPU
    file runs; the shape list holds the sizes that file is about."""
    assert {(16, 1024), (32, 512)} == {s for s in PROXY_SHAPES if s[0] * s[1] == 16384} and all(c * d <= 16384 and c <= 32 and d <= 1024 for c, d in PROXY_SHAPES)
    assert any(d % 64 for _, d in PROXY_SHAPES) and any(d == 1000 for _, d in PROXY_SHAPES) and (1, 1) in PROXY_SHAPES
    assert all(2 * 4 * c * d <= 64 * 1024 for c, d in PROXY_SHAPES if c * d < 16384)  # only the two limit shapes take the large-LDS path
    for C, D in PROXY_SHAPES + [(8, 384)]:
        for kind in PROXY_KINDS + PROXY_STRUCTURED:
            if C == 1 and kind == "p = e[perm]":
                continue
            e, p = proxy_operands(C, D, kind)
            got, ref = proxy_restate(e, p, PROXY_SCALE), proxy_reference(e, p, PROXY_SCALE)
            if kind == "zero row":
                got, ref = (got[0], got[1][1:], got[2]), (ref[0], ref[1][1:], ref[2])
            assert max(proxy_errors(got, ref)) <= 1, (C, D, kind, proxy_errors(got, ref))
    assert all(int(proxy_perm(C)[i]) != i for C in (2, 5, 8) for i in range(C))


def test_proxy_saturation_operands_saturate():
    """At scale^2 = 200 the logits reach -800 and expf underflows off the maximum, in fp32 and for the diagonal of 'e = -p' in the restatement too; the measured
    restatement error, which the GPU test multiplies by PROXY_SAT_FACTOR, is finite and small."""
    e, p = proxy_operands(8, 384, "e = -p")
    a, b = PROXY_SCALE_SAT * F.normalize(e.double(), dim=-1), PROXY_SCALE_SAT * F.normalize(p.double(), dim=-1)
    L = -((a[:, None] - b[None]) ** 2).sum(-1)
    assert float(L.min()) < -799 and float((L - L.max(-1, keepdim=True).values).min()) < -104  # expf(-104) = 0 in fp32
    bound = proxy_saturation_bound()
    print("restatement error at saturation (loss, d_emb, d_proxies):", bound)
    assert all(math.isfinite(x) and 0 < x < 100 for x in bound)


def test_proxy_exact_rule_flags_a_shifted_class():
    """proxy_exact_findings on the restatement: clean as written; flagged when the identity is subtracted one class off (softmax - I[:, j + 1])."""
    e, p = proxy_exact_operands()
    C = e.shape[0]
    _, de, _ = proxy_restate(e, p, 2.0)
    assert proxy_exact_findings(de[0], p) == []
    # the same row with the target one class to the right
    sc = torch.tensor(2.0)
    pn = p / 4
    en = torch.cat([torch.zeros(1, e.shape[1]), e[1:] / 4])
    diff = sc * en[:, None, :] - sc * pn[None, :, :]
    L = -(diff * diff).sum(-1)
    W = ((L - L.logsumexp(-1, keepdim=True)).exp() - torch.eye(C).roll(1, 1)) / C
    wrong = sc * (W[0][:, None] * -2.0 * diff[0]).sum(0) / torch.tensor(1e-12)
    assert proxy_exact_findings(wrong, p) != []
