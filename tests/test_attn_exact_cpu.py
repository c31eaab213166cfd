"""Attention on operands for which every number the kernels round is exact: the builder, the closed-form expectation, the comparison rules of
tests/test_attn_exact_gpu.py, and the proof, without a GPU, that those rules flag one wrong term of N where the bf16 tolerances of the older tests do not.

"Group" operands (head_dim 64, scale 1/8).  Dimensions 0..11 of a key hold the +-1 code of its group, of a query BETA = 512 times the code of its target
group (zero elsewhere): the score is BETA * scale * (12 - 2 * Hamming distance), so the keys of the target group tie exactly at 768 nats and every other key
lies at least 128 nats = 185 log2 units below: its exp2 underflows to exactly zero in fp32, in the forward and in both backward kernels, and nothing from
outside the group reaches any sum.  (BETA = 128, a gap of 32 nats and p = 1e-14, is not enough on the hardware: where v or dO cancel exactly inside a group,
+2 - 2, the MFMA's aligned accumulation turned negative dust of 1e-14 into -2^-24, one unit of the alignment, measured on an MI355X in O, dQ and dV of
both chains; every nonzero expectation was bit-exact there too.)  Groups have 1, 2 or 4 keys, so P is 1, 1/2 or 1/4.  k carries 0 / 1 payloads in dimensions 12..63 (dQ lands
there), v is in {-2, 0, 2}, dO in {-1, 0, 1}; rows of dO are redrawn until P, dS, O, dQ, dK and dV are all exactly representable in bf16 and nonzero where a
softmax allows it.  A row whose target group has ONE key has P = 1 and therefore dS = 0 identically: such rows exist (one per 64-key tile: they alone can
raise a row's running maximum in a tile that holds a single key) and are checked through O, LSE and a zero dQ row; every other row has a nonzero dS.

The expectation is a closed form over the groups (gathers and index_add; no N x N matrix).  simulate() is the materialised float64 softmax of one (batch,
head) with the kernels' roundings and, optionally, a defect; it is the witness for both claims of this file."""
import math
import os
import sys
from collections import namedtuple

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_attn_seams_gpu import K3_KEYS, dkdv3_plan  # noqa: E402

SCALE = 0.125
BETA = 512.0
LOG2E = math.log2(math.e)
C = SCALE * LOG2E  # the pre-scaled chain's q~ = bf16(q * C)
DUST = 2.0 ** -30  # the most an output may hold where the expectation is zero (with BETA = 512 the kernels should leave exactly zero)
LSE_ULPS = 4       # fp32 ulps of |LSE|; see lse_mismatch
CUS = 256

# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Cases.  tail / in_loop: what dkdv3_plan must say at 256 CUs (asserted below and, with the device's CU count, on the GPU).
GCase = namedtuple("GCase", "B N H Nq tail in_loop")
GROUP_CASES = [
    GCase(1, 1, 1, None, "none", False), GCase(2, 17, 3, None, "none", False),                                  # fewer keys than one tile
    GCase(3, 63, 1, None, "none", False), GCase(1, 64, 2, None, "none", False), GCase(2, 65, 2, None, "none", False),  # the 64-key tile edge
    GCase(3, 128, 3, None, "none", False), GCase(1, 129, 3, None, "none", False),                               # the second tile edge
    GCase(2, 256, 1, None, "none", False), GCase(3, 257, 2, None, "tail2", False),                              # the 256-key item edge
    GCase(1, 289, 3, None, "tail2", False),                                                                     # remainder 33
    GCase(2, 321, 1, None, "ranged", False), GCase(3, 384, 2, None, "ranged", False),                           # remainders 65 and 128
    GCase(1, 385, 2, None, "none", False),                                                                      # remainder 129: no split
    GCase(2, 960, 3, None, "none", False), GCase(1, 981, 1, None, "none", True), GCase(3, 1040, 2, None, "tail2", True),  # nt 15, 16, 17
    GCase(2, 1569, 3, None, "tail2", True),                                                                     # headline token count
    GCase(3, 1569, 2, 1, "tail2", False), GCase(2, 600, 3, 33, "ranged", False), GCase(1, 257, 1, 64, "tail2", False),  # query-row subsets
    GCase(48, 289, 6, None, "tail2", False), GCase(12, 1040, 6, None, "tail2", True),                           # workgroups walk several items
]
BATCHED = [c for c in GROUP_CASES if c.B > 3]
GROUP_IDS = [f"B{c.B}-N{c.N}-H{c.H}-Nq{c.Nq or 'all'}" for c in GROUP_CASES]
UNIFORM_NS = list(range(1, 701)) + [1 + 196 * c for c in range(4, 9)]  # every N to 700, then the channel-sampling counts beyond (1 + 196 c <= 700 for c <= 3)
UNIFORM_CHUNKS = [UNIFORM_NS[i:i + 90] for i in range(0, len(UNIFORM_NS), 90)]

# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Structure: which keys form a group, which group a query row targets.  Shared by all (batch, head) pairs of a case; the payloads differ.
Structure = namedtuple("Structure", "N Nq gid gsize code tgt pi pj singles")


def structure(N, Nq=None, seed=0):
    Nq = N if Nq is None else Nq
    g = torch.Generator().manual_seed(7919 * N + 31 * Nq + seed)
    nt = -(-N // 64)
    # one single-key group per 64-key tile; the last key the mask admits, N - 1, is one only when it is alone in its tile: elsewhere it belongs to the
    # first group of 4, which row 0 targets, so that a mask off by one shows in dQ as well
    singles = [64 * t + (17 * t + 5) % min(64, N - 64 * t) for t in range(nt)]
    if singles[-1] == N - 1 and N % 64 != 1:
        singles[-1] -= 1
    rest = [j for j in torch.randperm(N, generator=g).tolist() if j not in set(singles) and j != N - 1]
    if N - 1 not in singles:
        rest.insert(0, N - 1)
    groups = [[j] for j in singles]
    want = 4
    while rest:
        n = want if len(rest) >= want else (2 if len(rest) >= 2 else 1)
        groups.append(rest[:n])
        rest = rest[n:]
        want = 6 - want  # 4, 2, 4, 2, ...
    assert len(groups) <= 4096
    gid = torch.empty(N, dtype=torch.long)
    for i, grp in enumerate(groups):
        gid[grp] = i
    gsize = torch.tensor([len(grp) for grp in groups])
    cid = (torch.arange(len(groups)) * 2731 + 1234) % 4096  # a bijection of the 12-bit codes: neighbouring groups are not neighbouring codes
    code = (((cid[:, None] >> torch.arange(12)) & 1) * 2 - 1).double()
    # query rows: row 0 targets a group of 4 (of 2 when there is none), so that Nq = 1 has a dS; then a group of 2, the singles, the rest
    by_size = {n: [grp for grp in groups if len(grp) == n] for n in (1, 2, 4)}
    head = [by_size[n][0][0] for n in (4, 2) if by_size[n]] + singles
    order = head + [j for j in torch.randperm(N, generator=g).tolist() if j not in set(head)]
    order = order[:Nq]
    if Nq > 2:
        order = order[:1] + [order[1 + i] for i in torch.randperm(Nq - 1, generator=g).tolist()]
    tgt = gid[torch.tensor(order)]
    pairs = [(i, j) for i in range(Nq) for j in groups[int(tgt[i])]]  # (query row, key of its group): the only nonzero entries of P and dS
    pi, pj = (torch.tensor(x, dtype=torch.long) for x in zip(*pairs))
    return Structure(N, Nq, gid, gsize, code, tgt, pi, pj, singles)


def closed_form(st, k, v, dO, qamp):
    """Ideal o, lse, dq, dk, dv (float64, [P, rows, 64]; lse [P, Nq]) and the nonzero entries of P and dS ([np], [P, np]) for P (batch, head) problems
    that share a structure.  k, v [P, N, 64], dO [P, Nq, 64]; the query rows are qamp * code of the target group in units where the score is
    SCALE * q . k (plain chain: BETA; pre-scaled chain: bf16(BETA * C) / C, what the kernels see, unscaled)."""
    Pn, N = k.shape[0], st.N
    gs = st.gsize.double()
    o = (torch.zeros(Pn, len(gs), 64, dtype=torch.float64).index_add_(1, st.gid, v) / gs[None, :, None])[:, st.tgt]
    lse = (SCALE * qamp * 12 + gs[st.tgt].log()).expand(Pn, -1)
    q = torch.zeros(st.Nq, 64, dtype=torch.float64)
    q[:, :12] = qamp * st.code[st.tgt]
    p = 1.0 / gs[st.tgt[st.pi]]
    delta = (dO * o).sum(-1)
    ds = ((dO[:, st.pi] * v[:, st.pj]).sum(-1) - delta[:, st.pi]) * p
    dq = SCALE * torch.zeros(Pn, st.Nq, 64, dtype=torch.float64).index_add_(1, st.pi, ds[..., None] * k[:, st.pj])
    dk = SCALE * torch.zeros(Pn, N, 64, dtype=torch.float64).index_add_(1, st.pj, ds[..., None] * q[st.pi][None])
    dv = torch.zeros(Pn, N, 64, dtype=torch.float64).index_add_(1, st.pj, dO[:, st.pi] * p[None, :, None])
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, p=p, ds=ds)


def bf16_exact(x):
    return x.to(torch.bfloat16).double() == x


GroupOps = namedtuple("GroupOps", "case st k v dO plain ps")
_cache = {}


def group_operands(case):
    """k, v [P, N, 64] and dO [P, Nq, 64] in float64 (every value a bf16 number), P = B * H problems with their own payloads, and the two chains'
    expectations.  Rows of dO are redrawn (a fixed generator) until the ideal tensors are bf16-exact and nonzero where they can be."""
    if case in _cache:
        return _cache[case]
    st = structure(case.N, case.Nq)
    Pn, N, Nq = case.B * case.H, st.N, st.Nq
    g = torch.Generator().manual_seed(1000 * N + 10 * case.B + case.H)
    k = torch.zeros(Pn, N, 64, dtype=torch.float64)
    k[:, :, :12] = st.code[st.gid]
    k[:, :, 12:] = torch.randint(0, 2, (Pn, N, 52), generator=g).double()
    v = torch.tensor([-2.0, 0.0, 0.0, 2.0], dtype=torch.float64)[torch.randint(0, 4, (Pn, N, 64), generator=g)]
    dO = torch.randint(-1, 2, (Pn, Nq, 64), generator=g).double()
    G = len(st.gsize)
    multi = (st.gsize > 1)[st.tgt]  # rows that have a dS at all
    targeted = torch.zeros(N, dtype=torch.bool)
    targeted[st.pj] = True
    todo = torch.arange(Pn)  # the problems that still have a flaw
    for _ in range(400):
        e = closed_form(st, k[todo], v[todo], dO[todo], BETA)
        n = len(todo)
        row_bad = ~(bf16_exact(e["o"]).all(-1) & bf16_exact(e["dq"]).all(-1))
        row_bad |= multi & ~(e["dq"][:, :, 12:] != 0).any(-1)
        pair_bad = ~bf16_exact(e["ds"]) | (e["ds"] == 0)
        key_bad = ~(bf16_exact(e["dk"]).all(-1) & bf16_exact(e["dv"]).all(-1))  # [n, N]
        key_bad |= (targeted & (st.gsize[st.gid] > 1))[None] & ~(e["dk"] != 0).any(-1)
        key_bad |= targeted[None] & ~(e["dv"] != 0).any(-1)
        grp_bad = torch.zeros(n, G, dtype=torch.long)
        grp_bad.scatter_add_(1, st.tgt[None].expand(n, -1), row_bad.long())
        grp_bad.scatter_add_(1, st.tgt[st.pi][None].expand(n, -1), (pair_bad & multi[st.pi][None]).long())
        grp_bad.scatter_add_(1, st.gid[None].expand(n, -1), key_bad.long())
        redo = grp_bad[:, st.tgt] > 0  # every row that targets a group with a flaw
        if not redo.any():
            break
        sub = dO[todo]
        sub[redo] = torch.randint(-1, 2, (int(redo.sum()), 64), generator=g).double()
        dO[todo] = sub
        todo = todo[redo.any(-1)]
    else:
        raise AssertionError(f"{case}: no exact payload found")
    e = closed_form(st, k, v, dO, BETA)
    qt = float(torch.tensor(BETA * C).to(torch.bfloat16))  # 92.5
    ops = GroupOps(case, st, k, v, dO, e, closed_form(st, k, v, dO, qt / C))
    _cache[case] = ops
    return ops


def to_device_layout(ops, prescaled):
    """qkv [B, N, 3 H 64] bf16 as the chain reads it, and dO [B, N, H 64] bf16 whose rows >= Nq are NaN (not the kernels' to read)."""
    c, st = ops.case, ops.st
    B, H, N = c.B, c.H, c.N
    q = torch.zeros(st.N, 64, dtype=torch.float64)
    q[:st.Nq, :12] = BETA * st.code[st.tgt]
    q = q[None].expand(B * H, -1, -1)
    if prescaled:
        q = (q.float() * C).to(torch.bfloat16).double()
    qkv = torch.stack([x.reshape(B, H, N, 64).transpose(1, 2) for x in (q, ops.k, ops.v)], 2).reshape(B, N, 3 * H * 64).to(torch.bfloat16)
    dO = torch.full((B, N, H * 64), float("nan"), dtype=torch.bfloat16)
    dO[:, :st.Nq] = ops.dO.reshape(B, H, st.Nq, 64).transpose(1, 2).reshape(B, st.Nq, H * 64).to(torch.bfloat16)
    return qkv, dO


def from_device_layout(x, B, H):
    """[B, rows, H 64] -> [B H, rows, 64]."""
    return x.reshape(B, x.shape[1], H, 64).transpose(1, 2).reshape(B * H, x.shape[1], 64)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The comparison rules.  Each returns the mask of failing elements; NaN (memory a kernel left untouched) always fails.
def exact_mismatch(got, want):
    """Bit-exact: the bf16 pattern where the expectation is nonzero, |x| <= 2^-30 where it is zero."""
    w = want.to(torch.bfloat16)
    assert bool((w.double() == want).all()), "the expectation itself is not a bf16 number"
    return torch.where(want != 0, got.view(torch.int16) != w.view(torch.int16), ~(got.double().abs() <= DUST))


def ulp1_mismatch(got, want):
    """At most one bf16 ulp of the float64 expectation (2^-30 where that is zero)."""
    _, e = torch.frexp(want)  # |want| in [2^(e-1), 2^e): eight significant bits -> ulp 2^(e-8)
    tol = torch.where(want != 0, torch.ldexp(torch.ones_like(want), e - 8), torch.full_like(want, DUST))
    return ~((got.double() - want).abs() <= tol)


def lse_mismatch(got, want, ulps=LSE_ULPS):
    """LSE in fp32 against float64, in fp32 ulps of |LSE|.  attn.hip:245 is fl(fl(m * k) + logf(l)):
      plain chain       m * scale is exact for scale = 1/8.  p = exp2(fma(s, c, -fl(m c))): the argument of a tied key is the rounding error of m c, at
                        most half an ulp of 1108 log2 units = 2^-14, so ln l is off by at most 2^-14 ln 2 = 4.2e-5 = 0.7 ulp of 768 (without the
                        contraction the argument is exactly zero);
      pre-scaled chain  the tied scores cancel -m exactly, l is the group size; 1 / log2 e as an fp32 constant is off by at most 2^-25 relative
                        (0.4 ulp of the product) and the product rounds once (0.5 ulp);
      both              logf to 1 ulp of ln l <= ln 4 (0.002 ulp of 768; the whole error when m = 0) and the final add (0.5 ulp).
    That is at most 1.6 ulp; the bound is 4 ulp (2.4e-4 at 768 nats, 5e-7 at ln 4), far below the ln(5/4) = 0.22 of one key too many in a group of 4
    or the 1 / N >= 6e-4 of one key too many among N <= 1569 equal ones."""
    _, e = torch.frexp(want)
    return ~((got.double() - want).abs() <= ulps * torch.ldexp(torch.ones_like(want), e - 24))


def describe(name, bad, H, key_rows):
    """Names the first failing rows: (batch, head), row, its 64-row tile and, for dK / dV, its 256-key item."""
    idx = bad.flatten(2).any(-1).nonzero()
    if len(idx) == 0:
        return None
    first = ", ".join(f"(b {int(p) // H}, h {int(p) % H}) row {int(r)} = tile {int(r) // 64}" + (f", item {int(r) // K3_KEYS}" if key_rows else "")
                      for p, r in idx[:6].tolist())
    return f"{name}: {int(bad.sum())} elements in {len(idx)} rows wrong; first: {first}"


def compare_group(got, exp, H, prescaled):
    """got / exp: o, lse, dq, dk, dv in [P, rows, 64] layout (lse [P, Nq]; got's dq has all N rows).  Returns the list of findings (empty: pass).
      O   bit-exact: attn.hip:235-243 multiplies the exact integer sums by fl(1 / l), l within 5e-5 of a power of two; the bf16 rounding lands on the ideal
      dV  bit-exact: attn_bwd.hip:370-385 (attn_bwd3.hip:274-285) rounds p = exp2(..) = (1 + 2e-4) / G to bf16 = 1 / G exactly; sums of dO / G are exact in fp32
      dQ  bit-exact: dS = bf16(p (dP - delta)) (attn_bwd.hip:178-186) is the ideal for the same reason; x scale = 1/8 at attn_bwd.hip:223 is exact
      dK  plain chain: bit-exact (scale = 1/8 at attn_bwd.hip:431); pre-scaled chain: one inexact factor 1 / log2 e (attn_bwd.hip:431, attn_bwd3.hip:338)
          on an exact sum, rounded to fp32 and to bf16: at most one bf16 ulp
      dQ rows >= Nq are exactly zero."""
    nq = exp["o"].shape[1]
    out = [describe("O", exact_mismatch(got["o"][:, :nq], exp["o"]), H, False),
           describe("LSE", lse_mismatch(got["lse"][:, :nq], exp["lse"])[..., None], H, False),
           describe("dQ", exact_mismatch(got["dq"][:, :nq], exp["dq"]), H, False),
           describe("dQ rows >= Nq (not zero)", got["dq"][:, nq:].view(torch.int16) != 0, H, False),
           describe("dK", (ulp1_mismatch if prescaled else exact_mismatch)(got["dk"], exp["dk"]), H, True),
           describe("dV", exact_mismatch(got["dv"], exp["dv"]), H, True)]
    return [x for x in out if x]


def old_bounds_flag(got, ref):
    """The bounds of test_attention_fwd_bwd: O 2e-2 / 2e-2, LSE 1e-4 / 2e-3, dQ / dK / dV rtol 3e-2 and atol 3e-2 max|ref| of the slot."""
    def off(a, b, rtol, atol):
        return bool(((a.double() - b).abs() > atol + rtol * b.abs()).any()) or not bool(torch.isfinite(a.double()).all())
    hit = [n for n, r, a in (("O", 2e-2, 2e-2), ("LSE", 1e-4, 2e-3)) if off(got[n.lower()], ref[n.lower()], r, a)]
    return hit + [n for n in ("dQ", "dK", "dV") if off(got[n.lower()], ref[n.lower()], 3e-2, 3e-2 * ref[n.lower()].abs().max().item())]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The materialised float64 model of one (batch, head), with the kernels' roundings and optionally one defect.
def _bf(x):
    return x.to(torch.bfloat16).double()


def simulate(q, k, v, dO, scale, defect=None, rounded=True):
    """q, dO [Nq, 64], k, v [N, 64] float64.  Returns o, lse [Nq], dq, dk, dv; with `rounded` as the kernels round them (O, P, dS and the outputs to bf16,
    LSE to fp32), else plain float64.  defect = (kind, ...):
      fwd_key / dq_key (j, w)    key j counts w times (0: dropped, 2: taken twice) in the forward / in the dQ kernel; the mask off by one is key N - 1
                                 dropped, or taken twice (rows >= N are clamped to N - 1: attn.hip:63-66)
      dk_row / dv_row (i, lo, hi)  query row i is missing from the dK / dV sums of keys lo..hi-1
      rescale (i, t)             row i's accumulators are not rescaled when its maximum rises in key tile t
      overlap / gap (j)          two launches split the keys at j: key j is accumulated by both / key j is written by neither"""
    Nq, N = q.shape[0], k.shape[0]
    kind, args = (defect[0], defect[1:]) if defect else (None, ())
    rb = _bf if rounded else (lambda x: x)
    s = scale * q @ k.T
    wf = torch.ones(N, dtype=torch.float64)
    wq = wf.clone()
    rk = torch.ones(Nq, N, dtype=torch.float64)
    rv = rk.clone()
    if kind == "fwd_key":
        wf[args[0]] = args[1]
    if kind == "dq_key":
        wq[args[0]] = args[1]
    if kind in ("dk_row", "dv_row"):
        (rk if kind == "dk_row" else rv)[args[0], args[1]:args[2]] = 0
    if kind == "overlap":
        rk[:, args[0]] = rv[:, args[0]] = 2
    m = torch.where(wf > 0, s, torch.full_like(s, -math.inf)).max(-1).values
    e = (s - m[:, None]).exp() * wf
    if kind == "rescale":
        i, t = args
        assert 0 < 64 * t < N and s[i, :64 * t].max() < s[i, 64 * t:64 * t + 64].max()
        e[i, :64 * t] = (s[i, :64 * t] - s[i, :64 * t].max()).exp() * wf[:64 * t]  # still relative to the old maximum
    l = e.sum(-1)
    o = rb(e @ v / l[:, None])
    lse = m + l.log()
    if rounded:
        lse = lse.float().double()
    p = (s - lse[:, None]).exp()
    ds = rb(p * (dO @ v.T - (dO * o).sum(-1)[:, None]))
    p = rb(p)
    out = dict(o=o, lse=lse, dq=rb(scale * (ds * wq) @ k), dk=rb(scale * (ds * rk).T @ q), dv=rb((p * rv).T @ dO))
    if kind == "gap":
        out["dk"][args[0]] = out["dv"][args[0]] = float("nan")
    return out


def _as_got(sim, N):
    """simulate()'s output as compare_group's `got`: one problem, bf16 outputs, dQ padded to N rows of zeros."""
    dq = torch.zeros(N, 64, dtype=torch.float64)
    dq[:sim["dq"].shape[0]] = sim["dq"]
    return dict(o=sim["o"].to(torch.bfloat16)[None], lse=sim["lse"].float()[None], dq=dq.to(torch.bfloat16)[None],
                dk=sim["dk"].to(torch.bfloat16)[None], dv=sim["dv"].to(torch.bfloat16)[None])


def _problem(ops, n, prescaled):
    """Problem n of a case as simulate() takes it, and its expectation."""
    st = ops.st
    amp = float(torch.tensor(BETA * C).to(torch.bfloat16)) / C if prescaled else BETA
    q = torch.zeros(st.Nq, 64, dtype=torch.float64)
    q[:, :12] = amp * st.code[st.tgt]
    e = ops.ps if prescaled else ops.plain
    return q, ops.k[n], ops.v[n], ops.dO[n], {x: e[x][n:n + 1] for x in ("o", "lse", "dq", "dk", "dv")}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GROUP_CASES, ids=GROUP_IDS)
def test_the_case_reaches_the_path_it_is_listed_for(case):
    p = dkdv3_plan(case.B, case.N, case.H, case.Nq, CUS)
    assert (p.tail, p.in_loop) == (case.tail, case.in_loop)
    if case in BATCHED:
        assert p.walk_max >= 2


def test_the_table_covers_the_edges():
    plans = {c: dkdv3_plan(c.B, c.N, c.H, c.Nq, CUS) for c in GROUP_CASES}
    full = {c.N for c in GROUP_CASES if c.Nq is None}
    assert {1, 17, 63, 64, 65, 128, 129, 256, 257, 289, 321, 384, 385, 960, 981, 1040, 1569} <= full
    assert {(c.N, c.Nq) for c in GROUP_CASES if c.Nq} == {(1569, 1), (600, 33), (257, 64)}
    assert {plans[c].rem for c in GROUP_CASES} >= {1, 33, 65, 128, 129}
    assert {15, 16, 17} <= {p.nt for p in plans.values()}
    assert (48, 289, 6) in {(c.B, c.N, c.H) for c in BATCHED} and any(c.N >= 1024 for c in BATCHED)
    assert all(1 <= c.B <= 3 and 1 <= c.H <= 3 for c in GROUP_CASES if c not in BATCHED)
    assert set(range(1, 701)) <= set(UNIFORM_NS) and {1 + 196 * c for c in range(1, 9)} <= set(UNIFORM_NS)
    assert {1 + 16 * c for c in range(1, 19)} <= set(UNIFORM_NS) and sum(UNIFORM_CHUNKS, []) == UNIFORM_NS


@pytest.mark.parametrize("case", GROUP_CASES, ids=GROUP_IDS)
def test_group_operands_meet_the_conditions(case):
    ops = group_operands(case)
    st, N, Nq = ops.st, case.N, ops.st.Nq
    nt = -(-N // 64)
    qkv, dOd = to_device_layout(ops, False)
    assert bool((from_device_layout(qkv[:, :, 2 * case.H * 64:].double(), case.B, case.H) == ops.v).all())  # the operands survive the bf16 layout
    assert bool((from_device_layout(qkv[:, :, case.H * 64:2 * case.H * 64].double(), case.B, case.H) == ops.k).all())
    assert bool((from_device_layout(dOd[:, :Nq].double(), case.B, case.H) == ops.dO).all()) and bool(dOd[:, Nq:].isnan().all())
    multi_row = (st.gsize > 1)[st.tgt]
    multi_pair = multi_row[st.pi]
    targeted = torch.zeros(N, dtype=torch.bool)
    targeted[st.pj] = True
    for e in (ops.plain, ops.ps):
        # ideal P and dS and the ideal outputs are bf16 numbers (dK of the pre-scaled chain carries 1 / log2 e: held to one ulp, not bit for bit)
        assert bool(bf16_exact(e["p"]).all()) and bool(bf16_exact(e["ds"]).all())
        for nm in ("o", "dq", "dv") + (("dk",) if e is ops.plain else ()):
            assert bool(bf16_exact(e[nm]).all()), nm
        # every row that can have a dS (a group of 2 or 4) has one, with a dQ in the payload dimensions; rows of a single key have none
        assert bool((e["ds"][:, multi_pair] != 0).all()) and bool((e["ds"][:, ~multi_pair] == 0).all())
        assert bool((e["dq"][:, multi_row, 12:] != 0).any(-1).all()) and bool((e["dq"][:, :, :12] == 0).all())
        # every targeted key has a dV row, and a dK row when its group has partners
        assert bool((e["dv"][:, targeted] != 0).any(-1).all()) and bool((e["dv"][:, ~targeted] == 0).all())
        assert bool((e["dk"][:, targeted & (st.gsize[st.gid] > 1)] != 0).any(-1).all())
    assert bool(multi_row[0]) or N == 1  # row 0 has a dS, so Nq = 1 has one (a single key has none to give)
    assert int((~multi_row).sum()) <= nt + 1  # rows without a dS: the singles only
    # O names its keys and dV its queries: rows of different groups differ, in every problem
    first = torch.tensor([int((st.tgt == t).nonzero()[0]) for t in st.tgt.unique()])
    keys = torch.tensor([int((st.gid == t).nonzero()[0]) for t in st.tgt.unique()])
    for n in range(0, case.B * case.H, max(1, case.B * case.H // 4)):
        assert len(ops.plain["o"][n, first].unique(dim=0)) == len(first) and len(ops.plain["dv"][n, keys].unique(dim=0)) == len(keys)
    # every 64-key tile, the first, the last and the masked one included, holds a key that is some row's sole maximum; with a row for each
    # (not when Nq is smaller than the number of tiles) the running maximum of some row rises in every tile
    assert all(any(64 * t <= j < 64 * t + 64 for j in st.singles) for t in range(nt))
    tiles_hit = {j // 64 for j in st.singles if int(st.gid[j]) in set(st.tgt.tolist())}
    if Nq >= nt + 3:
        assert tiles_hit == set(range(nt))
        if nt > 1:  # some rows meet their maximum only in a late tile: every key of their group lies in the last one
            assert any(min(int(j) for j in (st.gid == t).nonzero().flatten()) >= 64 * (nt - 1) for t in st.tgt.tolist())
    # partners sit in different tiles, different items, and on either side of the remainder split
    groups = [(st.gid == t).nonzero().flatten().tolist() for t in range(len(st.gsize)) if st.gsize[t] > 1]
    p = dkdv3_plan(case.B, N, case.H, case.Nq, CUS)
    if N > 64 + 8:
        assert any(len({j // 64 for j in grp}) > 1 for grp in groups)
    if N > K3_KEYS + 8:
        assert any(len({j // K3_KEYS for j in grp}) > 1 for grp in groups)
    if p.split and p.rem >= 8:
        assert any(len({j >= p.key_hi for j in grp}) > 1 for grp in groups)


@pytest.mark.parametrize("case", GROUP_CASES, ids=GROUP_IDS)
def test_the_float64_softmax_is_the_ideal(case):
    """The materialised softmax of the operands, in plain float64, leaves at most 2^-30 outside the closed form (P itself included), and with the kernels'
    roundings it passes the comparison rules: the expectation is right, and reachable.  Batched cases: a spread of their (batch, head) pairs."""
    ops = group_operands(case)
    Pn = case.B * case.H
    for n in sorted({0, Pn - 1} | set(range(0, Pn, max(1, Pn // 6)))):
        for prescaled in (False, True):
            q, k, v, dO, exp = _problem(ops, n, prescaled)
            pure = simulate(q, k, v, dO, SCALE, rounded=False)
            for nm in ("o", "lse", "dq", "dk", "dv"):
                assert float((pure[nm] - exp[nm][0]).abs().max()) <= DUST, (n, prescaled, nm)
            s = SCALE * q @ k.T
            pm = (s - torch.logsumexp(s, -1, keepdim=True)).exp()
            ideal = torch.zeros_like(pm)
            ideal[ops.st.pi, ops.st.pj] = ops.plain["p"]
            assert float((pm - ideal).abs().max()) <= DUST
            assert compare_group(_as_got(simulate(q, k, v, dO, SCALE), case.N), exp, case.H, prescaled) == []


def _gauss(N, seed):
    """The operands of test_attention_fwd_bwd (one head): N(0, 1.5) in bf16, one query x 4 and one late key equal to it; dO N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(N, 3, 64, generator=g) * 1.5).to(torch.bfloat16)
    qkv[N // 2, 0] *= 4
    qkv[N - 1, 1] = qkv[N // 2, 0]
    return qkv[:, 0].double(), qkv[:, 1].double(), qkv[:, 2].double(), torch.randn(N, 64, generator=g).to(torch.bfloat16).double()


DEFECT_CASES = [c for c in GROUP_CASES if (c.N, c.Nq, c.B) in ((289, None, 1), (1569, None, 2))]


def _defects(ops):
    """(name, defect) for one problem of a case: each placed where the issue's list puts it, on a row or key that the operands make observable."""
    st, N = ops.st, ops.case.N
    p = dkdv3_plan(ops.case.B, N, ops.case.H, ops.case.Nq, CUS)
    key_of = lambda i: [int(j) for j in (st.gid == st.tgt[i]).nonzero().flatten()]  # noqa: E731
    late = next(i for i in range(st.Nq) if min(key_of(i)) >= 64 and st.gsize[st.tgt[i]] > 1)  # a row whose maximum arrives after the first tile
    out = [("forward: key 64 dropped (tile edge)", ("fwd_key", 64, 0)), ("forward: key 63 taken twice (tile edge)", ("fwd_key", 63, 2)),
           ("forward: mask one key short", ("fwd_key", N - 1, 0)), ("forward: mask one key long", ("fwd_key", N - 1, 2)),
           ("dQ: mask one key short", ("dq_key", N - 1, 0)), ("dQ: mask one key long", ("dq_key", N - 1, 2)),
           ("dQ: key 64 taken twice (tile edge)", ("dq_key", 64 if st.gsize[st.gid[64]] > 1 else 65, 2)),
           (f"forward: rescale of row {late} skipped", ("rescale", late, min(key_of(late)) // 64))]
    for i, what in ((63, "tile edge"), (64, "tile edge"), (256, "item edge")):
        i = next(r for r in range(i, st.Nq) if st.gsize[st.tgt[r]] > 1)  # (a row of a single key has no dS)
        j = key_of(i)[0] // K3_KEYS * K3_KEYS
        out += [(f"dK: query row {i} ({what}) missing from item {j // K3_KEYS}", ("dk_row", i, j, j + K3_KEYS)),
                (f"dV: query row {i} ({what}) missing from item {j // K3_KEYS}", ("dv_row", i, j, j + K3_KEYS))]
    if p.split:
        j = p.key_hi if st.gsize[st.gid[p.key_hi]] > 1 else p.key_hi + 1
        out += [(f"dK / dV: tail and persistent launch overlap at key {j}", ("overlap", j)), (f"dK / dV: tail and persistent launch leave out key {j}", ("gap", j))]
    return out


@pytest.mark.parametrize("case", DEFECT_CASES, ids=[f"N{c.N}" for c in DEFECT_CASES])
def test_every_injected_defect_is_flagged(case, capsys):
    """Each defect, injected into the model of one (batch, head) on the group operands, is flagged by compare_group on both chains.  The same defect on the
    Gaussian operands of test_attention_fwd_bwd against that test's bounds is printed, not asserted: it records the gap."""
    ops = group_operands(case)
    gq, gk, gv, gdO = _gauss(case.N, case.N)
    gref = simulate(gq, gk, gv, gdO, SCALE, rounded=False)
    assert old_bounds_flag(simulate(gq, gk, gv, gdO, SCALE), gref) == []  # the model without a defect is inside the old bounds
    lines = []
    for name, defect in _defects(ops):
        for prescaled in (False, True):
            q, k, v, dO, exp = _problem(ops, 0, prescaled)
            found = compare_group(_as_got(simulate(q, k, v, dO, SCALE, defect), case.N), exp, case.H, prescaled)
            assert found, f"{name} ({'pre-scaled' if prescaled else 'plain'} chain) passes the exact comparison"
        if defect[0] == "rescale":  # on the Gaussian operands: the spiked row, whose maximum arrives with the last key
            defect = ("rescale", case.N // 2, (case.N - 1) // 64)
        old = old_bounds_flag(simulate(gq, gk, gv, gdO, SCALE, defect), gref)
        lines.append(f"N {case.N}: {name}: exact operands flag {found[0].split(':')[0]}; old bounds on Gaussian operands: {'flag ' + ', '.join(old) if old else 'MISS'}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
