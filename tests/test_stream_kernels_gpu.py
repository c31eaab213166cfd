"""The memory-bound ("streaming") kernels past their grid caps, against float64.

Every one of these entries caps its grid and walks the rest of the data in a grid-stride loop; the older kernel-level tests stay below
the caps, so each thread ran its loop body once.  This module holds

* the launch plans of those entries, restated in pure Python with file:line references (checked without a GPU by
  test_stream_kernels_cpu.py, which also asserts that the case tables below contain every regime), and
* the GPU tests over those tables.  Two families of inputs:
    - EXACT inputs for everything that sums across rows or workgroups (LayerNorm's dgamma / dbeta, the gradient norm's sum of squares,
      the tokeniser's dE / dpos / dcls): small integers (or half-integers), so that every product and every partial sum is exactly
      representable in fp32.  The result then does not depend on the order of the additions, the int64 / float64 reference rounds to the
      same fp32 number, and the assertion is torch.equal in both reduction modes (hence also between them).  The condition - the sum of
      the absolute values of all terms of an output element, initial value included, stays below 2^23 quanta - is asserted by each test on
      its own inputs before the kernel runs.  One lost or doubled row cannot hide inside a tolerance because there is none.
    - RANDOM inputs for what is rounded per element, against the same formula in float64 from the kernel's own fp32 / bf16 operands.
"""
import math
import os
import re
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # test_kernels_gpu's helpers

pytestmark = pytest.mark.gpu

HEADLINE_M = 64 * 1569          # token rows of the batch-64 step
ARENA_FLOATS = 21_599_009       # parameters of the S / 8-channel / 161-class model: the optimiser's and the casts' range
SENT = -12345.0                 # sentinel for "never written"


# =====================================================================================================================================
# Launch plans (pure Python; no GPU).  Each restates the host launch code and the kernel's loop.
# =====================================================================================================================================
def _cdiv(a, b):
    return -(-a // b)


LnFwdPlan = namedtuple("LnFwdPlan", "grid stride rows_max rows_min")


def ln_fwd_plan(M):
    """csrc/norm.hip:235-236 (grid = min(ceil(M / 4), 4096) workgroups of 4 waves) and :88-103 (wave w of workgroup b takes rows
    4 b + w, + 4 grid, ...)."""
    grid = min(_cdiv(M, 4), 4096)
    stride = 4 * grid
    return LnFwdPlan(grid, stride, _cdiv(M, stride), M // stride)


LnBwdPlan = namedtuple("LnBwdPlan", "grid stride classes")


def ln_bwd_plan(M):
    """csrc/norm.hip:251-254 (grid = min(ceil(M / 4), 1024)) and :189-202: a wave with first row r walks rows r, r + stride, ... two at a
    time while `row + stride < M`, then one more if `row < M`.  classes: the set of (pairs, trailing single row) over the launch's waves."""
    grid = min(_cdiv(M, 4), 1024)
    stride = 4 * grid
    q, rem = divmod(M, stride)
    counts = set()
    if rem:
        counts.add(q + 1)
    if rem < stride:
        counts.add(q)
    classes = set()
    for cnt in counts:  # replay the loop literally for a wave with cnt rows
        row, pairs = 0, 0
        m = cnt * stride  # rows 0, stride, ..., (cnt - 1) stride exist for this wave
        while row + stride < m:
            pairs += 1
            row += 2 * stride
        single = 1 if row < m else 0
        assert 2 * pairs + single == cnt
        classes.add((pairs, single))
    return LnBwdPlan(grid, stride, frozenset(classes))


DetPlan = namedtuple("DetPlan", "tall vec unrolled remainder nv grid")
DET_TALL_CG, DET_TALL_PL = 4, 64  # csrc/det_reduce.hip


def det_reduce_plan(nparts, nA, QA, ldA, nB, part_stride, aligned=True):
    """csrc/det_reduce.hip det_reduce().  vec: every extent a multiple of 4 and 16-byte aligned pointers; tall: nparts >= 32 and at most 16 384
    column groups; unrolled: the 8-loads-in-flight loop runs at least once (flat :219 `k + 8 <= nparts`; tall :266, part lane 0:
    `7 * 64 < nparts`); remainder: some thread then adds parts one at a time (flat :234, tall :281)."""
    vec = aligned and not any(v & 3 for v in (nA, QA, ldA, nB, part_stride))
    nv = (nA + nB) // (4 if vec else 1)
    tall = nparts >= 32 and nv <= 16384
    if tall:
        unrolled = remainder = False
        for pl in range(DET_TALL_PL):  # replay the two loops of a part lane
            k = pl
            while k + 7 * DET_TALL_PL < nparts:
                unrolled = True
                k += 8 * DET_TALL_PL
            remainder = remainder or k < nparts
        return DetPlan(True, vec, unrolled, remainder, nv, _cdiv(nv, DET_TALL_CG))
    return DetPlan(False, vec, nparts >= 8, nparts % 8 != 0, nv, max(1, min(_cdiv(nv, 256), 2048)))


def ln_bwd_det_plan(M, D, aligned=True):
    """csrc/norm.hip:276: one part of 2 D floats per workgroup, dgamma then dbeta."""
    return det_reduce_plan(ln_bwd_plan(M).grid, D, D, D, D, 2 * D, aligned)


def ln_bwd_ws_floats(M, D):
    return ln_bwd_plan(M).grid * 2 * D  # csrc/norm.hip:286


FlatPlan = namedtuple("FlatPlan", "grid n4 full_rounds ragged tail iters_max")
FLAT_CAPS = {"adamw": 4096, "clip_scale": 4096, "cast_bf16": 8192, "sumsq": 1024}  # csrc/optim.hip:198, 322, 242 / 256, 295


def flat_plan(n, cap):
    """The flat kernels of csrc/optim.hip (adamw :196-199 and :20-49, cast :240-243, sumsq :293-297, clip_scale :320-323): float4 index i
    of n4 = n / 4 goes to thread i % (256 grid) in round i / (256 grid); the n % 4 last floats to workgroup 0's scalar tail."""
    n4 = n // 4
    grid = max(1, min(_cdiv(n4, 256), cap))
    per_round = 256 * grid
    return FlatPlan(grid, n4, n4 // per_round, n4 % per_round, n % 4, _cdiv(n4, per_round))


def flat_regime(n, cap):
    """One word for the regime a size exercises (the CPU file asserts every word appears in each table)."""
    p = flat_plan(n, cap)
    if n < 4:
        return "scalar only"
    if p.grid < cap:
        return "below cap"
    if p.full_rounds == 1 and p.ragged == 0:
        return "at cap"
    if p.full_rounds == 1 and p.ragged <= 4:
        return "cap + 1"
    if p.full_rounds >= 2 and p.ragged:
        return "rounds + ragged"
    return "past cap"


def sumsq_ws_floats(n):
    return flat_plan(n, FLAT_CAPS["sumsq"]).grid  # csrc/optim.hip:310


def sumsq_det_plan(n):
    return det_reduce_plan(flat_plan(n, FLAT_CAPS["sumsq"]).grid, 1, 1, 1, 0, 1)  # csrc/optim.hip:306


GridStridePlan = namedtuple("GridStridePlan", "threads grid full_rounds ragged")
GATHER_CAP = IM2COL_CAP = 8192  # csrc/tokenizer.hip:305, 317


def gather_plan(B, N, Nk, D):
    """csrc/tokenizer.hip:303-305 and :287-288: one thread per float4 of the KEPT rows."""
    total = B * Nk * (D // 4)
    grid = min(_cdiv(total, 256), GATHER_CAP)
    return GridStridePlan(total, grid, total // (256 * grid), total % (256 * grid))


def im2col_plan(B, C, H, W, P):
    """csrc/tokenizer.hip:315-317 and :26-31: one thread per 4 pixels of the full patches of the gathered image."""
    total = B * C * ((H // P) * P) * ((W // P) * P // 4)
    grid = min(_cdiv(total, 256), IM2COL_CAP)
    return GridStridePlan(total, grid, total // (256 * grid), total % (256 * grid))


def stride_regime(p, cap):
    if p.grid < cap:
        return "below cap"
    if p.full_rounds == 1 and p.ragged == 0:
        return "at cap"
    if p.full_rounds == 1 and p.ragged <= 4:
        return "cap + 1"
    if p.full_rounds >= 2 and p.ragged:
        return "rounds + ragged"
    return "past cap"


PatchPlan = namedtuple("PatchPlan", "grid_x grid_y bpar idle_threads ragged_block batches_max batches_min det_dE det_dpos ws_floats")
PB_IT = 2  # csrc/tokenizer.hip:58


def patch_bwd_plan(B, C, n, D):
    """csrc/tokenizer.hip:332-334 and :84-94: grid (ceil(n / 2), C + 1); a workgroup holds bpar = 256 / (D / 4) batch lanes of D / 4
    threads (the rest idle), lane bsub takes batches bsub, bsub + bpar, ...; the last position block is ragged when n is odd.  The two
    det_reduce launches of :342-343."""
    nv = D // 4
    bpar = 256 // nv
    gx = _cdiv(n, PB_IT)
    lanes = [len(range(s, B, bpar)) for s in range(bpar)]
    nE, nP = gx * bpar * C * D, C * bpar * n * D
    return PatchPlan(gx, C + 1, bpar, 256 - bpar * nv, n % PB_IT != 0, max(lanes), min(lanes),
                     det_reduce_plan(gx * bpar, C * D, D, D, 0, C * D), det_reduce_plan(C * bpar, n * D, D, D, 0, n * D), nE + nP)


OrthoPlan = namedtuple("OrthoPlan", "grid_x grid_y ragged_chunk det ws_floats")
ORTHO_CHUNK = 28  # csrc/tokenizer.hip:135


def ortho_plan(B, C, n, D):
    """csrc/tokenizer.hip:367-376: grid (ceil(n / 28), B C); one part of B C D + B C floats per token chunk."""
    gx = _cdiv(n, ORTHO_CHUNK)
    nS, nQ = B * C * D, B * C
    return OrthoPlan(gx, B * C, n % ORTHO_CHUNK != 0, det_reduce_plan(gx, nS, D, D, nQ, nS + nQ), gx * (nS + nQ))


# =====================================================================================================================================
# Case tables (imported by test_stream_kernels_cpu.py, which asserts that every regime is present)
# =====================================================================================================================================
LnCase = namedtuple("LnCase", "M D du_f32 dx_in misaligned")  # dx_in: "given" | "none" | "alias"; misaligned: dgamma / dbeta one float off 16 bytes
LN_CASES = [
    LnCase(20, 384, False, "given", True),        # 5 workgroups: flat det_reduce, no unrolled round, scalar form
    LnCase(20, 192, True, "none", False),         # ... vector form
    LnCase(100, 768, True, "alias", True),        # 25 parts: flat, unrolled, scalar
    LnCase(100, 4, False, "given", False),        # ... vector; D = 4: one float4 per row
    LnCase(1001, 192, False, "none", True),       # 251 parts: tall, remainder loop only, scalar; three waves of the last workgroup have no row
    LnCase(1000, 516, True, "given", False),      # ... vector; D = 516: 129 float4 (the four-register kernel with two idle registers)
    LnCase(3000, 384, True, "given", False),      # 750 parts: tall, one unrolled round AND a remainder after it
    LnCase(4096, 384, False, "alias", False),     # ln_bwd exactly at its cap: one row per wave, no pair
    LnCase(4097, 1024, True, "given", False),     # cap + 1: one wave runs one pair
    LnCase(8192, 516, False, "none", False),      # every wave one pair, no single row
    LnCase(8193, 4, True, "alias", True),         # one wave a pair and a single row
    LnCase(12293, 768, False, "given", True),     # waves with two pairs beside waves with one pair + a single row; tall unrolled scalar
    LnCase(16384, 192, True, "none", False),      # ln_fwd exactly at its cap
    LnCase(16385, 384, False, "given", False),    # ln_fwd cap + 1
    LnCase(40001, 516, True, "alias", False),     # ln_fwd: two full rounds and a ragged one
    LnCase(HEADLINE_M, 384, False, "given", False),  # the headline launch: 12 pairs, 2112 waves with a trailing row
    LnCase(HEADLINE_M, 768, True, "none", True),
]
LN_STRIDED = [(64, 384, 1569 * 384), (5000, 384, 388), (4100, 1024, 1028)]  # (M, D, row stride): the final norm over the CLS rows; padded rows

ADAMW_N = [1, 3, 5, 6, 1000, 4 * 256 * 4096, 4 * 256 * 4096 + 4 + 2, 2 * 4194304 + 4 * 777 + 3, ARENA_FLOATS]
CAST_N = [2, 1001, 4 * 256 * 8192, 4 * 256 * 8192 + 4 + 3, 8388608 + 4 * 333 + 2, 2 * 8388608 + 4 * 333 + 1, ARENA_FLOATS + 3]
SUMSQ_N = [1, 2, 3, 4096 + 2, 4 * 256 * 1024, 4 * 256 * 1024 + 4 + 1, 2 * 1048576 + 4 * 555 + 3, 3_400_000, 16_000_000, ARENA_FLOATS]

GatherCase = namedtuple("GatherCase", "B N Nk D")
GATHER_CASES = [
    GatherCase(64, 1569, 785, 384),     # the headline token drop: two full rounds and a ragged one
    GatherCase(64, 600, 512, 256),      # exactly one round at the cap
    GatherCase(1, 233017, 233017, 36),  # cap + 1 float4 (2^21 + 1 = 9 x 233017); Nk == N
    GatherCase(3, 50, 1, 384),          # Nk = 1
    GatherCase(5, 33, 20, 4),           # D = 4
    GatherCase(2, 197, 197, 192),       # Nk == N below the cap
]

Im2colCase = namedtuple("Im2colCase", "B Ct C H W P u8")
IM2COL_CASES = [
    Im2colCase(64, 10, 8, 224, 224, 16, False),   # the headline tokeniser: three full rounds and a ragged one
    Im2colCase(64, 10, 8, 224, 224, 16, True),
    Im2colCase(64, 8, 8, 64, 256, 16, False),     # exactly one round at the cap
    Im2colCase(1, 3, 3, 4, 699052, 4, False),     # the first size past the cap that exists (the thread count is a multiple of 4): cap + 4 threads
    Im2colCase(2, 5, 3, 40, 48, 16, False),       # non-square, height not a multiple of P
    Im2colCase(2, 5, 3, 40, 48, 16, True),
]

PatchCase = namedtuple("PatchCase", "B C n D")
PATCH_CASES = [
    PatchCase(64, 8, 196, 384),   # headline: bpar 2, 32 batches per lane
    PatchCase(1, 3, 7, 384),      # bpar 2, B below it (one lane idle), odd n
    PatchCase(2, 2, 9, 384),      # B == bpar
    PatchCase(5, 2, 5, 384),      # B not a multiple of bpar
    PatchCase(3, 2, 9, 192),      # bpar 5, B below
    PatchCase(5, 1, 4, 192),      # B == bpar, even n
    PatchCase(7, 3, 11, 192),     # not a multiple
    PatchCase(1, 2, 3, 1024),     # bpar 1, B == bpar
    PatchCase(3, 2, 5, 516),      # bpar 1 (129 float4: 127 idle threads), B above
    PatchCase(64, 2, 6, 4),       # D = 4: bpar 256, B far below
]

OrthoCase = namedtuple("OrthoCase", "B C n D")
ORTHO_CASES = [OrthoCase(64, 8, 196, 384), OrthoCase(3, 5, 30, 384), OrthoCase(2, 1, 57, 192)]


def det_jobs():
    """Every det_reduce launch the tables above cause in deterministic mode: (what, DetPlan)."""
    jobs = [(f"ln_bwd M{c.M} D{c.D}", ln_bwd_det_plan(c.M, c.D, not c.misaligned)) for c in LN_CASES]
    jobs += [(f"sumsq n{n}", sumsq_det_plan(n)) for n in SUMSQ_N]
    for c in PATCH_CASES:
        p = patch_bwd_plan(*c)
        jobs += [(f"patch dE {tuple(c)}", p.det_dE), (f"patch dpos {tuple(c)}", p.det_dpos)]
    jobs += [(f"ortho {tuple(c)}", ortho_plan(*c).det) for c in ORTHO_CASES]
    return jobs


def case_bytes(kind, c):
    """Upper bound of the device memory a case's test holds at once, references included (asserted < 6 GB by the CPU file)."""
    if kind == "ln":  # fp32: x, dx_in, dx_out x 2, du, ref chunks; int32 du / terms; bf16 copies; float64 chunk temporaries (<= 2^22 elements each)
        return c.M * c.D * (4 * 8 + 2 * 4) + 12 * 8 * (1 << 22)
    if kind == "adamw":  # p, g, m, v, three clones, six float64 temporaries
        return c * (7 * 4 + 6 * 8)
    if kind == "cast":
        return c * (4 + 2 * 4 + 8)
    if kind == "sumsq":
        return c * (4 + 4 + 8) + 100003 * 4
    if kind == "gather":
        return (c.B * c.N * c.D * 3 + c.B * c.Nk * c.D * 3) * 8
    if kind == "im2col":
        return c.B * c.Ct * c.H * c.W * 4 + c.B * c.C * c.H * c.W * (2 * 2 + 3 * 4)
    if kind == "patch":
        T = c.C * c.n
        return c.B * (T + 1) * c.D * (4 + 8 + 8) + c.B * T * c.D * (4 + 2 + 8) + patch_bwd_plan(*c).ws_floats * 4
    if kind == "ortho":
        T = c.C * c.n
        return c.B * T * c.D * (4 + 4 + 8 * 6) + ortho_plan(*c).ws_floats * 4
    raise KeyError(kind)


# =====================================================================================================================================
# GPU tests
# =====================================================================================================================================
@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, device="cuda", generator=_gen(seed)) * scale


def _randint(lo, hi, shape, seed, dtype=torch.int32):
    return torch.randint(lo, hi + 1, shape, device="cuda", generator=_gen(seed), dtype=dtype)


def _row_chunks(M, D, budget=1 << 22):
    step = max(1, budget // D)
    for r0 in range(0, M, step):
        yield slice(r0, min(M, r0 + step))


def _within(got, ref64, rtol, atol, what):
    """|got - ref| <= atol + rtol |ref| element-wise against a float64 reference; NaN (an element never written) fails."""
    g = got.double()
    err = (g - ref64).abs()
    bad = ~(err <= atol + rtol * ref64.abs())
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements off; first at flat index {i}: got {g.flatten()[i].item()!r}, "
                             f"want {ref64.flatten()[i].item()!r}; max err {err[~err.isnan()].max().item() if (~err.isnan()).any() else float('nan'):.4g}")


def _untouched(t):
    """every element still holds the sentinel (compared in the tensor's own dtype)"""
    return bool((t == torch.tensor(SENT, dtype=t.dtype, device=t.device)).all())


def _explain_terms(diff, terms, name_of):
    """diff = got - want of one exact output element (in quanta), terms = the integer terms of its sum: names the rows whose single term
    explains the difference (a lost row has term == -diff, a row added twice term == diff)."""
    lost = (terms == -diff).nonzero().flatten()
    twice = (terms == diff).nonzero().flatten()
    return (f"difference {diff} quanta; rows whose term would explain it if LOST: {[name_of(int(i)) for i in lost[:6]]} ({lost.numel()} candidates); "
            f"if ADDED TWICE: {[name_of(int(i)) for i in twice[:6]]} ({twice.numel()} candidates)")


def _assert_exact(got, want64, what, explain=None):
    want = want64.to(got.dtype)
    assert torch.equal(want.double(), want64.double()), f"{what}: the reference itself is not representable in {got.dtype} (test bug)"
    if torch.equal(got, want):
        return
    bad = (got != want) | got.isnan()
    i = int(bad.flatten().nonzero()[0])
    msg = (f"{what}: {int(bad.sum())}/{bad.numel()} elements differ from the exact sum; first at flat index {i}: got {got.flatten()[i].item()!r}, "
           f"want {want.flatten()[i].item()!r}")
    if explain is not None:
        msg += "; " + explain(i, got.flatten()[i].double().item() - want64.flatten()[i].double().item())
    raise AssertionError(msg)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
def _ln_id(c):
    return f"M{c.M}-D{c.D}-{'f32' if c.du_f32 else 'bf16'}-{c.dx_in}{'-misaligned' if c.misaligned else ''}"


def _ln_bwd_call(hip, case, du, x, mean, rstd, gamma, dx_in, dg0, db0, scale=None, rows_per_sample=1):
    """One dcv_ln_bwd* call with sentinel-guarded dgamma / dbeta (offset by one float from 16 bytes when the case says so) and
    NaN-filled outputs.  Returns (dx_out, dx_bf16, dgamma, dbeta)."""
    M, D = case.M, case.D
    buf = torch.full((2 * D + 8,), SENT, device="cuda")
    off = 1 if case.misaligned else 4
    dg, db = buf[off:off + D], buf[off + D:off + 2 * D]
    assert (dg.data_ptr() % 16 != 0) == case.misaligned and (db.data_ptr() % 16 != 0) == case.misaligned
    dg.copy_(dg0)
    db.copy_(db0)
    if case.dx_in == "alias":
        dx_out = dx_in.clone()
        din = dx_out
    else:
        dx_out = torch.full((M, D), float("nan"), device="cuda")
        din = dx_in if case.dx_in == "given" else None
    dxb = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    kw = {} if scale is None else dict(bf16_row_scale=scale, rows_per_sample=rows_per_sample)
    hip.ln_bwd(du, x, mean, rstd, gamma, din, dx_out, dxb, dg, db, M, D, **kw)
    assert (buf[:off] == SENT).all() and (buf[off + 2 * D:] == SENT).all(), "ln_bwd wrote outside dgamma / dbeta"
    return dx_out, dxb, dg, db


@pytest.mark.parametrize("case", LN_CASES, ids=_ln_id)
def test_ln_bwd_exact_column_sums(hip, case, reduction_mode):
    """dgamma / dbeta on exact inputs: du integers in [-4, 4], x - mean integers in [-16, 16], rstd = 0.5 (mean and rstd are INPUTS of the
    backward), so a term of dgamma is a multiple of 0.5 of magnitude <= 32 and 100 416 rows sum to < 2^23 quanta in the worst case.  Both
    accumulate into non-zero integers.  torch.equal with the int64 sums in both reduction modes; the DropPath row scale changes nothing
    but the bf16 copy."""
    M, D = case.M, case.D
    plan = ln_bwd_plan(M)
    mean = _randint(-3, 3, (M,), seed=M + 1).float()
    xc = _randint(-16, 16, (M, D), seed=M + 2)
    x = xc.float() + mean[:, None]
    rstd = torch.full((M,), 0.5, device="cuda")
    du_i = _randint(-4, 4, (M, D), seed=M + 3)
    du = du_i.float() if case.du_f32 else du_i.to(torch.bfloat16)
    assert torch.equal(du.to(torch.int32), du_i)
    gamma = 1 + 0.1 * _randn(D, seed=4)
    dx_in = _randn(M, D, seed=M + 5) if case.dx_in != "none" else None
    dg0, db0 = _randint(-50, 50, (D,), seed=6).float(), _randint(-50, 50, (D,), seed=7).float()
    terms = du_i * xc  # int32, in quanta of 0.5: du * xhat = du * (x - mean) * 0.5
    # the exactness condition, worst case over the columns: sum of |terms| + |initial value| < 2^23 quanta
    assert int(terms.abs().sum(0, dtype=torch.int64).max()) + 2 * 50 < 2 ** 23
    assert int(du_i.abs().sum(0, dtype=torch.int64).max()) + 50 < 2 ** 23
    want_dg = (2 * dg0.double() + terms.sum(0, dtype=torch.int64).double()) / 2
    want_db = db0.double() + du_i.sum(0, dtype=torch.int64).double()
    dx, dxb, dg, db = _ln_bwd_call(hip, case, du, x, mean, rstd, gamma, dx_in, dg0, db0)

    def where(row):
        k = row // plan.stride
        return f"row {row} (iteration {k} of its wave: {'second' if k % 2 else 'first'} row of pair {k // 2}, or the trailing single row)"

    def explain(col_terms, diff):
        """single rows first; then whole rounds of the walk (rows k stride .. (k + 1) stride - 1: iteration k of every wave)"""
        pad = (-M) % plan.stride
        rounds = torch.nn.functional.pad(col_terms.long(), (0, pad)).view(-1, plan.stride).sum(1)
        lost, twice = (rounds == -diff).nonzero().flatten().tolist(), (rounds == diff).nonzero().flatten().tolist()
        swapped = [k for k in range(0, rounds.numel() - 1, 2) if int(rounds[k] - rounds[k + 1]) == diff]
        return (_explain_terms(diff, col_terms, where) + f"; whole iterations (of {rounds.numel()}) that explain it if lost: {lost}, if added twice: {twice}, "
                f"if the second row of pair k / 2 repeated the first: {swapped}; all pairs so: {int((rounds[0:-1:2] - rounds[1::2]).sum()) == diff}")

    tag = f"ln_bwd M={M} D={D} ({plan.grid} workgroups, wave classes (pairs, single) {sorted(plan.classes)}, det_reduce {ln_bwd_det_plan(M, D, not case.misaligned)})"
    _assert_exact(dg, want_dg, f"dgamma, {tag}", lambda c, d: f"column {c}: " + explain(terms[:, c], round(2 * d)))
    _assert_exact(db, want_db, f"dbeta, {tag}", lambda c, d: f"column {c}: " + explain(du_i[:, c], round(d)))
    assert torch.isfinite(dx).all() and torch.isfinite(dxb.float()).all()
    # DropPath's per-sample factor on the bf16 copy only
    rps = 1569 if M % 1569 == 0 else 1
    sc = torch.tensor([0.0, 1.25, 1.0, 1.25], device="cuda")[_randint(0, 3, (M // rps,), seed=8, dtype=torch.int64)]
    dx2, dxb2, dg2, db2 = _ln_bwd_call(hip, case, du, x, mean, rstd, gamma, dx_in, dg0, db0, scale=sc, rows_per_sample=rps)
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db), "the row scale changed dx_out / dgamma / dbeta"
    assert torch.equal(dxb2, (dx * sc.repeat_interleave(rps)[:, None]).to(torch.bfloat16)), "scaled bf16 copy"
    assert torch.equal(dxb, dx.to(torch.bfloat16))


@pytest.mark.parametrize("case", LN_CASES, ids=_ln_id)
def test_ln_fwd_bwd_per_element(hip, case):
    """Forward (fp32 and bf16 output, mean, rstd) and the backward's dx_out / dx_bf16 on random inputs with a row mean far from zero,
    against float64 of the same formulas on the kernel's own operands.  Bounds: test_layernorm's (1e-5 / 1e-5 fp32 output and mean,
    1e-4 / 1e-4 dx, 1e-2 / 1e-2 bf16 dx), test_gemm_nt_resid_ln's for rstd (2e-6 / 1e-7); the bf16 output within one bf16 ulp,
    2^-8 |ref| + 2e-5 (half an ulp of rounding plus the fp32 output's bound)."""
    M, D = case.M, case.D
    x = _randn(M, D, seed=M + 11, scale=3.0) + 5.0
    gamma, beta = 1 + 0.1 * _randn(D, seed=12), 0.1 * _randn(D, seed=13)
    u = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    uf = torch.full((M, D), float("nan"), device="cuda")
    mean, rstd = torch.full((M,), float("nan"), device="cuda"), torch.full((M,), float("nan"), device="cuda")
    hip.ln_fwd(x, gamma, beta, u, mean, rstd, M, D, 1e-6)
    hip.ln_fwd(x, gamma, beta, uf, None, None, M, D, 1e-6)
    du = _randn(M, D, seed=M + 14)
    du = du if case.du_f32 else du.to(torch.bfloat16)
    dx_in = _randn(M, D, seed=M + 15) if case.dx_in != "none" else None
    dx, dxb, _, _ = _ln_bwd_call(hip, case, du, x, mean, rstd, gamma, dx_in, torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda"))
    g64 = gamma.double()
    tag = f"M={M} D={D} (ln_fwd {ln_fwd_plan(M)}, ln_bwd classes {sorted(ln_bwd_plan(M).classes)})"
    for sl in _row_chunks(M, D):
        x64 = x[sl].double()
        mu = x64.mean(-1)
        rs = (((x64 - mu[:, None]) ** 2).mean(-1) + 1e-6).rsqrt()
        ref = (x64 - mu[:, None]) * rs[:, None] * g64 + beta.double()
        rows = f"rows {sl.start}..{sl.stop - 1}, {tag}"
        _within(mean[sl], mu, 1e-5, 1e-5, f"mean, {rows}")
        _within(rstd[sl], rs, 2e-6, 1e-7, f"rstd, {rows}")
        _within(uf[sl], ref, 1e-5, 1e-5, f"fp32 output, {rows}")
        _within(u[sl], ref, 2.0 ** -8, 2e-5, f"bf16 output, {rows}")
        # backward from the kernel's own statistics
        xh = (x64 - mean[sl].double()[:, None]) * rstd[sl].double()[:, None]
        gg = du[sl].double() * g64
        m1, m2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
        dref = rstd[sl].double()[:, None] * (gg - m1 - xh * m2) + (dx_in[sl].double() if dx_in is not None else 0.0)
        _within(dx[sl], dref, 1e-4, 1e-4, f"dx_out, {rows}")
        _within(dxb[sl], dref, 1e-2, 1e-2, f"dx_bf16, {rows}")


@pytest.mark.parametrize("M,D,stride", LN_STRIDED)
def test_ln_strided_rows(hip, M, D, stride, reduction_mode):
    """x_row_stride / dx_row_stride as the final norm uses them (M = B rows, N D apart) and a padded stride D + 4: bit-identical to the same
    rows run contiguously; the gaps hold NaN on the input side (never read into a result) and a sentinel on the output side (never written)."""
    xs = torch.full((M * stride,), float("nan"), device="cuda")
    xrows = xs.view(M, stride)[:, :D]
    xc = _randn(M, D, seed=21, scale=2.0) + 1.0
    xrows.copy_(xc)
    gamma, beta = 1 + 0.1 * _randn(D, seed=22), 0.1 * _randn(D, seed=23)
    outs = []
    for xin, st in ((xc, None), (xs, stride)):
        u = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device="cuda")
        uf = torch.full((M, D), float("nan"), device="cuda")
        mean, rstd = torch.full((M,), float("nan"), device="cuda"), torch.full((M,), float("nan"), device="cuda")
        hip.ln_fwd(xin, gamma, beta, u, mean, rstd, M, D, 1e-6, x_row_stride=st)
        hip.ln_fwd(xin, gamma, beta, uf, None, None, M, D, 1e-6, x_row_stride=st)
        outs.append((u, uf, mean, rstd))
    for a, b, nm in zip(outs[0], outs[1], ("bf16 output", "fp32 output", "mean", "rstd")):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), f"ln_fwd {nm}: strided rows differ from contiguous rows"
    mean, rstd = outs[0][2], outs[0][3]
    du = _randn(M, D, seed=24).to(torch.bfloat16)
    dinc = _randn(M, D, seed=25)
    dins = torch.full((M * stride,), float("nan"), device="cuda")
    dins.view(M, stride)[:, :D].copy_(dinc)
    res = []
    for xin, din, st in ((xc, dinc, None), (xs, dins, stride)):
        for alias in (False, True):
            if alias:
                dout = din.clone()
                dout[dout.isnan()] = SENT
                din_arg = dout
            else:
                dout = torch.full((M * (st or D),), SENT, device="cuda")
                din_arg = din
            dxb = torch.full((M, D), float("nan"), dtype=torch.bfloat16, device="cuda")
            dg, db = torch.ones(D, device="cuda"), torch.ones(D, device="cuda")
            hip.ln_bwd(du, xin, mean, rstd, gamma, din_arg, dout, dxb, dg, db, M, D, x_row_stride=st, dx_row_stride=st)
            full = dout.view(M, st or D)
            assert (full[:, D:] == SENT).all(), "ln_bwd wrote between the rows of dx_out"
            res.append((full[:, :D].clone(), dxb, dg, db))
    for r in res[1:]:
        for a, b, nm in zip(res[0], r, ("dx_out", "dx_bf16", "dgamma", "dbeta")):
            if nm in ("dgamma", "dbeta") and reduction_mode != "det":
                continue  # random inputs: the atomic form's column sums depend on the order (the exact test above covers them)
            assert torch.isfinite(a.float()).all() and torch.equal(a, b), f"ln_bwd {nm}: strided / in-place form differs from the contiguous one"


def test_ln_refusals(hip, monkeypatch):
    """D % 4, D > 1024, a row stride that is not a multiple of 4 and a workspace that is too small are refused (include/dcv.h) - with real
    tensors large enough for the call, so a missing refusal is a failed assertion and not a fault."""
    M = 64
    for D, stride in ((6, 8), (1028, 1028), (384, 386)):
        big = max(D, stride, 1028)
        x = torch.zeros(M * big, device="cuda")
        g = torch.ones(big, device="cuda")
        out = torch.zeros(M * big, device="cuda")
        st = torch.zeros(M, device="cuda")
        with pytest.raises(RuntimeError):
            hip.ln_fwd(x, g, g, out, st, st, M, D, 1e-6, x_row_stride=stride)
        with pytest.raises(RuntimeError):
            hip.ln_bwd(x, x, st, st, g, None, out, None, g.clone(), g.clone(), M, D, x_row_stride=stride)
        if stride != D:
            with pytest.raises(RuntimeError):
                hip.ln_bwd(x, x, st, st, g, None, out, None, g.clone(), g.clone(), M, D, dx_row_stride=stride)
    old = hip.set_deterministic(True)
    try:
        M, D = 5000, 384
        need = ln_bwd_ws_floats(M, D)
        ws = torch.zeros(need, device="cuda")
        monkeypatch.setattr(hip, "_workspace", lambda n, like: ws[:need - 4])  # memory for the whole call, size reported 4 floats short
        x = torch.zeros(M, D, device="cuda")
        st = torch.ones(M, device="cuda")
        with pytest.raises(RuntimeError):
            hip.ln_bwd(x, x, st, st, torch.ones(D, device="cuda"), None, torch.zeros(M, D, device="cuda"), None, torch.zeros(D, device="cuda"),
                       torch.zeros(D, device="cuda"), M, D)
    finally:
        hip.set_deterministic(old)


# ---- gradient norm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_exact(hip, n, reduction_mode):
    """dcv_sumsq_acc(_det) on x in {-1, 0, 1}: the sum of squares is the count of non-zeros, an integer below 2^23 (the density is chosen so),
    added to a non-zero *acc, and a second buffer on top as clip_grad_norm_ does.  Exact in both modes."""
    plan = flat_plan(n, FLAT_CAPS["sumsq"])
    dens = min(0.6, 3.0e6 / n)
    x = _randint(-1, 1, (n,), seed=n % 1000 + 31).float() * (torch.rand(n, device="cuda", generator=_gen(32)) < dens)
    n2 = 100003
    x2 = _randint(-1, 1, (n2,), seed=33).float()
    c1, c2 = int(x.abs().sum(dtype=torch.float64)), int(x2.abs().sum(dtype=torch.float64))
    assert 1000 + c1 + c2 < 2 ** 23  # the exactness condition (quantum 1)
    acc = torch.full((1,), 1000.0, device="cuda")
    hip.sumsq_acc(x, n, acc)
    tag = (f"n={n}: {plan.grid} workgroups, {plan.full_rounds} full rounds + {plan.ragged} float4 in a ragged one, scalar tail {plan.tail}, "
           f"det_reduce {sumsq_det_plan(n)}")
    got = acc.item()
    assert got == 1000.0 + c1, f"sumsq_acc {tag}: got {got}, want {1000.0 + c1} (difference {got - 1000.0 - c1}; one workgroup's round holds 1024 floats, ~{1024 * dens:.0f} non-zeros)"
    hip.sumsq_acc(x2, n2, acc)
    p2 = flat_plan(n2, FLAT_CAPS["sumsq"])
    assert acc.item() == 1000.0 + c1 + c2, (f"second buffer (n={n2}: {p2.grid} workgroups, {p2.full_rounds} full rounds + {p2.ragged} float4, scalar tail {p2.tail}) on top of "
                                            f"the first: got {acc.item()}, want {1000.0 + c1 + c2}")


def test_sumsq_refusals(hip, monkeypatch):
    n = 3_000_000
    x = torch.ones(n + 4, device="cuda")
    acc = torch.zeros(1, device="cuda")
    with pytest.raises(RuntimeError):
        hip.sumsq_acc(x[1:], n, acc)  # misaligned x
    with pytest.raises(RuntimeError):
        hip.sumsq_acc(x, 0, acc)
    old = hip.set_deterministic(True)
    try:
        ws = torch.zeros(sumsq_ws_floats(n), device="cuda")
        monkeypatch.setattr(hip, "_workspace", lambda k, like: ws[:ws.numel() - 1])
        with pytest.raises(RuntimeError):
            hip.sumsq_acc(x, n, acc)
    finally:
        hip.set_deterministic(old)
    assert acc.item() == 0.0


def _clip_coef_bound(n):
    """Relative error bound of the norm computed by dcv_sumsq_acc: all terms are positive, so each fp32 addition adds at most 2^-24 relative:
    a thread adds 4 squares per round sequentially, then 8 tree levels in the workgroup, then at most 16 + 64 additions in the reduction
    across workgroups (or 1024 atomics, of which a value passes at most 1024); the square itself one more.  The square root halves it."""
    k = 4 * flat_plan(n, FLAT_CAPS["sumsq"]).iters_max + 3 + 1 + 8 + 1024
    return 0.5 * k * 2.0 ** -24


@pytest.mark.parametrize("n", ADAMW_N)
def test_clip_scale(hip, n):
    """coefficient >= 1 (far above, and exactly 1) leaves x bit-identical; below 1 every element is x max_norm / (sqrt(sumsq) + 1e-6) within
    8 x 2^-24 relative (sqrt, add, divide, multiply: four fp32 roundings, doubled)."""
    x0 = _randn(n, seed=41)
    ss = x0.double().pow(2).sum().float().reshape(1)
    norm32 = np.float32(np.sqrt(np.float32(ss.item())))
    exactly_one = float(np.float32(norm32 + np.float32(1e-6)))
    for max_norm in (1e6 * float(norm32) + 1.0, exactly_one):
        x = x0.clone()
        hip.clip_scale(x, n, ss, max_norm)
        assert torch.equal(x, x0), f"clip_scale n={n} max_norm={max_norm}: coefficient >= 1 changed x"
    full = torch.full((n + 8,), SENT, device="cuda")
    x = full[4:4 + n]
    x.copy_(x0)
    max_norm = float(np.float32(0.37 * float(norm32)))
    hip.clip_scale(x, n, ss, max_norm)
    ref = x0.double() * max_norm / (math.sqrt(float(ss.item())) + 1e-6)
    _within(x, ref, 8 * 2.0 ** -24, 0.0, f"clip_scale n={n} ({flat_plan(n, FLAT_CAPS['clip_scale'])})")
    assert (full[:4] == SENT).all() and (full[4 + n:] == SENT).all()


def test_clip_pair_against_torch(hip, reduction_mode):
    """dcv_sumsq_acc over three buffers + dcv_clip_scale on each, against torch.nn.utils.clip_grad_norm_ in float64."""
    sizes = [2 * 4194304 + 4 * 777 + 3, 100003, 5]
    bufs = [_randn(n, seed=50 + i, scale=0.3 * (i + 1)) for i, n in enumerate(sizes)]
    params = [torch.nn.Parameter(torch.zeros(n, dtype=torch.float64, device="cuda")) for n in sizes]
    for p, b in zip(params, bufs):
        p.grad = b.double()
    max_norm = 3.0
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    assert total.item() > max_norm
    acc = torch.zeros(1, device="cuda")
    for b, n in zip(bufs, sizes):
        hip.sumsq_acc(b, n, acc)
    bound = _clip_coef_bound(max(sizes))
    assert abs(math.sqrt(acc.item()) - total.item()) <= (bound + 2.0 ** -24) * total.item(), (acc.item(), total.item() ** 2)
    for b, n, p in zip(bufs, sizes, params):
        hip.clip_scale(b, n, acc, max_norm)
        _within(b, p.grad, 8 * 2.0 ** -24 + bound, 0.0, f"clipped gradient, n={n}")


def test_clip_scale_refusals(hip):
    n = 5000
    x = torch.ones(n + 4, device="cuda")
    ss = torch.full((1,), 1e12, device="cuda")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError):
            hip.clip_scale(x, n, ss, bad)
    with pytest.raises(RuntimeError):
        hip.clip_scale(x[1:], n, ss, 1.0)
    assert (x == 1).all()


# ---- AdamW --------------------------------------------------------------------------------------------------------------------------
LR, B1, B2, EPS, WD, GS = 0.1, 0.9, 0.999, 1e-8, 0.04, 0.5


def _hyper_f32(lr, b1, b2, eps, wd, step, gs):
    """The eight fp32 values of include/dcv.h: bias corrections in double from the fp32 betas, then rounded."""
    f = np.float32
    bc1, bc2 = 1.0 - float(f(b1)) ** step, 1.0 - float(f(b2)) ** step
    return np.array([f(lr), f(b1), f(b2), f(eps), f(wd), f(1.0 / bc1), f(1.0 / math.sqrt(bc2)), f(gs)], dtype=np.float32)


def _adamw_ref64(p, g, m, v, h):
    """csrc/optim.hip's formula in float64 on the kernel's fp32 operands and fp32 scalars."""
    lr, b1, b2, eps, wd, ibc1, isbc2, gs = (float(t) for t in h)
    f = np.float32
    decay, step = float(f(1.0) - f(h[0] * h[4])), float(f(h[0] * h[5]))  # the kernel's two derived scalars, rounded to fp32 as it rounds them (:21)
    gr = g.double() * gs
    m64 = b1 * m.double() + (1.0 - b1) * gr
    v64 = b2 * v.double() + (1.0 - b2) * gr * gr
    p64 = p.double() * decay - step * m64 / (v64.sqrt() * isbc2 + eps)
    return p64, m64, v64


@pytest.mark.parametrize("n", ADAMW_N)
def test_adamw_against_float64(hip, n):
    """p, m AND v after steps 1, 2, 3 and 1000, each step against float64 from the state the kernel itself left, with lr = 0.1 (the update
    is as large as the parameter, so an element that was skipped or updated twice is off by ~0.1, far outside 1e-6 |p| + 1e-7) and
    grad_scale = 0.5.  Elements next to the range keep their sentinel.

    Where the decayed parameter and the update cancel, 1e-7 absolute is a few fp32 roundings of quantities of size 0.5, so the reference
    takes the kernel's two derived scalars (1 - lr wd and lr / bc1) as the kernel rounds them, and p is drawn at the update's own size
    (0.3): with the double-precision scalars and p ~ N(0, 1) one element of 4.2 M missed the bound at step 1000 by 3 %.

    m is held to v's bound (1e-4 relative, 1e-12 absolute).  A bound relative to the RESULT only holds for a sum of terms of one sign, which v
    always is and m is when an element's gradient keeps its sign, so the gradients of these four steps are sign_e |g|: with independent signs
    b1 m + (1 - b1) g cancels and 1472 of 21.6 M elements of a correct fp32 kernel missed that bound at step 2 (worst error 1.5e-8 = half an
    ulp of the terms, on results near 1e-6).  A fifth step with an independent-sign gradient then checks m against the bound that follows from
    the arithmetic - three fp32 roundings of quantities no larger than |b1 m| + |(1 - b1) g| - and p and v as before."""
    plan = flat_plan(n, FLAT_CAPS["adamw"])
    full = [torch.full((n + 8,), SENT, device="cuda") for _ in range(4)]
    p, g, m, v = (t[4:4 + n] for t in full)
    p.copy_(_randn(n, seed=61, scale=0.3))
    m.zero_()
    v.zero_()
    sign = torch.where(_randn(n, seed=60) < 0, -1.0, 1.0)
    for step in (1, 2, 3, 1000, 4):
        g.copy_(_randn(n, seed=62 + step, scale=0.7))
        if step != 4:
            g.copy_(g.abs() * sign)
        h = _hyper_f32(LR, B1, B2, EPS, WD, step, GS)
        rp, rm, rv = _adamw_ref64(p, g, m, v, h)
        terms = float(h[1]) * m.double().abs() + (1.0 - float(h[1])) * (g.double() * float(h[7])).abs()
        hip.adamw(p, g, m, v, n, LR, B1, B2, EPS, WD, step, GS)
        tag = f"n={n} step {step} ({plan.grid} workgroups, {plan.full_rounds} full rounds + {plan.ragged} float4 ragged, scalar tail {plan.tail})"
        _within(p, rp, 1e-6, 1e-7, f"adamw p, {tag}")
        if step != 4:
            _within(m, rm, 1e-4, 1e-12, f"adamw m, {tag}")
        else:
            bad = ~((m.double() - rm).abs() <= 3 * 2.0 ** -24 * terms + 1e-12)
            assert not bad.any(), f"adamw m (independent signs), {tag}: {int(bad.sum())} elements off"
        _within(v, rv, 1e-4, 1e-12, f"adamw v, {tag}")
        del rp, rm, rv, terms
    for t in full:
        assert (t[:4] == SENT).all() and (t[4 + n:] == SENT).all(), "adamw wrote outside its range"


def test_adamw_set_hyper_and_dyn(hip):
    """dcv_adamw_set_hyper writes exactly the eight fp32 values of the header's double-precision formulas; dcv_adamw_dyn with them is
    bit-identical to dcv_adamw with the same scalars, on a slice of a larger buffer at a 16-byte offset; rewriting the block between two
    calls changes the second call only."""
    for step in (1, 2, 7, 1000, 100000):
        hyper = torch.full((8,), float("nan"), device="cuda")
        hip.adamw_set_hyper(hyper, 4.9e-5, B1, B2, EPS, WD, step, GS)
        assert np.array_equal(hyper.cpu().numpy(), _hyper_f32(4.9e-5, B1, B2, EPS, WD, step, GS)), step
    for n in (5, 2 * 4194304 + 4 * 777 + 3):
        state0 = [_randn(n, seed=71), _randn(n, seed=72, scale=0.3), _randn(n, seed=73, scale=0.1), _randn(n, seed=74).abs() * 0.01]
        ref = [t.clone() for t in state0]
        full = [torch.full((n + 12,), SENT, device="cuda") for _ in range(4)]
        dyn = [t[4:4 + n] for t in full]
        for d, s in zip(dyn, state0):
            d.copy_(s)
        hyper = torch.full((8,), float("nan"), device="cuda")
        hip.adamw_set_hyper(hyper, LR, B1, B2, EPS, WD, 1, GS)
        hip.adamw_dyn(*dyn, n, hyper)
        after1 = [d.clone() for d in dyn]
        hip.adamw_set_hyper(hyper, 0.05, B1, B2, EPS, 0.0, 2, 1.0)  # rewritten AFTER the first call was queued
        hip.adamw_dyn(*dyn, n, hyper)
        hip.adamw(*ref, n, LR, B1, B2, EPS, WD, 1, GS)
        for a, b, nm in zip(after1, ref, "pgmv"):
            assert torch.equal(a, b), f"adamw_dyn vs adamw, first call, {nm}, n={n}"
        hip.adamw(*ref, n, 0.05, B1, B2, EPS, 0.0, 2, 1.0)
        for a, b, nm in zip(dyn, ref, "pgmv"):
            assert torch.equal(a, b), f"adamw_dyn vs adamw, second call, {nm}, n={n}"
        for t in full:
            assert (t[:4] == SENT).all() and (t[4 + n:] == SENT).all()


def test_adamw_refusals(hip):
    n = 5000
    t = [torch.ones(n + 4, device="cuda") for _ in range(4)]
    hyper = torch.zeros(8, device="cuda")
    for k in range(4):  # each of p, g, m, v one float off a 16-byte boundary
        args = [x[1:1 + n] if i == k else x[:n] for i, x in enumerate(t)]
        with pytest.raises(RuntimeError):
            hip.adamw(*args, n, LR, B1, B2, EPS, WD, 1, 1.0)
        with pytest.raises(RuntimeError):
            hip.adamw_dyn(*args, n, hyper)
    for step in (0, -3):
        with pytest.raises(RuntimeError):
            hip.adamw(*(x[:n] for x in t), n, LR, B1, B2, EPS, WD, step, 1.0)
        with pytest.raises(RuntimeError):
            hip.adamw_set_hyper(hyper, LR, B1, B2, EPS, WD, step, 1.0)
    with pytest.raises(RuntimeError):
        hip.adamw(*(x[:n] for x in t), 0, LR, B1, B2, EPS, WD, 1, 1.0)
    assert all((x == 1).all() for x in t) and (hyper == 0).all()


# ---- casts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CAST_N)
def test_casts_bit_exact(hip, n):
    """dcv_cast_bf16 against .to(bfloat16) and dcv_cast_bf16_sr against the header's integer definition (element index = offset from src),
    bit for bit; the bf16 elements after the range keep their sentinel."""
    from test_kernels_gpu import _sr_bf16_numpy
    src = _randn(n, seed=81, scale=0.03)
    full = torch.full((n + 8,), SENT, dtype=torch.bfloat16, device="cuda")
    dst = full[:n]
    hip.cast_bf16(src, dst, n)
    tag = f"n={n} ({flat_plan(n, FLAT_CAPS['cast_bf16'])})"
    assert torch.equal(dst, src.to(torch.bfloat16)), f"cast_bf16 {tag}"
    assert _untouched(full[n:])
    full.fill_(SENT)
    seed = 12345
    sd = torch.tensor([seed], dtype=torch.int32, device="cuda")
    hip.cast_bf16_sr(src, dst, n, sd)
    got = dst.view(torch.int16).cpu().numpy().view(np.uint16)
    want = _sr_bf16_numpy(src.cpu().numpy(), np.arange(n), seed)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"cast_bf16_sr {tag}: {bad.size} elements differ, first at {bad[:4]}"
    assert _untouched(full[n:])


# ---- token gather / scatter, CLS fill ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GATHER_CASES, ids=lambda c: f"B{c.B}-N{c.N}-Nk{c.Nk}-D{c.D}")
def test_gather_tokens(hip, case):
    """Gather and scatter bit-exact against torch indexing with an unsorted idx; scatter into zeros leaves the other rows zero; scatter after
    gather restores the kept rows; <gather(x), y> == <x, scatter(y)> exactly on integer data."""
    B, N, Nk, D = case
    idx = torch.randperm(N, device="cuda", generator=_gen(91))[:Nk]
    if Nk > 2:
        assert not torch.equal(idx, idx.sort().values)
    idx32 = idx.to(torch.int32)
    x = _randint(-8, 8, (B, N, D), seed=92).float() + 0.25 * _randint(0, 3, (B, N, D), seed=93).float()
    y = _randint(-8, 8, (B, Nk, D), seed=94).float()
    gx = torch.full((B, Nk, D), float("nan"), device="cuda")
    hip.gather_tokens(x, idx32, gx, B, N, Nk, D)
    tag = f"{tuple(case)} ({gather_plan(*case)})"
    assert torch.equal(gx, x[:, idx]), f"gather {tag}"
    sy = torch.zeros(B, N, D, device="cuda")
    hip.gather_tokens(y, idx32, sy, B, N, Nk, D, scatter=True)
    want = torch.zeros(B, N, D, device="cuda")
    want[:, idx] = y
    assert torch.equal(sy, want), f"scatter {tag}"
    back = torch.zeros(B, N, D, device="cuda")
    hip.gather_tokens(gx, idx32, back, B, N, Nk, D, scatter=True)
    assert torch.equal(back[:, idx], x[:, idx])
    kept = torch.zeros(N, dtype=torch.bool, device="cuda")
    kept[idx] = True
    assert (back[:, ~kept] == 0).all()
    xi = x.round()
    gi = torch.empty(B, Nk, D, device="cuda")
    hip.gather_tokens(xi, idx32, gi, B, N, Nk, D)
    assert (gi.double() * y.double()).sum().item() == (xi.double() * sy.double()).sum().item(), f"adjoint identity {tag}"


def test_gather_refusals(hip):
    B, N, D = 2, 40, 8
    x, out = torch.ones(B, 2 * N, D, device="cuda"), torch.zeros(B, 2 * N, D, device="cuda")
    idx = torch.arange(2 * N, dtype=torch.int32, device="cuda") % N
    with pytest.raises(RuntimeError):
        hip.gather_tokens(x, idx, out, B, N, N + 1, D)  # Nk > N
    with pytest.raises(RuntimeError):
        hip.gather_tokens(x, idx, out, B, N, N, 6)      # D % 4
    with pytest.raises(RuntimeError):
        hip.gather_tokens(x, idx, out, B, N, 0, D)
    assert (out == 0).all()


@pytest.mark.parametrize("B,N,D,dense", [(64, 1569, 384, False), (7, 5, 36, False), (3, 1, 516, True), (5, 3, 100, False)])
def test_fill_cls(hip, B, N, D, dense):
    """Rows b * batch_stride hold cls + pos0 bit for bit, everything else its sentinel; B D not a multiple of 256; batch_stride N D and D."""
    cls, pos0 = _randn(D, seed=95), _randn(D, seed=96)
    x = torch.full((B, N, D), SENT, device="cuda")
    hip.fill_cls(x, cls, pos0, B, D if dense else N * D, D)
    assert torch.equal(x[:, 0], (cls + pos0).expand(B, D))
    assert (x[:, 1:] == SENT).all()


# ---- tokeniser ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IM2COL_CASES, ids=lambda c: f"B{c.B}-C{c.C}of{c.Ct}-{c.H}x{c.W}-P{c.P}-{'u8' if c.u8 else 'f32'}")
def test_im2col(hip, case):
    """Bit-exact (fp32 input) or at test_im2col's bound (uint8 with the affine) against oracle.unfold_patches of the gathered channels."""
    from oracle import dichavit_oracle as orc
    B, Ct, C, H, W, P, u8 = case
    idx = torch.randperm(Ct, device="cuda", generator=_gen(101))[:C]
    n = (H // P) * (W // P)
    out = torch.full((B * C * n, P * P), float("nan"), dtype=torch.bfloat16, device="cuda")
    tag = f"{tuple(case)} ({im2col_plan(B, C, H, W, P)})"
    if u8:
        raw = torch.randint(0, 256, (B, Ct, H, W), dtype=torch.uint8, device="cuda", generator=_gen(102))
        scale, shift = 0.02 + 0.01 * torch.rand(C, device="cuda", generator=_gen(103)), _randn(C, seed=104)
        hip.im2col(raw, idx.to(torch.int32), out, B, Ct, C, H, W, P, scale=scale, shift=shift)
        xn = raw[:, idx].double() * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
        ref = orc.unfold_patches(xn, P).reshape(-1, P * P)
        err = (out.double() - ref).abs().max().item()
        assert err <= 1e-2 * ref.abs().max().item(), f"im2col u8 {tag}: {err}"
        _within(out, ref, 2.0 ** -8, 1e-6, f"im2col u8, per element, {tag}")  # one bf16 rounding of an fp32 multiply-add
    else:
        x = _randn(B, Ct, H, W, seed=105)
        hip.im2col(x, idx.to(torch.int32), out, B, Ct, C, H, W, P)
        ref = orc.unfold_patches(x[:, idx], P).reshape(-1, P * P).to(torch.bfloat16)
        assert torch.equal(out, ref), f"im2col f32 {tag}"


def _patch_inputs(case):
    B, C, n, D = case
    T = C * n
    dx0 = _randint(-8, 8, (B, T + 1, D), seed=111)
    dYl = _randint(-8, 8, (B, T, D), seed=112)
    return dx0, dYl


@pytest.mark.parametrize("case", PATCH_CASES, ids=lambda c: f"B{c.B}-C{c.C}-n{c.n}-D{c.D}")
def test_patch_bwd_exact(hip, case, reduction_mode):
    """dE, dpos (row 0 and rows 1..n), dcls and the bf16 dY on integers in [-8, 8], accumulated into non-zero integers: exact in both modes."""
    B, C, n, D = case
    T = C * n
    plan = patch_bwd_plan(*case)
    dx0_i, dYl_i = _patch_inputs(case)
    dx0, dYl = dx0_i.float(), dYl_i.float()
    tok = dx0_i[:, 1:].reshape(B, C, n, D).long()
    assert 8 * B * max(n, C) + 100 < 2 ** 23  # the exactness condition: |term| <= 8, B n (dE) or B C (dpos) or B (dcls) terms, |initial| <= 100
    init = lambda shape, seed: _randint(-100, 100, shape, seed=seed).float()  # noqa: E731
    tag = f"{tuple(case)} ({plan})"
    for with_loss in (True, False):
        dE, dpos, dcls = init((C, D), 113), init((n + 1, D), 114), init((D,), 115)
        dE0, dpos0, dcls0 = dE.clone(), dpos.clone(), dcls.clone()
        dYb = torch.full((B * T, D), float("nan"), dtype=torch.bfloat16, device="cuda")
        hip.patch_bwd(dx0, dYl if with_loss else None, dYb, dE, dpos, dcls, B, C, n, D)
        want_dY = dx0_i[:, 1:].reshape(B * T, D) + (dYl_i.reshape(B * T, D) if with_loss else 0)
        assert torch.equal(dYb, want_dY.to(torch.bfloat16)), f"dY_bf16 (loss gradient {with_loss}) {tag}"
        _assert_exact(dE, dE0.double() + tok.sum((0, 2)).double(), f"dE {tag}",
                      lambda i, d: f"channel {i // D} column {i % D}: " + _explain_terms(round(d), tok[:, i // D, :, i % D].reshape(-1), lambda r: f"(batch {r // n}, position {r % n})"))
        _assert_exact(dpos[1:], dpos0[1:].double() + tok.sum((0, 1)).double(), f"dpos[1:] {tag}",
                      lambda i, d: f"position {i // D} column {i % D}: " + _explain_terms(round(d), tok[:, :, i // D, i % D].reshape(-1), lambda r: f"(batch {r // C}, channel {r % C})"))
        cls_sum = dx0_i[:, 0].long().sum(0).double()
        _assert_exact(dpos[0], dpos0[0].double() + cls_sum, f"dpos[0] {tag}", lambda i, d: f"column {i}: " + _explain_terms(round(d), dx0_i[:, 0, i].long(), lambda r: f"batch {r}"))
        _assert_exact(dcls, dcls0.double() + cls_sum, f"dcls {tag}", lambda i, d: f"column {i}: " + _explain_terms(round(d), dx0_i[:, 0, i].long(), lambda r: f"batch {r}"))


def test_patch_bwd_refusals(hip, monkeypatch):
    B, C, n = 2, 2, 4
    for D in (6, 1028):
        T = C * n
        dx0 = torch.zeros(B, T + 1, 1028, device="cuda")
        dYb = torch.zeros(B * T, 1028, dtype=torch.bfloat16, device="cuda")
        dE, dpos, dcls = torch.zeros(C, 1028, device="cuda"), torch.zeros(n + 1, 1028, device="cuda"), torch.zeros(1028, device="cuda")
        with pytest.raises(RuntimeError):
            hip.patch_bwd(dx0, None, dYb, dE, dpos, dcls, B, C, n, D)
    old = hip.set_deterministic(True)
    try:
        D = 384
        ws = torch.zeros(patch_bwd_plan(B, C, n, D).ws_floats, device="cuda")
        monkeypatch.setattr(hip, "_workspace", lambda k, like: ws[:ws.numel() - 4])
        with pytest.raises(RuntimeError):
            hip.patch_bwd(dx0[..., :D].contiguous(), None, dYb[:, :D].contiguous(), dE[:, :D].contiguous(), dpos[:, :D].contiguous(), dcls[:D].contiguous(), B, C, n, D)
        # the diversity statistics' workspace likewise
        Y = torch.ones(B, C * n, D, device="cuda")
        ws2 = torch.zeros(ortho_plan(B, C, n, D).ws_floats, device="cuda")
        monkeypatch.setattr(hip, "_workspace", lambda k, like: ws2[:ws2.numel() - 4])
        with pytest.raises(RuntimeError):
            hip.ortho_fwd(Y, torch.zeros(B, C, D, device="cuda"), torch.zeros(B, C, device="cuda"), torch.zeros(B, D, device="cuda"),
                          torch.zeros(B, C * n, device="cuda"), torch.zeros(B, 2, device="cuda"), B, C, n, D)
    finally:
        hip.set_deterministic(old)


@pytest.mark.parametrize("case", ORTHO_CASES, ids=lambda c: f"B{c.B}-C{c.C}-n{c.n}-D{c.D}")
def test_ortho_at_the_headline_grid(hip, case, reduction_mode):
    """dcv_ortho_fwd / dcv_ortho_bwd at test_ortho_loss's bounds, with the float64 reference (autograd) evaluated on the device."""
    B, C, n, D = case
    T = C * n
    Y = _randn(B, T, D, seed=121) + 0.3
    S, selfsq = torch.full((B, C, D), float("nan"), device="cuda"), torch.full((B, C), float("nan"), device="cuda")
    tot, inv, stats = torch.full((B, D), float("nan"), device="cuda"), torch.full((B, T), float("nan"), device="cuda"), torch.full((B, 2), float("nan"), device="cuda")
    hip.ortho_fwd(Y, S, selfsq, tot, inv, stats, B, C, n, D)
    Yr = Y.double().requires_grad_(True)
    f = torch.nn.functional.normalize(Yr, dim=-1).reshape(B, C, n, D)
    s = f.sum(2)
    pos_sum = ((s * s).sum(-1) - (f * f).sum(-1).sum(-1)).sum(-1)
    neg_sum = (s.sum(1) ** 2).sum(-1) - (s * s).sum(-1).sum(-1)
    tag = f"{tuple(case)} ({ortho_plan(*case)})"
    _within(stats[:, 0], pos_sum.detach(), 1e-4, 1e-3 * max(1.0, pos_sum.abs().max().item()), f"pos_sum {tag}")
    if C > 1:
        _within(stats[:, 1], neg_sum.detach(), 1e-4, 1e-3 * max(1.0, neg_sum.abs().max().item()), f"neg_sum {tag}")
    else:
        assert (stats[:, 1] == 0).all()
    coef = _randn(B, 2, seed=122)
    loss = (coef[:, 0].double() * pos_sum).sum() + ((coef[:, 1].double() * neg_sum).sum() if C > 1 else 0)
    loss.backward()
    del f, s, loss
    dY = torch.full_like(Y, float("nan"))
    hip.ortho_bwd(Y, S, tot, inv, coef, dY, B, C, n, D)
    _within(dY, Yr.grad, 1e-3, 1e-4 * Yr.grad.abs().max().item() + 1e-6, f"dY {tag}")


@pytest.mark.parametrize("case", ORTHO_CASES, ids=lambda c: f"B{c.B}-C{c.C}-n{c.n}-D{c.D}")
def test_ortho_exact_channel_sums(hip, case, reduction_mode):
    """The sums over a channel's tokens on exact inputs: every token row holds exactly 16 entries of +-1 (norm 4, so 1 / norm = 0.25 and the
    normalised entries are +-0.25 exactly); S is then a sum of n multiples of 0.25, selfsq = n, tot the sum of S over the channels, all exact
    in fp32 whatever the order: torch.equal in both reduction modes."""
    B, C, n, D = case
    T = C * n
    assert D % 16 == 0 and n < 2 ** 23  # n terms of one quantum (0.25) each per element of S; C n per element of tot
    off = _randint(0, D // 16 - 1, (B, T, 1), seed=131, dtype=torch.int64)
    mask = (torch.arange(D, device="cuda") % (D // 16)).expand(B, T, D) == off
    sgn = _randint(0, 1, (B, T, D), seed=132) * 2 - 1
    Yi = mask * sgn  # int32 in {-1, 0, 1}
    assert int(Yi.abs().sum(-1).min()) == 16 and int(Yi.abs().sum(-1).max()) == 16
    Y = Yi.float()
    S, selfsq = torch.full((B, C, D), float("nan"), device="cuda"), torch.full((B, C), float("nan"), device="cuda")
    tot, inv, stats = torch.full((B, D), float("nan"), device="cuda"), torch.full((B, T), float("nan"), device="cuda"), torch.full((B, 2), float("nan"), device="cuda")
    hip.ortho_fwd(Y, S, selfsq, tot, inv, stats, B, C, n, D)
    tag = f"{tuple(case)} ({ortho_plan(*case)})"
    sums = Yi.reshape(B, C, n, D).sum(2, dtype=torch.int64)
    assert torch.equal(inv, torch.full_like(inv, 0.25)), f"inv_norm {tag}"
    _assert_exact(S, sums.double() / 4, f"S {tag}", lambda i, d: f"(image, channel) {i // D} column {i % D}: " + _explain_terms(
        round(4 * d), Yi.reshape(B * C, n, D)[i // D, :, i % D], lambda t: f"token {t} (chunk {t // ORTHO_CHUNK})"))
    _assert_exact(selfsq, torch.full((B, C), float(n), dtype=torch.float64, device="cuda"), f"selfsq {tag}")
    _assert_exact(tot, sums.sum(1).double() / 4, f"tot {tag}")


def older_test_sizes():
    """The shapes of test_layernorm and the n of test_adamw_and_casts, read from test_kernels_gpu (for the CPU file's statement of the gap)."""
    import inspect

    import test_kernels_gpu as old
    marks = [m for m in old.test_layernorm.pytestmark if m.name == "parametrize" and m.args[0] == "M,D"]
    assert len(marks) == 1
    src = inspect.getsource(old.test_adamw_and_casts)
    ns = [int(v) for v in re.findall(r"^\s+n = (\d+)\s*$", src, flags=re.M)]
    assert len(ns) == 1
    return list(marks[0].args[1]), ns[0]
