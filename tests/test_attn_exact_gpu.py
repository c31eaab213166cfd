"""The attention kernels (csrc/attn.hip, attn_bwd.hip, attn_bwd3.hip) through hip.attn_fwd / hip.attn_bwd on operands for which every number they round is
exact, on both chains (plain and pre-scaled q): O, dQ, dV and the plain chain's dK bit for bit, the pre-scaled chain's dK to one bf16 ulp, LSE to four fp32
ulps, every output on NaN-prefilled memory.  One wrong term of N — a key lost at a tile edge, a mask off by one, a query row missing from a dK / dV sum —
changes a bit pattern here; the operands, the closed-form expectation, the rules and the reasons are in tests/test_attn_exact_cpu.py, which also proves on
the CPU that the rules flag such defects.  The "uniform" sweep (q = 0: P = 1 / N) runs every token count from 1 to 700 and the channel-sampling counts
beyond.  Needs an MI355X: run with -m gpu."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_attn_exact_cpu import (DUST, GROUP_CASES, GROUP_IDS, BATCHED, LSE_ULPS, SCALE, UNIFORM_CHUNKS, compare_group, from_device_layout,  # noqa: E402
                                 group_operands, lse_mismatch, to_device_layout, ulp1_mismatch)
from test_attn_seams_gpu import dkdv3_plan  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def _run(hip, qkv, dO, B, N, H, Nq, prescaled):
    """One chain on NaN-filled outputs: o, lse, dqkv."""
    D = H * 64
    o = torch.full((B, N, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, H, N), float("nan"), device="cuda")
    dqkv = torch.full((B, N, 3 * D), float("nan"), dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(2, B, H, N, device="cuda")
    hip.attn_fwd(qkv, o, lse, B, N, H, 64, SCALE, nq=Nq, prescaled=prescaled)
    hip.attn_bwd(qkv, o, dO, lse, ws, dqkv, B, N, H, 64, SCALE, nq=Nq, prescaled=prescaled)
    torch.cuda.synchronize()
    return o, lse, dqkv


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("case", GROUP_CASES, ids=GROUP_IDS)
def test_group_operands(hip, case, prescaled):
    """Which rule holds for which output, and the kernel line behind it: compare_group in tests/test_attn_exact_cpu.py."""
    B, N, H = case.B, case.N, case.H
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = dkdv3_plan(B, N, H, case.Nq, cus)
    assert (p.tail, p.in_loop) == (case.tail, case.in_loop) and (case not in BATCHED or p.walk_max >= 2), \
        f"this device has {cus} CUs (an MI355X has 256): the plan {p} is not the one this case is in the table for"
    ops = group_operands(case)
    qkv, dO = to_device_layout(ops, prescaled)
    o, lse, dqkv = _run(hip, qkv.cuda(), dO.cuda(), B, N, H, case.Nq, prescaled)
    slots = dqkv.cpu().reshape(B, N, 3, H * 64)
    got = dict(o=from_device_layout(o.cpu(), B, H), lse=lse.cpu().reshape(B * H, N),
               dq=from_device_layout(slots[:, :, 0], B, H), dk=from_device_layout(slots[:, :, 1], B, H), dv=from_device_layout(slots[:, :, 2], B, H))
    found = compare_group(got, ops.ps if prescaled else ops.plain, H, prescaled)
    assert not found, f"{'pre-scaled' if prescaled else 'plain'} chain, key_hi {p.key_hi} (tail: {p.tail}):\n" + "\n".join(found)


_uniform = {}


def _uniform_operands(H, N):
    """k (a +-1 address and 0 / 1 payloads), v in {-2, 0, 2} and dO in {-1, 0, 1} as in the group operands, q = 0, for the largest N; a sweep takes the first
    rows.  Every column of dO is drawn so that the sum of its first n rows stays in {-1, 0, 1} for every n: bf16(p) sum(dO) is then a bf16 number, the
    rounding of the dV output adds nothing to p's, and the 2^-8 bound on dV is attainable (with a free sum the two roundings reach 2^-7); a row missing
    from the sum moves such a column from +-1 to 0 or +-2."""
    if not _uniform:
        g = torch.Generator().manual_seed(4242)
        qkv = torch.zeros(1, N, 3, H, 64)
        qkv[0, :, 1, :, :12] = torch.randint(0, 2, (N, H, 12), generator=g).float() * 2 - 1
        qkv[0, :, 1, :, 12:] = torch.randint(0, 2, (N, H, 52), generator=g).float()
        qkv[0, :, 2] = torch.tensor([-2.0, 0.0, 0.0, 2.0])[torch.randint(0, 4, (N, H, 64), generator=g)]
        dO, run = torch.randint(-1, 2, (1, N, H * 64), generator=g), torch.zeros(H * 64, dtype=torch.long)
        for i in range(N):
            dO[0, i] = torch.where((run + dO[0, i]).abs() > 1, -dO[0, i], dO[0, i])
            run += dO[0, i]
        _uniform.update(qkv=qkv.reshape(1, N, 3 * H * 64).to(torch.bfloat16).cuda(), dO=dO.to(torch.bfloat16).cuda())
    return _uniform["qkv"], _uniform["dO"]


UNIFORM_CHECKS = ["LSE = ln N", "O rows identical", "O within one bf16 ulp of mean(v)", "dV rows identical", "dV within 2^-8 of sum(dO) / N", "dK zero", "dQ"]


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("ns", UNIFORM_CHUNKS, ids=[f"N{c[0]}-{c[-1]}" for c in UNIFORM_CHUNKS])
def test_uniform_sweep(hip, ns, prescaled):
    """q = 0: every score is 0 and P = 1 / N over all keys, for B = 1, H = 2.
      LSE   ln N within the fp32 bound of lse_mismatch (m = 0, l = N exactly: only logf rounds); one key too many or too few moves it by 1 / N >= 6e-4
      O     every row sums the same v rows in the same order and multiplies by the same fl(1 / N) (attn.hip:235-243): rows bit-identical, one bf16 ulp of mean(v)
      dV    the same bf16(p) for every (row, key) and the same order over the rows for every key: rows bit-identical; sum(dO) bf16(p) is exact in fp32 and,
            sum(dO) being 0 or +-1 (see _uniform_operands), in bf16: the error is the rounding of p alone, 2^-8 relative of sum(dO) / N
      dK    dS^T q with q = 0: zero (to 2^-30)
      dQ    (scale / N) dO (sum_j (v_j - mean v) k_j^T) in float64, at the bounds of the older tests (rtol 3e-2, atol 3e-2 max|ref|): dS is rounded to bf16 there."""
    H, D = 2, 128
    allqkv, alldO = _uniform_operands(H, max(max(c) for c in UNIFORM_CHUNKS))
    flags = []
    for N in ns:
        qkv, dO = allqkv[:, :N].contiguous(), alldO[:, :N].contiguous()
        o, lse, dqkv = _run(hip, qkv, dO, 1, N, H, None, prescaled)
        k, v = qkv[0, :, D:2 * D].double(), qkv[0, :, 2 * D:].double()
        dq, dk, dv = dqkv[0, :, :D], dqkv[0, :, D:2 * D], dqkv[0, :, 2 * D:]
        vbar = v.mean(0, keepdim=True)
        dvref = dO[0].double().sum(0, keepdim=True) / N
        dv_tol = torch.where(dvref != 0, dvref.abs() * 2.0 ** -8, torch.full_like(dvref, DUST))
        dqref = torch.cat([(SCALE / N) * dO[0, :, 64 * h:64 * h + 64].double() @ ((v - vbar)[:, 64 * h:64 * h + 64].T @ k[:, 64 * h:64 * h + 64])
                           for h in range(H)], 1)
        flags.append(torch.stack([
            ~lse_mismatch(lse, torch.full_like(lse, math.log(N), dtype=torch.float64), LSE_ULPS).any(),
            (o[0].view(torch.int16) == o[0, :1].view(torch.int16)).all(),
            ~ulp1_mismatch(o[0], vbar.expand(N, -1)).any(),
            (dv.view(torch.int16) == dv[:1].view(torch.int16)).all(),
            ((dv.double() - dvref).abs() <= dv_tol).all(),
            (dk.double().abs() <= DUST).all(),
            ((dq.double() - dqref).abs() <= 3e-2 * dqref.abs().max() + 3e-2 * dqref.abs()).all()]))
    ok = torch.stack(flags).cpu()
    bad = [f"N {N}: " + ", ".join(c for c, good in zip(UNIFORM_CHECKS, row.tolist()) if not good) for N, row in zip(ns, ok) if not bool(row.all())]
    assert not bad, f"{'pre-scaled' if prescaled else 'plain'} chain, {len(bad)} of {len(ns)} token counts:\n" + "\n".join(bad[:20])
