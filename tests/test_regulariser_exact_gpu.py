"""The two regularisers of the train step on the device: the channel-diversity loss (ortho_fwd_partial, ortho_fwd_final, ortho_bwd_kernel in csrc/tokenizer.hip)
through hip.ortho_fwd / hip.ortho_bwd in both reduction modes, and the channel-proxy loss (proxy_loss_kernel in csrc/loss.hip) through hip.proxy_loss.

* Ortho, bit for bit: on the dyadic operands of tests/test_regulariser_exact_cpu.py every output — inv_norm, S, selfsq, tot, (pos_sum, neg_sum) and every element
  of dY, the rows that are exactly 0 included (base * 1e12f) — is torch.equal to the float64 closed form.  That file proves that the expectation is an fp32 number
  and that no summation order or multiply-add contraction can change it, and that one wrong term (an element of S left out of the sum of squares, a column left
  out of g . fh, an inv_norm from the neighbouring row, coef or tot from the previous image) changes a bit.
* Ortho with one patch per channel on ordinary data: pos_sum is exactly 0 (no same-channel pair exists; the host divides by pos_cnt = 1e-6).
* Ortho with rows under the 1e-12 clamp (norm 3e-13, and 0) against float64 autograd through F.normalize at test_ortho_loss's bounds, the clamped rows and the
  others each against their own max |grad|.
* The refusals of both entries (D % 4, D > 1024) leave every output byte alone.
* Proxy loss: ragged and limit shapes ((1, 1) .. (16, 1024), (32, 512): D that is no multiple of the wave, D = 1000 and 1024 with dn[16], the over-64-KB
  dynamic-LDS path and a small call after it), structured operands (p = e, p = e[perm], e = -p), logits down to -800, and the one thing that is exact about
  it; loss and gradients live between 64-float sentinels that must come back untouched.
Needs an MI355X: run with -m gpu."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_regulariser_exact_cpu import (INV_CLAMP, ORTHO_CASES, ORTHO_IDS, PROXY_KINDS, PROXY_SAT_CASES, PROXY_SAT_FACTOR, PROXY_SCALE,  # noqa: E402
                                        PROXY_SCALE_SAT, PROXY_SHAPES, PROXY_STRUCTURED, clamp_operands, old_bounds_findings, ortho_expect,
                                        ortho_mismatches, ortho_operands, ortho_reference64, proxy_errors, proxy_exact_findings, proxy_exact_operands,
                                        proxy_operands, proxy_perm, proxy_reference, proxy_saturation_bound)

pytestmark = pytest.mark.gpu

SENT = -12345.0
NAN = float("nan")


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


# ---- ortho ----------------------------------------------------------------------------------------------------------------------------------------------------
def _ortho_run(hip, Y, coef, B, C, n, D, fill=NAN):
    """hip.ortho_fwd and hip.ortho_bwd on outputs prefilled with NaN: the six outputs by name."""
    T = C * n
    o = dict(S=torch.full((B, C, D), fill, device="cuda"), selfsq=torch.full((B, C), fill, device="cuda"), tot=torch.full((B, D), fill, device="cuda"),
             inv_norm=torch.full((B, T), fill, device="cuda"), stats=torch.full((B, 2), fill, device="cuda"), dY=torch.full((B, T, D), fill, device="cuda"))
    hip.ortho_fwd(Y, o["S"], o["selfsq"], o["tot"], o["inv_norm"], o["stats"], B, C, n, D)
    hip.ortho_bwd(Y, o["S"], o["tot"], o["inv_norm"], coef, o["dY"], B, C, n, D)
    torch.cuda.synchronize()
    return o


_expect = {}


def _ortho_expectation(case):
    if case not in _expect:
        Y, coef, _ = ortho_operands(case)
        _expect[case] = ortho_expect(Y, coef, case)
    return _expect[case]


@pytest.mark.parametrize("case", ORTHO_CASES, ids=ORTHO_IDS)
def test_ortho_exact(hip, case, reduction_mode):
    """Every output of the forward and the backward on the dyadic operands, torch.equal with the closed form (rules and their proof:
    tests/test_regulariser_exact_cpu.py).  A failure names the image, channel, token and column."""
    B, C, n, D = case[:4]
    Y, coef, _ = ortho_operands(case)
    want = _ortho_expectation(case)
    o = _ortho_run(hip, Y.cuda(), coef.cuda(), B, C, n, D)
    got = {k: v.cpu() for k, v in o.items()}
    if case.zero_rows:
        assert bool(want["zero"].any()) and bool((got["inv_norm"][want["zero"]] == torch.tensor(1e12, dtype=torch.float32)).all()), "inv_norm of the zero rows is not 1e12f"
        assert INV_CLAMP == float(torch.tensor(1e12, dtype=torch.float32))
    found = ortho_mismatches(got, want, Y, case)
    assert not found, f"{case.covers} ({reduction_mode}):\n" + "\n".join(found)
    if C == 1:
        # what the C == 1 guard of ortho_bwd_kernel is for: tot - s_c is bitwise 0, so only a non-finite dL/dneg_sum can show whether cb was zeroed
        cinf = coef.clone()
        cinf[:, 1] = float("inf")
        dY = torch.full((B, C * n, D), NAN, device="cuda")
        hip.ortho_bwd(Y.cuda(), o["S"], o["tot"], o["inv_norm"], cinf.cuda(), dY, B, C, n, D)
        found = ortho_mismatches(dict(got, dY=dY.cpu()), want, Y, case)
        assert not found, "C == 1 with coef[:, 1] = inf:\n" + "\n".join(found)


@pytest.mark.parametrize("B,C,D", [(4, 8, 384), (2, 3, 192)])
def test_ortho_single_patch_on_ordinary_data(hip, B, C, D, reduction_mode):
    """n == 1 (image side == patch side): no same-channel pair exists, the reference's pos_pairs_mean is 0 / 1e-6 = 0 (models/loss_fn.py:40-47), and pos_sum must be
    exactly 0 — not the rounding difference of sum S^2 against sum q inv inv, which pos_cnt = 1e-6 would multiply by 1e6.  neg_sum and dY at test_ortho_loss's bounds."""
    n = 1
    Y = (torch.randn(B, C, D, generator=torch.Generator().manual_seed(211)) + 0.3).cuda()
    for seed in (212, 213):
        coef = torch.randn(B, 2, generator=torch.Generator().manual_seed(seed)).cuda()
        got = _ortho_run(hip, Y, coef, B, C, n, D)
        print(f"n == 1, B {B} C {C} D {D} ({reduction_mode}): pos_sum {got['stats'][:, 0].tolist()}")
        assert bool((got["stats"][:, 0] == 0).all()), f"pos_sum at n == 1 is not exactly 0: {got['stats'][:, 0].tolist()} (times 1e6 in the loss)"
        pos, neg, grad = ortho_reference64(Y, coef, C, n)
        assert float(pos.abs().max()) < 1e-12
        assert old_bounds_findings(got, pos, neg, grad, C) == []


def test_ortho_rows_under_the_clamp(hip, reduction_mode):
    """Rows of norm 3e-13 and rows equal to 0 among randn + 0.3 rows: normalize divides them by the constant 1e-12, their gradient is g * 1e12 without the
    projection (the `clamped` branch of ortho_bwd_kernel).  float64 autograd through F.normalize on the device; test_ortho_loss's bounds, the rows under the
    clamp and the others each with their own max |grad| (the former are 1e12 times larger and would hide the rest behind the absolute term)."""
    (B, C, n, D), Y, coef, mask = clamp_operands("cuda")
    got = _ortho_run(hip, Y, coef, B, C, n, D)
    assert bool((got["inv_norm"][mask] == torch.tensor(1e12, dtype=torch.float32)).all()) and bool((got["inv_norm"][~mask] < 1).all())
    pos, neg, grad = ortho_reference64(Y, coef, C, n)
    assert float(grad[mask].abs().max()) > 1e9 * float(grad[~mask].abs().max())
    assert old_bounds_findings(got, pos, neg, grad, C, rows=mask) == []


def test_ortho_refusals(hip, reduction_mode):
    """D % 4 != 0 and D > 1024 are refused by both entries before anything is launched: no output byte changes."""
    B, C, n = 2, 2, 4
    T = C * n
    for D in (6, 1028):
        Y = torch.ones(B, T, 1028, device="cuda")
        coef = torch.ones(B, 2, device="cuda")
        o = dict(S=torch.full((B, C, 1028), SENT, device="cuda"), selfsq=torch.full((B, C), SENT, device="cuda"), tot=torch.full((B, 1028), SENT, device="cuda"),
                 inv_norm=torch.full((B, T), SENT, device="cuda"), stats=torch.full((B, 2), SENT, device="cuda"), dY=torch.full((B, T, 1028), SENT, device="cuda"))
        with pytest.raises(RuntimeError):
            hip.ortho_fwd(Y, o["S"], o["selfsq"], o["tot"], o["inv_norm"], o["stats"], B, C, n, D)
        with pytest.raises(RuntimeError):
            hip.ortho_bwd(Y, o["S"], o["tot"], o["inv_norm"], coef, o["dY"], B, C, n, D)
        torch.cuda.synchronize()
        for k, v in o.items():
            assert bool((v == SENT).all()), f"D = {D}: {k} was written by a refused call"


# ---- proxy loss -----------------------------------------------------------------------------------------------------------------------------------------------
def _guarded(*shape):
    """a NaN-filled fp32 tensor with 64 floats of sentinel before and after it, in one allocation"""
    n = int(np.prod(shape))
    buf = torch.full((n + 128,), SENT, device="cuda")
    buf[64:64 + n] = NAN
    return buf, buf[64:64 + n].view(*shape)


def _proxy_run(hip, e, p, scale):
    """hip.proxy_loss on guarded outputs: (loss [1], d_emb, d_proxies), sentinels checked."""
    C, D = e.shape
    bufs, outs = zip(*(_guarded(1), _guarded(C, D), _guarded(C, D)))
    hip.proxy_loss(e.cuda(), p.cuda(), scale, *outs)
    torch.cuda.synchronize()
    for name, buf, out in zip(("loss", "d_emb", "d_proxies"), bufs, outs):
        n = out.numel()
        assert bool((buf[:64] == SENT).all()) and bool((buf[64 + n:] == SENT).all()), f"{name} [{C}, {D}]: a sentinel next to the output was overwritten"
        assert not bool(out.isnan().any()), f"{name} [{C}, {D}]: an element was not written (or is NaN)"
    return tuple(o.clone() for o in outs)


def _proxy_check(hip, C, D, kind, scale=PROXY_SCALE):
    """One call against float64 autograd at test_proxy_loss_kernel's bounds (2e-6 relative on the loss, 2e-5 max |grad| + 1e-9 on the gradients)."""
    e, p = proxy_operands(C, D, kind)
    loss, de, dp = _proxy_run(hip, e, p, scale)
    assert bool(torch.isfinite(loss).all() and torch.isfinite(de).all() and torch.isfinite(dp).all()), (C, D, kind)
    rl, rde, rdp = proxy_reference(e.cuda(), p.cuda(), scale)
    if kind == "zero row":  # the clamped row's gradient is 1e12-scaled in both; finiteness above, the rest of d_emb here
        de, rde = de[1:], rde[1:]
    err = proxy_errors((loss, de, dp), (rl, rde, rdp))
    assert max(err) <= 1, f"[{C}, {D}] {kind}: loss, d_emb, d_proxies are {err} times their bounds"
    return err


@pytest.mark.parametrize("C,D", PROXY_SHAPES)
def test_proxy_ragged_and_limit_shapes(hip, C, D):
    """D that is no multiple of 64 (the d < D guards false part-way through a wave), D = 1000 and 1024 (all of dn[16]), C = 1, C > 16 (rows walk the waves twice),
    and the two shapes at exactly 16384 floats, which take the over-64-KB dynamic-LDS path."""
    for kind in PROXY_KINDS:
        _proxy_check(hip, C, D, kind)


def test_proxy_small_call_after_the_large_lds_path(hip):
    """A call with 128 KB of dynamic LDS must not disturb the next small one: (3, 4) after each limit shape gives the bits it gives alone."""
    e, p = proxy_operands(3, 4, "random")
    alone = _proxy_run(hip, e, p, PROXY_SCALE)
    for C, D in ((16, 1024), (32, 512)):
        _proxy_check(hip, C, D, "random")
        again = _proxy_run(hip, e, p, PROXY_SCALE)
        assert all(torch.equal(a, b) for a, b in zip(alone, again)), f"(3, 4) after ({C}, {D}) differs from (3, 4) alone"
        for kind in PROXY_KINDS:
            _proxy_check(hip, 3, 4, kind)


@pytest.mark.parametrize("C,D", [(8, 384), (5, 100)])
def test_proxy_structured_operands(hip, C, D):
    """p = e (diagonal logits 0); p = e[perm] with a permutation that has no fixed point (the right class is the far one; an L[i][j] / L[j][i] mix-up in
    d_proxies is a permuted gradient); e_i = -p_i (the right class is the farthest point of the sphere)."""
    assert all(int(proxy_perm(C)[i]) != i for i in range(C))
    for kind in PROXY_STRUCTURED:
        _proxy_check(hip, C, D, kind)


def test_proxy_saturated_logits(hip):
    """scale^2 = 1 / 0.005 = 200: logits reach -800 and expf underflows off the maximum.  Loss and gradients are finite and match float64.  The bounds at the
    workload's scale were not set for logits this large, so the bound is measured: the worst error of the fp32 restatement of the kernel's formulas
    (tests/test_regulariser_exact_cpu.py, torch's summation order and exp / log, computed here on the CPU) against float64 on the same operands, times 4 for the
    kernel's own summation order and its expf / logf.  Measured (profiles/regulariser_exact.txt): restatement 0.105 / 1.14 / 0.78 times the workload-scale bounds
    for loss / d_emb / d_proxies; the kernel's figures are in that file."""
    bound = proxy_saturation_bound()
    worst = [0.0, 0.0, 0.0]
    for C, D, kind in PROXY_SAT_CASES:
        e, p = proxy_operands(C, D, kind)
        loss, de, dp = _proxy_run(hip, e, p, PROXY_SCALE_SAT)
        assert bool(torch.isfinite(loss).all() and torch.isfinite(de).all() and torch.isfinite(dp).all()), (C, D, kind)
        err = proxy_errors((loss, de, dp), proxy_reference(e.cuda(), p.cuda(), PROXY_SCALE_SAT))
        print(f"saturation [{C}, {D}] {kind}: kernel error {err} (multiples of the workload-scale bounds)")
        worst = [max(a, b) for a, b in zip(worst, err)]
    print(f"saturation: restatement worst {list(bound)}, factor {PROXY_SAT_FACTOR}, kernel worst {worst}")
    for name, w, b in zip(("loss", "d_emb", "d_proxies"), worst, bound):
        assert w <= PROXY_SAT_FACTOR * b, f"{name}: kernel error {w} exceeds {PROXY_SAT_FACTOR} x the restatement's {b} (multiples of the workload-scale bounds)"


def test_proxy_zero_row_exact(hip):
    """The loss goes through expf / logf, so value and gradients cannot be held bit for bit.  What is exact: dyadic rows of norm 4 on disjoint supports, scale = 2
    and e[0] = 0 make d_emb[0] = dn / 1e-12f with dn[d] = +-2 w_j for the one proxy j that has an entry at d: exact zeros elsewhere, one bit pattern per proxy
    with the proxy's signs, one for all wrong classes, and the magnitudes within 8 ulps of 2 (1 - 1/C) / C / 1e-12f and 2 / C^2 / 1e-12f
    (proxy_exact_findings derives the 8).  Everything else: finite."""
    e, p = proxy_exact_operands()
    loss, de, dp = _proxy_run(hip, e, p, 2.0)
    assert bool(torch.isfinite(loss).all() and torch.isfinite(de).all() and torch.isfinite(dp).all())
    found = proxy_exact_findings(de[0], p)
    assert not found, "\n".join(found)
    rl, rde, rdp = proxy_reference(e.cuda(), p.cuda(), 2.0)
    err = proxy_errors((loss, de[1:], dp), (rl, rde[1:], rdp))
    assert max(err) <= 1, err
