"""The attention probe kernels through hip.attn_probs, hip.attn_channel_mass and hip.attn_rollout_step (csrc/attn_probs.hip, attn_channel_mass.hip,
attn_rollout.hip; both forms, plain and pre-scaled q) on operands whose ideal softmax is exactly 1, 1/2, 1/4 or 0, with their own structure per (batch,
head), against closed forms in float64: P, the token masses T, the channel matrix A and the rollout step, every output in a NaN-prefilled buffer between
guards.  A key lost at a segment edge, a flush into the wrong channel, a clamped row that leaks, another head's LSE moves an output by a quarter of a term
or more; the bound is 2^-10 relative (2^-30 where the expectation is zero).  The operands, the expectations, the rules with the derivation of the bound, the
regimes each table reaches and the proof that the rules flag such defects are in tests/test_attn_probes_exact_cpu.py.  LSE is the float32 rounding of the
closed form; the three *_with_the_forwards_lse tests take it from hip.attn_fwd, the chain the model runs.  Needs an MI355X: run with -m gpu.

Measured on the MI355X (each test prints its largest err / bound; the bounds are the derived ones, not tightened to these):
  plain form       P, T, A and out: 0.065 at every shape of the sweeps and tables (0.022 where the rows do not meet every group size: N = 1569 with Nq = 1, C = 1
                   with n_p = 1): the 6.3e-5 is fl(-lse LOG2E)'s rounding on the 2^-13 grid of the exponent, the same for every row of a group size;
  pre-scaled form  P and T: 0, bit for bit 1 / g and its sums — the ideal exponent 1110 + log2 g is itself on the 2^-13 grid and fl(-lse LOG2E) lands on
                   it, 1110 - 1110 cancels exactly in the accumulator; A at most 1.2e-4 (the fp32 row chain and 1 / n_p), out at most 8.1e-5
                   (fl((1 - alpha) / H));
  LSE from attn_fwd  plain 0.052 of the wider bound (the same 6.3e-5: the forward's LSE is the closed form's float32), pre-scaled 0 (A 5.7e-5, out 6.5e-5);
  A against mean64(T)  at most 0.333 (plain) and 0.222 (pre-scaled) in the sweep, 0.062 in the table; A[:, :, 0] = T[:, :, 0] bit for bit everywhere.
The 88 tests of this module take 7.4 s in all; the slowest, a chunk of 76 channel-mass shapes with N up to 1041, 0.5 s."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_attn_probes_exact_cpu import (ALPHAS, GUARD, MASS_FWD, MASS_SWEEP_CHUNKS, MASS_TABLE, PROBS_FWD, PROBS_SWEEP_CHUNKS, PROBS_TABLE, REL, REL_FWD,  # noqa: E402
                                        ROLLOUT_FWD, ROLLOUT_SWEEP_CHUNKS, ROLLOUT_TABLE, SCALE, buffer_findings, closed_lse, device_qkv, guarded_nan,
                                        mean_rule, out_ref, p_ref, probe_ops, rollout_weights, rule, seg_mean64, t_ref, where_bad, _ops)

pytestmark = pytest.mark.gpu
FORMS = pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "prescaled"])


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    yield h
    _ops.clear()  # the sweeps' structures


def _inputs(hip, ops, prescaled, fwd_lse):
    """qkv and LSE on the device: the closed form's float32 rounding, or what hip.attn_fwd writes into it (rows >= Nq keep the closed form's 0)."""
    qkv = device_qkv(ops, prescaled).cuda()
    lse = closed_lse(ops, prescaled).cuda()
    if fwd_lse:
        lse[:, :, :ops.Nq] = float("nan")
        o = torch.empty(ops.B, ops.N, ops.H * 64, dtype=torch.bfloat16, device="cuda")
        hip.attn_fwd(qkv, o, lse, ops.B, ops.N, ops.H, 64, SCALE, nq=ops.Nq, prescaled=prescaled)
    return qkv, lse


def _tag(prescaled):
    return "pre-scaled" if prescaled else "plain"


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _probs(hip, B, H, N, Nq, prescaled, fwd_lse=False):
    ops = probe_ops(B, H, N, Nq)
    qkv, lse = _inputs(hip, ops, prescaled, fwd_lse)
    n = B * H * ops.Nq * N
    buf, inner = guarded_nan(n, "cuda")
    hip.attn_probs(qkv, lse, inner.view(B, H, ops.Nq, N), B, N, H, 64, SCALE, nq=Nq, prescaled=prescaled)
    buf = buf.cpu()
    bad, ratio = rule(buf[GUARD:GUARD + n].view(B, H, ops.Nq, N), p_ref(ops), 0, REL_FWD if fwd_lse else REL)
    return [f"B{B} H{H} N{N} Nq{Nq}: {x}" for x in buffer_findings("P", buf, n) + where_bad("P", bad, ratio)], ratio


@FORMS
@pytest.mark.parametrize("ns", PROBS_SWEEP_CHUNKS, ids=[f"N{c[0]}-{c[-1]}" for c in PROBS_SWEEP_CHUNKS])
def test_probs_sweep(hip, ns, prescaled):
    found, worst = [], 0.0
    for N in ns:
        f, r = _probs(hip, 1, 2, N, None, prescaled)
        found, worst = found + f, max(worst, r)
    print(f"probs {_tag(prescaled)} N {ns[0]}..{ns[-1]}: largest err / bound {worst:.3g}")
    assert not found, "\n".join(found[:20])


@FORMS
@pytest.mark.parametrize("B,H,N,Nq", PROBS_TABLE, ids=[f"B{b}-H{h}-N{n}-Nq{q or 'all'}" for b, h, n, q in PROBS_TABLE])
def test_probs_table(hip, B, H, N, Nq, prescaled):
    found, worst = _probs(hip, B, H, N, Nq, prescaled)
    print(f"probs {_tag(prescaled)} B{B} H{H} N{N} Nq{Nq}: largest err / bound {worst:.3g}")
    assert not found, "\n".join(found)


@FORMS
def test_probs_with_the_forwards_lse(hip, prescaled):
    found, worst = [], 0.0
    for B, H, N, Nq in PROBS_FWD:
        f, r = _probs(hip, B, H, N, Nq, prescaled, fwd_lse=True)
        found, worst = found + f, max(worst, r)
    print(f"probs {_tag(prescaled)}, LSE from attn_fwd: largest err / bound {worst:.3g}")
    assert not found, "\n".join(found)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _mass(hip, B, H, C_, n_p, prescaled, modes=("both",), fwd_lse=False):
    """modes: "both" (tok and ch), "ch" (ch alone, the token masses through a NaN-filled workspace), "tok" (tok alone)."""
    N, W = 1 + C_ * n_p, 1 + C_
    ops = probe_ops(B, H, N)
    qkv, lse = _inputs(hip, ops, prescaled, fwd_lse)
    rel = REL_FWD if fwd_lse else REL
    Tr = t_ref(ops, C_, n_p)
    Ar = seg_mean64(Tr, C_, n_p)
    nT, nA = B * H * N * W, B * H * W * W
    assert hip.load().dcv_attn_channel_mass_ws_floats(B, N, H, C_) == nT
    found, ratios, first = [], dict(T=0.0, A=0.0, AT=0.0), {}
    for mode in modes:
        bT, iT = guarded_nan(nT, "cuda")  # in mode "ch": the workspace
        bA, iA = guarded_nan(nA, "cuda")
        tok = iT.view(B, H, N, W) if mode != "ch" else None
        ch = iA.view(B, H, W, W) if mode != "tok" else None
        hip.attn_channel_mass(qkv, lse, B, N, H, 64, SCALE, C_, n_p, tok=tok, ch=ch, prescaled=prescaled, ws=iT if mode == "ch" else None)
        bT, bA = bT.cpu(), bA.cpu()
        T, A = bT[GUARD:GUARD + nT].view(B, H, N, W), bA[GUARD:GUARD + nA].view(B, H, W, W)
        f = buffer_findings("T" if mode != "ch" else "workspace", bT, nT)
        bad, r = rule(T, Tr, 4, rel)
        f += where_bad("T", bad, r)
        ratios["T"] = max(ratios["T"], r)
        if mode == "tok":
            f += [] if bool(bA.isnan().all()) else ["ch: written though not asked for"]
        else:
            f += buffer_findings("A", bA, nA)
            bad, r = rule(A, Ar, n_p, rel)
            f += where_bad("A", bad, r)
            ratios["A"] = max(ratios["A"], r)
            bad, r, cls_equal = mean_rule(A, T, C_, n_p)
            f += where_bad("A against the segment mean of T", bad, r) + ([] if cls_equal else ["A[:, :, 0] is not T[:, :, 0] bit for bit"])
            ratios["AT"] = max(ratios["AT"], r)
        for name, x in (("T", T), ("A", A)):
            if (mode, name) != ("tok", "A"):
                if not torch.equal(first.setdefault(name, x), x):
                    f.append(f"{name}: differs from what the call for both outputs wrote")
        found += [f"B{B} H{H} C{C_} n_p{n_p} ({mode}): {x}" for x in f]
    return found, ratios


def _merge(a, b):
    return {k: max(a[k], b[k]) for k in a}


@FORMS
@pytest.mark.parametrize("shapes", MASS_SWEEP_CHUNKS, ids=[f"C{c[0][0]}n{c[0][1]}-C{c[-1][0]}n{c[-1][1]}" for c in MASS_SWEEP_CHUNKS])
def test_channel_mass_sweep(hip, shapes, prescaled):
    found, worst = [], dict(T=0.0, A=0.0, AT=0.0)
    for C_, n_p in shapes:
        f, r = _mass(hip, 1, 2, C_, n_p, prescaled)
        found, worst = found + f, _merge(worst, r)
    print(f"channel mass {_tag(prescaled)} {shapes[0]}..{shapes[-1]}: largest err / bound T {worst['T']:.3g} A {worst['A']:.3g} A against mean(T) {worst['AT']:.3g}")
    assert not found, "\n".join(found[:20])


@FORMS
@pytest.mark.parametrize("B,H,C_,n_p", MASS_TABLE, ids=[f"B{b}-H{h}-C{c}-n{n}" for b, h, c, n in MASS_TABLE])
def test_channel_mass_table(hip, B, H, C_, n_p, prescaled):
    found, worst = _mass(hip, B, H, C_, n_p, prescaled, modes=("both", "ch", "tok"))
    print(f"channel mass {_tag(prescaled)} B{B} H{H} C{C_} n_p{n_p}: largest err / bound T {worst['T']:.3g} A {worst['A']:.3g} A against mean(T) {worst['AT']:.3g}")
    assert not found, "\n".join(found)


@FORMS
def test_channel_mass_with_the_forwards_lse(hip, prescaled):
    found, worst = [], dict(T=0.0, A=0.0, AT=0.0)
    for B, H, C_, n_p in MASS_FWD:
        f, r = _mass(hip, B, H, C_, n_p, prescaled, fwd_lse=True)
        found, worst = found + f, _merge(worst, r)
    print(f"channel mass {_tag(prescaled)}, LSE from attn_fwd: largest err / bound T {worst['T']:.3g} A {worst['A']:.3g} A against mean(T) {worst['AT']:.3g}")
    assert not found, "\n".join(found)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _rollout(hip, B, H, N, prescaled, fwd_lse=False):
    ops = probe_ops(B, H, N)
    qkv, lse = _inputs(hip, ops, prescaled, fwd_lse)
    found, worst = [], 0.0
    for name, w in rollout_weights(B, N).items():
        wd = w.cuda()
        for alpha in ALPHAS:
            buf, inner = guarded_nan(B * N, "cuda")
            hip.attn_rollout_step(qkv, lse, wd, inner.view(B, N), B, N, H, 64, SCALE, alpha, prescaled=prescaled)
            buf = buf.cpu()
            ref, cnt = out_ref(ops, w, alpha)
            bad, r = rule(buf[GUARD:GUARD + B * N].view(B, N), ref, cnt, REL_FWD if fwd_lse else REL)
            found += [f"B{B} H{H} N{N} w {name} alpha {alpha}: {x}" for x in buffer_findings("out", buf, B * N) + where_bad("out", bad, r)]
            worst = max(worst, r)
        assert torch.equal(wd.cpu(), w)
    return found, worst


@FORMS
@pytest.mark.parametrize("ns", ROLLOUT_SWEEP_CHUNKS, ids=[f"N{c[0]}-{c[-1]}" for c in ROLLOUT_SWEEP_CHUNKS])
def test_rollout_sweep(hip, ns, prescaled):
    found, worst = [], 0.0
    for N in ns:
        f, r = _rollout(hip, 1, 3, N, prescaled)
        found, worst = found + f, max(worst, r)
    print(f"rollout {_tag(prescaled)} N {ns[0]}..{ns[-1]}: largest err / bound {worst:.3g}")
    assert not found, "\n".join(found[:20])


@FORMS
@pytest.mark.parametrize("B,H,N", ROLLOUT_TABLE, ids=[f"B{b}-H{h}-N{n}" for b, h, n in ROLLOUT_TABLE])
def test_rollout_table(hip, B, H, N, prescaled):
    found, worst = _rollout(hip, B, H, N, prescaled)
    print(f"rollout {_tag(prescaled)} B{B} H{H} N{N}: largest err / bound {worst:.3g}")
    assert not found, "\n".join(found)


@FORMS
def test_rollout_with_the_forwards_lse(hip, prescaled):
    found, worst = [], 0.0
    for B, H, N in ROLLOUT_FWD:
        f, r = _rollout(hip, B, H, N, prescaled, fwd_lse=True)
        found, worst = found + f, max(worst, r)
    print(f"rollout {_tag(prescaled)}, LSE from attn_fwd: largest err / bound {worst:.3g}")
    assert not found, "\n".join(found)
