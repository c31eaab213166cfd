"""The fused DINO loss kernels (csrc/dino_loss.hip) on the MI355X against tests/dino_ref.py: the float64 pairwise definition with autograd.

Bounds.  Exact operands (all logits 0; one-hot rows at 64 with ts = 1/8, tt = 1/16, n B ts a power of two): every dS entry bit for bit.  Random
operands: with e32 = max |float32 pairwise restatement - float64| on the SAME inputs, separately for the loss, dS and tsum, the kernel must stay
within 4 e32 of float64 — both are float32 evaluations of the same K-term sums in other association orders and with other exponentials, and the
factor 4 is the margin for that alone.  Every test prints its figures as a `dino_parity` line (profiles/dino_loss_parity.txt keeps them)."""
import functools

import pytest
import torch

import dino_ref
from switch_pairs import install_recorder

pytestmark = pytest.mark.gpu

TS, TT = 0.1, 0.04
SEAM_COLS = lambda K: sorted({c for c in (0, K - 1, 3, 4, 255, 256, 1023, 1024, 2047, 2048) if 0 <= c < K})  # noqa: E731


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def run(hip, S, T, c, ts=TS, tt=TT, g=1.0):
    """S [V, B, K], T [2, B, K], c [K] contiguous on the GPU -> loss [1], dS [V, B, K], tsum [K], s_stats, t_stats"""
    V, B, K = S.shape
    S2, T2 = S.view(V * B, K), T.view(2 * B, K)
    loss, tsum = torch.empty(1, device="cuda"), torch.empty(K, device="cuda")
    ss, tstat = torch.empty(V * B, 2, device="cuda"), torch.empty(2 * B, 3, device="cuda")
    hip.dino_loss_fwd(S2, T2, c, V, ts, tt, loss, ss, tstat, tsum)
    dS = torch.empty(V * B, K, device="cuda")
    hip.dino_loss_bwd(S2, T2, c, V, ts, tt, ss, tstat, torch.full((1,), g, device="cuda"), dS)
    torch.cuda.synchronize()
    return loss, dS.view(V, B, K), tsum, ss, tstat


@functools.lru_cache(maxsize=None)
def case(V, B, K, seed=0, extreme=False):
    """inputs (CPU, float32) and their references, computed once: (S, T, c, ts, tt, loss64, dS64, e32 loss, e32 dS, tsum64, e32 tsum)"""
    g = torch.Generator().manual_seed(1000 * V + 10 * B + K + seed)
    S, T, c = 3 * torch.randn(V, B, K, generator=g), 3 * torch.randn(2, B, K, generator=g), torch.randn(K, generator=g)
    ts, tt = TS, TT
    if extreme:  # one row at +1e4 and one at -1e4 in both, tau = 0.04, a centre of +-1e3
        ts = tt = 0.04
        S[0, 0] += 1e4
        S[V - 1, B - 1] -= 1e4
        T[0, B - 1] += 1e4
        T[1, 0] -= 1e4
        c = torch.where(torch.rand(K, generator=g) < 0.5, -1e3, 1e3) + c
    l64, d64 = dino_ref.pairwise(S, T, c, ts, tt, torch.float64)
    l32, d32 = dino_ref.pairwise(S, T, c, ts, tt, torch.float32)
    t64 = T.double().sum((0, 1))
    e_t = (T.flatten(0, 1).sum(0).double() - t64).abs().max().item()
    return S, T, c, ts, tt, l64, d64, abs(l32.double().item() - l64.item()), (d32.double() - d64).abs().max().item(), t64, e_t


def check_case(hip, V, B, K, **kw):
    S, T, c, ts, tt, l64, d64, e_l, e_d, t64, e_t = case(V, B, K, **kw)
    loss, dS, tsum, _, _ = run(hip, S.cuda(), T.cuda(), c.cuda(), ts, tt)
    assert torch.isfinite(loss).all() and torch.isfinite(dS).all() and torch.isfinite(tsum).all()
    k_l = abs(loss.double().item() - l64.item())
    k_d = (dS.cpu().double() - d64).abs().max().item()
    k_t = (tsum.cpu().double() - t64).abs().max().item()
    print(f"dino_parity V{V} B{B} K{K}{' extreme' if kw.get('extreme') else ''}: loss {l64.item():.6f} err {k_l:.3e} e32 {e_l:.3e} ratio "
          f"{k_l / e_l if e_l else float('nan'):.2f} | dS err {k_d:.3e} e32 {e_d:.3e} ratio {k_d / e_d if e_d else float('nan'):.2f} | tsum err "
          f"{k_t:.3e} e32 {e_t:.3e} ratio {k_t / e_t if e_t else float('nan'):.2f}")
    assert k_l <= 4 * e_l, f"loss: |kernel - fp64| {k_l:.3e} > 4 e32 = {4 * e_l:.3e}"
    assert k_d <= 4 * e_d, f"dS: |kernel - fp64| {k_d:.3e} > 4 e32 = {4 * e_d:.3e}"
    assert k_t <= 4 * e_t, f"tsum: |kernel - fp64| {k_t:.3e} > 4 e32 = {4 * e_t:.3e}"


# the issue's shapes, then one on each seam of the plan: one column tile | two (1024 | 1025), past the grid cap of 2048 workgroups of four items
RANDOM = [(2, 1, 7), (3, 3, 1000), (10, 4, 4099), (10, 4, 65536), (2, 64, 64), (2, 1, 1024), (3, 2, 1025), (2, 8193, 3)]


@pytest.mark.parametrize("V,B,K", RANDOM)
def test_random_operands_against_float64(hip, V, B, K):
    check_case(hip, V, B, K)


@pytest.mark.parametrize("V,B,K", [(3, 3, 1000), (10, 4, 4099)])
def test_extremes(hip, V, B, K):
    check_case(hip, V, B, K, extreme=True)


@pytest.mark.parametrize("V", [2, 3, 5, 9])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_exact_operands_bit_for_bit(hip, V, B):
    ts, tt = 0.125, 0.0625
    for K in (64, 2048):  # (a) all logits 0, K a power of two: every dS entry exactly 0
        S, T, c = torch.zeros(V, B, K), torch.zeros(2, B, K), torch.zeros(K)
        loss, dS, tsum, _, _ = run(hip, S.cuda(), T.cuda(), c.cuda(), ts, tt)
        assert not dS.any(), f"K {K}: {int((dS != 0).sum())} entries are not 0"
        assert not tsum.any()
        l64, _ = dino_ref.pairwise(S, T, c, ts, tt, torch.float64)
        l32, _ = dino_ref.pairwise(S, T, c, ts, tt, torch.float32)
        assert abs(loss.double().item() - l64.item()) <= 4 * abs(l32.double().item() - l64.item())
    for K in (2048, 2050, 1025):  # (b) one-hot rows: 16-byte loads, 4-byte loads, a last tile of one column
        tp, sp = dino_ref.peaks(V, B, K, SEAM_COLS(K))
        S, T, c = dino_ref.one_hot_logits(sp, K), dino_ref.one_hot_logits(tp, K), torch.zeros(K)
        loss, dS, tsum, _, _ = run(hip, S.cuda(), T.cuda(), c.cuda(), ts, tt)
        want = dino_ref.one_hot_grad(tp, sp, K, ts)
        assert torch.equal(dS.cpu(), want), f"K {K}: {int((dS.cpu() != want).sum())} entries differ"
        assert torch.equal(tsum.cpu(), T.sum((0, 1)))  # sums of 0 and 64: exact
        l64, _ = dino_ref.pairwise(S, T, c, ts, tt, torch.float64)
        l32, _ = dino_ref.pairwise(S, T, c, ts, tt, torch.float32)
        assert abs(loss.double().item() - l64.item()) <= 4 * abs(l32.double().item() - l64.item())


def guarded(rows, K, ld, fill, G=64, off=0):
    """a [rows, K] view with row stride ld inside a buffer filled with `fill`, G floats of guard before and after (off: the view starts off floats
    later: off = 1 makes its base 4-byte but not 16-byte aligned) -> (buffer, view)"""
    buf = torch.full((G + off + rows * ld + G,), fill, dtype=torch.float32, device="cuda")
    return buf, buf[G + off:G + off + rows * ld].view(rows, ld)[:, :K]


@pytest.mark.parametrize("K,lds,ldt,ldd,off", [(1000, 1008, 1004, 1012, 0),   # 16-byte loads under padding
                                               (999, 1002, 1001, 1003, 0),    # K % 4 != 0: 4-byte loads
                                               (1000, 1003, 1001, 1002, 0),   # strides off the multiple of 4: 4-byte loads, the bits of the 16-byte dense call
                                               (2052, 2056, 2060, 2052, 0),   # three tiles, the last of four columns
                                               (1000, 1004, 1008, 1004, 1),   # every matrix base 4-byte but not 16-byte aligned: 4-byte loads
                                               (1000, 1000, 1000, 1000, 1)])  # the same, dense rows
def test_padded_layout_has_the_dense_bits_and_touches_nothing_else(hip, K, lds, ldt, ldd, off):
    V, B = 3, 2
    S, T, c, ts, tt = case(V, B, K)[:5]
    dense = run(hip, S.cuda(), T.cuda(), c.cuda(), ts, tt)
    again = run(hip, S.cuda(), T.cuda(), c.cuda(), ts, tt)
    for a, b in zip(dense, again):
        assert torch.equal(a, b), "two calls differ"
    nan, sent = float("nan"), -7.5
    Sb, Sv = guarded(V * B, K, lds, nan, off=off)
    Tb, Tv = guarded(2 * B, K, ldt, nan, off=off)
    Sv.copy_(S.view(V * B, K)); Tv.copy_(T.view(2 * B, K))
    cb, cv = guarded(1, K, K, nan, off=off)
    cv.copy_(c)
    db, dv = guarded(V * B, K, ldd, sent, off=off)
    n_ws = hip.dino_loss_ws_floats(V, B, K)
    wb, wv = guarded(1, n_ws, n_ws, sent)
    outs = [guarded(1, n, n, sent) for n in (1, K, 2 * V * B, 6 * B)]
    keep = [t.clone() for t in (Sb, Tb, cb)]
    loss, tsum, ss, tstat = (o[1].view(-1) for o in outs)
    hip.dino_loss_fwd(Sv, Tv, cv.view(-1), V, ts, tt, loss, ss.view(V * B, 2), tstat.view(2 * B, 3), tsum, ws=wv.view(-1))
    hip.dino_loss_bwd(Sv, Tv, cv.view(-1), V, ts, tt, ss.view(V * B, 2), tstat.view(2 * B, 3), torch.ones(1, device="cuda"), dv)
    torch.cuda.synchronize()
    for got, want in zip((loss, dv, tsum, ss, tstat), dense):
        assert torch.equal(got.reshape(-1), want.reshape(-1)), "the padded call's bits differ from the dense call's"
    for before, after in zip(keep, (Sb, Tb, cb)):
        assert torch.equal(before.view(torch.int32), after.view(torch.int32)), "an input buffer was written"
    G = 64
    for buf, n, o_ in [(db, V * B * ldd, off), (wb, n_ws, 0)] + [(o[0], o[0].numel() - 2 * G, 0) for o in outs]:
        assert bool((buf[:G + o_] == sent).all()) and bool((buf[G + o_ + n:] == sent).all()), "a guard row was written"
    assert bool((db[G + off:G + off + V * B * ldd].view(V * B, ldd)[:, K:] == sent).all()), "dS's padding was written"


def test_autograd_function(hip, monkeypatch):
    from diverse_channel_vit_amd import DINOLoss
    V, B, K = 3, 3, 1000
    S, T, c, ts, tt, l64, d64, e_l, e_d = case(V, B, K)[:9]
    crit = DINOLoss(K, student_temp=ts).cuda()
    crit.center.copy_(c)
    grads = []
    for scale in (1.0, 0.5):
        s = S.view(V * B, K).cuda().requires_grad_(True)
        t = T.view(2 * B, K).cuda().requires_grad_(True)
        loss = crit(s, t, tt, n_views=V)
        (scale * loss).backward()
        assert t.grad is None and loss.shape == ()
        grads.append(s.grad)
    assert abs(loss.double().item() - l64.item()) <= 4 * e_l
    assert (grads[0].cpu().double().view(V, B, K) - d64).abs().max().item() <= 4 * e_d
    normal = (grads[0] * 0.5).abs() >= 2.0 ** -126  # halving is exact wherever the half is a normal number; a subnormal half rounds or flushes
    assert bool(normal.any()) and torch.equal(grads[1][normal], grads[0][normal] * 0.5)
    assert (grads[1] - grads[0] * 0.5)[~normal].abs().max().item() <= 2.0 ** -126
    log = install_recorder(monkeypatch.setattr)
    with torch.no_grad():
        l2 = crit(S.view(V * B, K).cuda().requires_grad_(True), T.view(2 * B, K).cuda(), tt, n_views=V)
    assert l2.grad_fn is None and torch.equal(l2, loss.detach())
    calls = [(n, a) for n, a in log if n.startswith("dino_")]
    assert [n for n, _ in calls] == ["dino_loss_fwd"] and calls[0][1]["s_stats"] is None and calls[0][1]["t_stats"] is None
    with pytest.raises(RuntimeError, match="expected torch.float32"):
        crit(S.view(V * B, K).cuda().bfloat16(), T.view(2 * B, K).cuda(), tt, n_views=V)
    with pytest.raises(ValueError):
        crit(S.view(V * B, K).cuda(), T.view(2 * B, K).cuda(), tt, n_views=2)


def test_centre(hip):
    from diverse_channel_vit_amd import DINOLoss
    V, B, K = 3, 3, 1000
    S, T, c, ts, tt = case(V, B, K)[:5]
    t64, e_t = case(V, B, K)[9:]
    crit = DINOLoss(K, student_temp=ts, center_momentum=0.9).cuda()
    crit.center.copy_(c)
    crit(S.view(V * B, K).cuda(), T.view(2 * B, K).cuda(), tt, n_views=V)
    torch.cuda.synchronize()
    assert torch.equal(crit.center.cpu(), c), "the centre moved before update_center()"
    tsum = crit._tsum.clone()
    assert (tsum.cpu().double() - t64).abs().max().item() <= 4 * e_t
    crit.update_center()
    assert torch.equal(crit.center, c.cuda() * 0.9 + tsum * ((1.0 - 0.9) / (2 * B)))
    assert (crit.center.cpu().double() - (0.9 * c.double() + 0.1 * t64 / (2 * B))).abs().max().item() <= 1e-6
