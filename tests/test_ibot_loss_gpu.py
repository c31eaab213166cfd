"""The fused iBOT patch-loss kernels (csrc/ibot_loss.hip) on the MI355X against tests/ibot_ref.py: the float64 row-paired definition with autograd.

Bounds, as tests/test_dino_loss_gpu.py states them.  Exact operands (all logits 0; one-hot rows at 64 with ts = 1/8, tt = 1/16 and power-of-two
weights): every dS entry and every tsum entry bit for bit.  Random operands: with e32 = max |float32 restatement - float64| on the SAME inputs,
separately for the loss, dS and tsum, the kernel must stay within 4 e32 of float64.  Every test prints its figures as an `ibot_parity` line
(profiles/ibot_loss_parity.txt keeps them)."""
import functools

import pytest
import torch

import ibot_ref
from switch_pairs import install_recorder

pytestmark = pytest.mark.gpu

TS, TT = 0.1, 0.04


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def run(hip, S, T, c, w, ts=TS, tt=TT, g=1.0):
    """S, T [R, K], c [K], w [R] contiguous on the GPU -> loss [1], dS [R, K], tsum [K], s_stats, t_stats"""
    R, K = S.shape
    loss, tsum = torch.empty(1, device="cuda"), torch.empty(K, device="cuda")
    ss, tstat = torch.empty(R, 3, device="cuda"), torch.empty(R, 4, device="cuda")
    hip.ibot_loss_fwd(S, T, c, w, ts, tt, loss, ss, tstat, tsum)
    dS = torch.empty(R, K, device="cuda")
    hip.ibot_loss_bwd(S, T, c, w, ts, tt, ss, tstat, torch.full((1,), g, device="cuda"), dS)
    torch.cuda.synchronize()
    return loss, dS, tsum, ss, tstat


@functools.lru_cache(maxsize=None)
def case(R, K, seed=0, extreme=False, zeros=False):
    """inputs (CPU, float32) and their references, computed once: (S, T, c, w, ts, tt, loss64, dS64, e32 loss, e32 dS, tsum64, e32 tsum)"""
    g = torch.Generator().manual_seed(1000 * (R % 1000) + K + seed)
    S, T, c = 3 * torch.randn(R, K, generator=g), 3 * torch.randn(R, K, generator=g), torch.randn(K, generator=g)
    w = (0.05 + torch.rand(R, generator=g)) / R
    if zeros:  # a third of the weights 0
        w[::3] = 0.0
    ts, tt = TS, TT
    if extreme:  # one row at +1e4 and one at -1e4 in both, tau = 0.04, a centre of +-1e3
        ts = tt = 0.04
        S[0] += 1e4
        S[R - 1] -= 1e4
        T[R - 1] += 1e4
        T[0] -= 1e4
        c = torch.where(torch.rand(K, generator=g) < 0.5, -1e3, 1e3) + c
    l64, d64 = ibot_ref.paired(S, T, c, w, ts, tt, torch.float64)
    l32, d32 = ibot_ref.paired(S, T, c, w, ts, tt, torch.float32)
    t64 = T.double().sum(0)
    e_t = (T.sum(0).double() - t64).abs().max().item()
    return S, T, c, w, ts, tt, l64, d64, abs(l32.double().item() - l64.item()), (d32.double() - d64).abs().max().item(), t64, e_t


def check_case(hip, R, K, **kw):
    S, T, c, w, ts, tt, l64, d64, e_l, e_d, t64, e_t = case(R, K, **kw)
    loss, dS, tsum, _, _ = run(hip, S.cuda(), T.cuda(), c.cuda(), w.cuda(), ts, tt)
    assert torch.isfinite(loss).all() and torch.isfinite(dS).all() and torch.isfinite(tsum).all()
    k_l = abs(loss.double().item() - l64.item())
    k_d = (dS.cpu().double() - d64).abs().max().item()
    k_t = (tsum.cpu().double() - t64).abs().max().item()
    tag = "".join(f" {k}" for k, v in kw.items() if v)
    print(f"ibot_parity R{R} K{K}{tag}: loss {l64.item():.6f} err {k_l:.3e} e32 {e_l:.3e} ratio "
          f"{k_l / e_l if e_l else float('nan'):.2f} | dS err {k_d:.3e} e32 {e_d:.3e} ratio {k_d / e_d if e_d else float('nan'):.2f} | tsum err "
          f"{k_t:.3e} e32 {e_t:.3e} ratio {k_t / e_t if e_t else float('nan'):.2f}")
    assert k_l <= 4 * e_l, f"loss: |kernel - fp64| {k_l:.3e} > 4 e32 = {4 * e_l:.3e}"
    assert k_d <= 4 * e_d, f"dS: |kernel - fp64| {k_d:.3e} > 4 e32 = {4 * e_d:.3e}"
    assert k_t <= 4 * e_t, f"tsum: |kernel - fp64| {k_t:.3e} > 4 e32 = {4 * e_t:.3e}"
    if kw.get("zeros"):
        assert not dS[::3].any(), "a row of weight 0 has a dS row of exact zeros"
    return loss, dS, tsum


# the issue's shapes; the last one is past the grid cap (8193 chunks of 32 rows > 4 * 2048 items): workgroups walk
RANDOM = [(1, 7), (5, 1000), (3, 1024), (3, 1025), (7, 4099), (2, 8192), (8193, 3), (70, 64), (262177, 5)]


@pytest.mark.parametrize("R,K", RANDOM)
def test_random_operands_against_float64(hip, R, K):
    check_case(hip, R, K)


def test_random_operands_with_a_third_of_the_weights_zero(hip):
    check_case(hip, 70, 64, zeros=True)


@pytest.mark.parametrize("R,K", [(5, 1000), (7, 4099)])
def test_extremes(hip, R, K):
    check_case(hip, R, K, extreme=True)


@pytest.mark.parametrize("R", [1, 5, 40])
def test_exact_operands_bit_for_bit(hip, R):
    ts, tt = 0.125, 0.0625
    w = torch.tensor([2.0 ** -(r % 5) for r in range(R)])
    for K in (64, 2048):  # (a) all logits 0, K a power of two: every dS entry exactly 0
        S, T, c = torch.zeros(R, K), torch.zeros(R, K), torch.zeros(K)
        loss, dS, tsum, _, _ = run(hip, S.cuda(), T.cuda(), c.cuda(), w.cuda(), ts, tt)
        assert not dS.any(), f"K {K}: {int((dS != 0).sum())} entries are not 0"
        assert not tsum.any()
        l64, _ = ibot_ref.paired(S, T, c, w, ts, tt, torch.float64)
        l32, _ = ibot_ref.paired(S, T, c, w, ts, tt, torch.float32)
        assert abs(loss.double().item() - l64.item()) <= 4 * abs(l32.double().item() - l64.item())
    for K in (2048, 2050, 1025):  # (b) one-hot rows: 16-byte loads, 4-byte loads, a last tile of one column
        cols = sorted({col for col in (0, 3, 4, 255, 256, 1023, 1024, K - 1) if col < K})
        tp, sp = ibot_ref.peaks(R, K, cols)
        S, T, c = ibot_ref.one_hot_logits(sp, K), ibot_ref.one_hot_logits(tp, K), torch.zeros(K)
        for g in (1.0, 0.25):
            loss, dS, tsum, _, _ = run(hip, S.cuda(), T.cuda(), c.cuda(), w.cuda(), ts, tt, g=g)
            want = ibot_ref.one_hot_grad(tp, sp, w, K, ts, g=g)
            assert torch.equal(dS.cpu(), want), f"K {K}: {int((dS.cpu() != want).sum())} entries differ"
            assert torch.equal(tsum.cpu(), T.sum(0))  # sums of 0 and 64: exact
        l64, _ = ibot_ref.paired(S, T, c, w, ts, tt, torch.float64)
        l32, _ = ibot_ref.paired(S, T, c, w, ts, tt, torch.float32)
        assert abs(loss.double().item() - l64.item()) <= 4 * abs(l32.double().item() - l64.item())


def test_weight_zero_row(hip):
    """R = 40 rows, the LAST of weight 0: the one-block sum adds the rows' terms thread by thread in row order (R <= 256: one row per thread), so
    the zero term is the last addend and the 39-row call adds the same numbers in the same order."""
    R, K = 40, 1025
    S, T, c, w, ts, tt = case(R, K)[:6]
    w = w.clone()
    w[R - 1] = 0.0
    loss, dS, tsum, _, _ = run(hip, S.cuda(), T.cuda(), c.cuda(), w.cuda(), ts, tt)
    assert not dS[R - 1].any() and bool(dS[:R - 1].any(1).all())
    short = run(hip, S[:R - 1].cuda(), T[:R - 1].cuda(), c.cuda(), w[:R - 1].cuda(), ts, tt)
    assert torch.equal(loss, short[0]) and torch.equal(dS[:R - 1], short[1])
    assert (tsum.cpu().double() - T.double().sum(0)).abs().max().item() <= 4 * case(R, K)[11]  # tsum is unweighted: the row still counts
    assert not torch.equal(tsum, short[2])


def guarded(rows, K, ld, fill, G=64, off=0):
    """a [rows, K] view with row stride ld inside a buffer filled with `fill`, G floats of guard before and after (off: the view starts off floats
    later: off = 1 makes its base 4-byte but not 16-byte aligned) -> (buffer, view)"""
    buf = torch.full((G + off + rows * ld + G,), fill, dtype=torch.float32, device="cuda")
    return buf, buf[G + off:G + off + rows * ld].view(rows, ld)[:, :K]


@pytest.mark.parametrize("K,lds,ldt,ldd,off", [(1000, 1008, 1004, 1012, 0),   # 16-byte loads under padding
                                               (1002, 1004, 1008, 1004, 0),   # K % 4 != 0: 4-byte loads
                                               (1000, 1003, 1001, 1002, 0),   # strides off the multiple of 4: 4-byte loads, the bits of the 16-byte dense call
                                               (2052, 2056, 2060, 2052, 0),   # three tiles, the last of four columns
                                               (1000, 1004, 1008, 1004, 1),   # every matrix base 4-byte but not 16-byte aligned: 4-byte loads
                                               (1002, 1002, 1002, 1002, 1)])  # the same, dense rows, K % 4 != 0
def test_padded_layout_has_the_dense_bits_and_touches_nothing_else(hip, K, lds, ldt, ldd, off):
    R = 37  # two chunks, the second of five rows
    S, T, c, w, ts, tt = case(R, K)[:6]
    dense = run(hip, S.cuda(), T.cuda(), c.cuda(), w.cuda(), ts, tt)
    again = run(hip, S.cuda(), T.cuda(), c.cuda(), w.cuda(), ts, tt)
    for a, b in zip(dense, again):
        assert torch.equal(a, b), "two calls differ"
    nan, sent = float("nan"), -7.5
    Sb, Sv = guarded(R, K, lds, nan, off=off)
    Tb, Tv = guarded(R, K, ldt, nan, off=off)
    Sv.copy_(S); Tv.copy_(T)
    cb, cv = guarded(1, K, K, nan, off=off)
    cv.copy_(c)
    db, dv = guarded(R, K, ldd, sent, off=off)
    n_ws = hip.ibot_loss_ws_floats(R, K)
    wb, wv = guarded(1, n_ws, n_ws, sent)
    outs = [guarded(1, n, n, sent) for n in (1, K, 3 * R, 4 * R)]
    keep = [t.clone() for t in (Sb, Tb, cb)]
    loss, tsum, ss, tstat = (o[1].view(-1) for o in outs)
    wd = w.cuda()
    hip.ibot_loss_fwd(Sv, Tv, cv.view(-1), wd, ts, tt, loss, ss.view(R, 3), tstat.view(R, 4), tsum, ws=wv.view(-1))
    hip.ibot_loss_bwd(Sv, Tv, cv.view(-1), wd, ts, tt, ss.view(R, 3), tstat.view(R, 4), torch.ones(1, device="cuda"), dv)
    torch.cuda.synchronize()
    for got, want in zip((loss, dv, tsum, ss, tstat), dense):
        assert torch.equal(got.reshape(-1), want.reshape(-1)), "the padded call's bits differ from the dense call's"
    for before, after in zip(keep, (Sb, Tb, cb)):
        assert torch.equal(before.view(torch.int32), after.view(torch.int32)), "an input buffer was written"
    G = 64
    for buf, n, o_ in [(db, R * ldd, off), (wb, n_ws, 0)] + [(o[0], o[0].numel() - 2 * G, 0) for o in outs]:
        assert bool((buf[:G + o_] == sent).all()) and bool((buf[G + o_ + n:] == sent).all()), "a guard row was written"
    assert bool((db[G + off:G + off + R * ldd].view(R, ldd)[:, K:] == sent).all()), "dS's padding was written"


def test_autograd_function(hip, monkeypatch):
    from diverse_channel_vit_amd import IBOTPatchLoss
    R, K = 5, 1000
    S, T, c, w, ts, tt, l64, d64, e_l, e_d = case(R, K)[:10]
    crit = IBOTPatchLoss(K, student_temp=ts).cuda()
    crit.center.copy_(c)
    grads = []
    for scale in (1.0, 0.5):
        s, t = S.cuda().requires_grad_(True), T.cuda().requires_grad_(True)
        loss = crit(s, t, w.cuda(), tt)
        (scale * loss).backward()
        assert t.grad is None and loss.shape == ()
        grads.append(s.grad)
    assert abs(loss.double().item() - l64.item()) <= 4 * e_l
    assert (grads[0].cpu().double() - d64).abs().max().item() <= 4 * e_d
    normal = (grads[0] * 0.5).abs() >= 2.0 ** -126  # halving is exact wherever the half is a normal number
    assert bool(normal.any()) and torch.equal(grads[1][normal], grads[0][normal] * 0.5)
    assert (grads[1] - grads[0] * 0.5)[~normal].abs().max().item() <= 2.0 ** -126
    log = install_recorder(monkeypatch.setattr)
    with torch.no_grad():
        l2 = crit(S.cuda().requires_grad_(True), T.cuda(), w.cuda(), tt)
    assert l2.grad_fn is None and torch.equal(l2, loss.detach())
    calls = [(n, a) for n, a in log if n.startswith("ibot_")]
    assert [n for n, _ in calls] == ["ibot_loss_fwd"] and calls[0][1]["s_stats"] is None and calls[0][1]["t_stats"] is None
    with pytest.raises(RuntimeError, match="expected torch.float32"):
        crit(S.cuda().bfloat16(), T.cuda(), w.cuda(), tt)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        crit(S, T.cuda(), w.cuda(), tt)
    with pytest.raises(ValueError):
        crit(S.cuda(), T.cuda()[:-1], w.cuda(), tt)


def test_centre(hip):
    from diverse_channel_vit_amd import IBOTPatchLoss
    R, K = 5, 1000
    S, T, c, w, ts, tt = case(R, K)[:6]
    t64, e_t = case(R, K)[10:]
    crit = IBOTPatchLoss(K, student_temp=ts, center_momentum=0.9).cuda()
    crit.center.copy_(c)
    crit(S.cuda(), T.cuda(), w.cuda(), tt)
    torch.cuda.synchronize()
    assert torch.equal(crit.center.cpu(), c), "the centre moved before update_center()"
    tsum = crit._tsum.clone()
    assert (tsum.cpu().double() - t64).abs().max().item() <= 4 * e_t
    crit.update_center()
    assert torch.equal(crit.center, c.cuda() * 0.9 + tsum * ((1.0 - 0.9) / R))
