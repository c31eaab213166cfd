"""The premises of tests/test_gemm_exact_gpu.py, without a GPU: the launch plans restated there (from csrc/gemm_nt.hip and csrc/gemm_tn.hip) against hand-checked
values and the library's host-side answers, every regime the case tables are meant to reach, the exactness condition and the share of
exact bf16 ties on every case's generated inputs, the pads of the padded layouts, and a float32 emulation of the GELU epilogue that
shows where the slack of the one toleranced check comes from.  The library is loaded for its host logic only (tile picks, the 256 x 384
plan, workspace sizes); without a device it plans for 256 compute units, an MI355X's."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gemm_exact_gpu as T  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from diverse_channel_vit_amd import hip
    return hip.load()


def test_constants_and_pads():
    from diverse_channel_vit_amd import hip
    assert (T.EPI_BIAS, T.EPI_GELU, T.EPI_RESID, T.EPI_PLAIN, T.EPI_GELU_BWD, T.EPI_PATCH) == (
        hip.EPI_BIAS_BF16, hip.EPI_BIAS_GELU_BF16, hip.EPI_BIAS_RESID_F32, hip.EPI_PLAIN_BF16, hip.EPI_GELU_BWD_BF16, hip.EPI_PATCH)
    assert (T.TILE_NARROW, T.TILE_WIDE, T.TILE_PAIR, T.TILE_WS, T.TILE_AUTO_WS) == (hip.TILE_NARROW, hip.TILE_WIDE, hip.TILE_PAIR, hip.TILE_WS, hip.TILE_AUTO_WS)
    assert torch.tensor(T.SENT).to(torch.bfloat16).item() == T.SENT  # the sentinel is a bf16 number
    assert all(v == 0 for v in T.PADS["dense"].values())
    assert T.PADS["pad8"]["op"] == 8 and T.PADS["pad72"]["op"] == 72  # the smallest legal pad (rows only 16-byte aligned) and a larger one
    for lay in ("pad8", "pad72"):
        p = T.PADS[lay]
        # include/dcv.h: bf16 strides (and ldo of dcv_gemm_nt_ex, whatever the output type) multiples of 8, fp32 strides of 4
        assert all(p[k] % 8 == 0 and p[k] > 0 for k in ("op", "out", "out2", "f32o", "ln_u")) and all(p[k] % 4 == 0 and p[k] > 0 for k in ("f32r", "y", "ln_o", "ln_r", "dw"))
        # the buffers of one launch differ in their pads: an epilogue that takes one stride for another writes or reads a pad
        for group in (("op", "out", "out2"), ("op", "f32o", "f32r"), ("op", "f32o", "f32r", "y"), ("op", "ln_o", "ln_r", "ln_u"), ("op", "dw")):
            assert len({p[k] for k in group}) == len(group), (lay, group)
    assert T.PADS["pad8"]["ln_o"] == 4 and T.PADS["pad8"]["dw"] == 4 and T.PADS["pad72"]["ln_r"] == 4  # width + 4 where the header allows it


def test_tn_plan_restated(lib):
    """hand-checked values of tn_plan / tn_group_plan, the library's workspace sizes, and every regime of the TN tables"""
    N_, W_ = T.TILE_NARROW, T.TILE_WIDE
    p = T.tn_plan(N_, 4099, 192, 64)
    assert (p.planned, p.mps, p.splits, p.last_rows) == (65, 64, 65, 3)                     # 65 splits of one stage, the last with 3 rows
    p = T.tn_plan(N_, 5000, 384, 384)
    assert (p.tiles, p.planned, p.mps, p.splits) == (9, 56, 128, 40)                        # fewer splits launched than planned
    p = T.tn_plan(N_, 65, 200, 72)
    assert (p.tiles, p.planned, p.mps, p.splits, p.nk_max, p.last_rows) == (2, 2, 64, 2, 1, 1)  # one row in a second split
    p = T.tn_plan(W_, 1000, 384, 128)
    assert (p.planned, p.mps, p.splits, p.nk_max, p.last_rows) == (32, 32, 32, 1, 8)         # one stage per split
    p = T.tn_plan(W_, 333, 384, 1536)
    assert (p.tiles_q, p.planned, p.mps, p.splits, p.nk_max) == (12, 11, 32, 11, 1)          # nk < tiles_q
    p = T.tn_plan(W_, 4099, 1152, 384)
    assert (p.planned, p.mps, p.splits, p.last_rows) == (28, 160, 26, 99)                   # 26 of 28, the last split 3 full stages + 3 rows
    assert T.tn_plan(W_, 100416, 1536, 384).ws_floats == 21 * 1536 * 384 + 21 * 3 * 1536   # tests/test_cabi_cpu.py's figures
    assert T.tn_plan(N_, 100416, 384, 384).ws_floats == 55 * (384 * 384 + 384)
    assert T.tn_group_plan(T.GROUP_ITEMS, 100416)[:3] == (36, 14368, 7)
    for c in T.TN_CASES:
        assert lib.dcv_gemm_tn_pick(c.M, c.P, c.Q, c.tile) == c.tile, c
        assert lib.dcv_gemm_tn_det_ws_floats(c.M, c.P, c.Q, c.tile) == T.tn_plan(c.tile, c.M, c.P, c.Q).ws_floats, c
    for M in T.GROUP_MS:
        arr = (T.TnItem * len(T.GROUP_ITEMS))()
        for it, (P, Q, _) in zip(arr, T.GROUP_ITEMS):
            it.Y = it.X = it.dW = 16  # the size query reads shapes only
            it.ldy, it.ldx, it.P, it.Q, it.lddw = P, Q, P, Q, Q
        assert lib.dcv_gemm_tn_group_ws_floats(C.cast(arr, C.c_void_p), len(T.GROUP_ITEMS), M) == T.tn_group_plan(T.GROUP_ITEMS, M)[3], M
    # regimes: (name, predicate) — each must hold for a row of BOTH tables unless it exists on one tile only
    plans = {c: T.tn_plan(c.tile, c.M, c.P, c.Q) for c in T.TN_CASES}
    ring = {N_: 2, W_: 4}  # csrc/gemm_tn.hip: gemm_tn_kernel double-buffers, T3_STAGES = 4
    regimes = {
        "ragged last stage": lambda c, p: p.last_rows % p.stage != 0,
        "last split shorter than the others": lambda c, p: p.splits > 1 and p.last_rows < p.mps,
        "fewer splits launched than planned": lambda c, p: p.splits < p.planned,
        "fewer rows than one stage": lambda c, p: c.M < p.stage,
        "more stages than the ring is deep": lambda c, p: p.nk_max > ring[c.tile],
        "partial tiles": lambda c, p: c.tile == N_ and c.P % 128 and c.Q % 128,
    }
    for name, pred in regimes.items():
        for tile in (N_, W_):
            if name == "partial tiles" and tile == W_:
                continue
            assert any(pred(c, p) for c, p in plans.items() if c.tile == tile), f"no row of the {'narrow' if tile == N_ else 'wide'} TN table has: {name}"
    assert any(c.tile == W_ and p.nk_max < ring[W_] and p.splits > 1 for c, p in plans.items()), "fewer stages than the ring depth"
    assert any(c.tile == W_ and p.nk_max < p.tiles_q for c, p in plans.items()), "nk < tiles_q: the bias sum falls to tq = 0 alone"
    assert {c.M for c in T.TN_WIDE} >= {31, 32, 33}  # around one stage
    # the grouped launch: fewer rows than a stage, ragged ends, a last split shorter than the others
    g = {M: T.tn_group_plan(T.GROUP_ITEMS, M) for M in T.GROUP_MS}
    assert g[31][1:3] == (32, 1) and g[5000][1:3] == (736, 7) and g[64 * 197 + 5][1:3] == (1824, 7)
    assert all(t[0] == 36 for t in g.values()) and 5000 - 6 * 736 < 736 and (5000 - 6 * 736) % 32 and (12613 - 6 * 1824) % 32


def test_nt_tables_hold_their_regimes(lib):
    """each row of the NT tables reaches the regime it is listed for, by the restated walks and the library's host logic"""
    w = {(c.M, c.N, c.K, c.cap): T.nt_walk(c.tile, c.M, c.N, c.K, c.cap) for c in T.NT_NARROW}
    assert w[(1, 8, 64, 0)] == (1, 1, 1, 1, 1, 1)
    assert w[(300, 384, 384, 0)][:4] == (2, 3, 6, 1) and 300 % 256                                       # partial M tile
    assert w[(777, 200, 64, 3)] == (4, 2, 3, 3, 2, 1) and 200 % 128                                      # partial N tile, one stage, a short third round
    assert w[(1100, 392, 1536, 4)] == (5, 4, 4, 5, 4, 24) and 392 % 128 == 8                             # 24 stages, an 8-column last tile, five rounds
    w = {(c.M, c.N, c.K, c.cap): T.nt_walk(c.tile, c.M, c.N, c.K, c.cap) for c in T.NT_PAIR}
    assert w[(1, 8, 64, 0)] == (1, 1, 1, 1, 1, 1) and w[(300, 384, 384, 0)][:4] == (3, 3, 9, 1)
    assert w[(777, 200, 64, 2)] == (7, 2, 4, 4, 2, 1) and w[(1100, 392, 1536, 3)] == (9, 4, 6, 6, 6, 24)
    for c in T.NT_WIDE:
        tiles = T._cdiv(c.M, 256) * (c.N // 384)
        a, b = C.c_int(-1), C.c_int(-1)
        assert lib.dcv_gemm_nt384_plan(c.M, c.N, min(tiles, c.cap) if c.cap else tiles, C.byref(a), C.byref(b)) == 0
        assert (b.value > 0) == T.NT_WIDE_MIXED[(c.M, c.N, c.cap)], (c, a.value, b.value)
    assert sum(T.NT_WIDE_MIXED.values()) == 3
    assert T._cdiv(T._cdiv(2900, 256) * 1, 3) == 4 and T._cdiv(300, 256) * 1 <= T.CUS                     # four rounds; one round
    w = {(c.M, c.N, c.cap): T.ws_walk(c.M, c.N, c.cap) for c in T.NT_WS}
    assert w[(1, 384, 0)] == (1, 1, 1, 1, 1)
    assert w[(95, 1152, 4)] == (3, 3, 1, 3, 31)                                                          # one group of three slices, a 31-row last panel
    assert w[(1000, 1536, 7)] == (4, 32, 1, 32, 8)                                                       # 32 panels through a ring of 6 (3)
    assert w[(4100, 384, 3)] == (1, 129, 3, 43, 4)                                                       # three groups
    assert w[(8200, 384, 0)][2] == 256
    for c in T.NT_CASES:
        want = T.TILE_WS if c.tile == T.TILE_AUTO_WS else c.tile
        assert all(lib.dcv_gemm_nt_pick(c.M, c.N, c.K, e, c.tile) == want for e in (T.EPI_BIAS, T.EPI_GELU, T.EPI_PLAIN, T.EPI_GELU_BWD)), c
        assert c.cap == 0 or want != T.TILE_WS or c.cap >= c.N // 384
    assert any(c.tile == T.TILE_AUTO_WS and c.M >= T.WS_M_MIN for c in T.NT_WS)
    for c in T.NT_NARROW:
        B, Cc, n = T.PATCH_SPLIT[c.M]
        assert B * Cc * n == c.M
    assert [T.samples_of(c.M)[0] for c in T.NT_NARROW + T.NT_WIDE] == [1, 5, 3, 5, 5, 5, 5, 1, 5]
    assert {(c.M, c.K, c.cap) for c in T.LN_CASES} == {(300, 384, 0), (1500, 384, 4), (2100, 1536, 3), (777, 64, 3)}


def _nt_problems():
    return sorted({(c.M, c.N, c.K) for c in T.NT_CASES} | {(c.M, 384, c.K) for c in T.LN_CASES})


@pytest.mark.parametrize("M,N,K", _nt_problems())
def test_nt_inputs_are_exact_and_pin_the_rounding(M, N, K):
    """the exactness condition from the inputs' own extremes, every operand a bf16 number, the accumulator within 16 bits, and at least
    2 % exact bf16 ties among the reference outputs of every case with 10^4 outputs or more"""
    h = T.nt_inputs(M, N, K)
    A, W, bias, resid, acc = h["A"], h["W"], h["bias"], h["resid"], h["acc"]
    for t in (A, W, h["gp"]):
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    assert torch.equal(A, A.round()) and torch.equal(W, W.round()) and torch.equal(2 * bias, (2 * bias).round()) and torch.equal(2 * resid, (2 * resid).round())
    amax, wmax, bmax, rmax = (t.abs().max().item() for t in (A, W, bias, resid))
    assert amax <= 8 and wmax <= 8 and bmax <= 8 and rmax <= 32
    T.assert_exact("resid + s (acc + bias)", K, amax, wmax, 0.125, extra=max(T.FACTORS) * bmax + rmax, factor=max(T.FACTORS))
    T.assert_exact("z = acc / 256 + bias", K, amax, wmax / 256, 1 / 256, extra=bmax)
    assert torch.equal(acc.double(), A.double() @ W.double().t())  # the fp32 product on the CPU is itself exact
    assert acc.abs().max().item() < 2 ** 16  # GELU_BWD: 16 significant bits times a bf16's 8 fit fp32's 24
    assert torch.equal((acc.double() * h["gp"].double()).float().double(), acc.double() * h["gp"].double())
    if M * N >= 10 ** 4:
        for name, ref in (("PLAIN_BF16", acc), ("BIAS_BF16", acc + bias)):
            assert T.tie_share(ref) >= 0.02, f"{name}: {T.tie_share(ref):.2%} exact ties"


def test_tn_inputs_are_exact():
    for c in T.TN_CASES:
        h = T.tn_inputs(c.M, c.P, c.Q)
        assert all(torch.equal(h[k].to(torch.bfloat16).float(), h[k]) and torch.equal(h[k], h[k].round()) for k in ("Y", "X"))
        assert torch.equal(h["dW0"], h["dW0"].round()) and torch.equal(h["db0"], h["db0"].round())
        T.assert_exact("dW", c.M, h["Y"].abs().max().item(), h["X"].abs().max().item(), 1.0, extra=max(h["dW0"].abs().max().item(), h["db0"].abs().max().item()))
    assert max(c.M for c in T.TN_CASES) <= max(T.GROUP_MS) == 12613 and 64 * 12613 + 100 < 2 ** 24


def test_tie_share_and_ulp_helpers():
    x = torch.tensor([255.0, 257.0, 259.0, 258.0, 513.0, 514.0, 128.5, 0.5, -1027.0, -1028.0], dtype=torch.float64)
    ties = [False, True, True, False, False, True, True, False, False, True]
    assert T.tie_share(x) == sum(ties) / len(ties)
    assert [T.tie_share(v.reshape(1)) == 1.0 for v in x] == ties
    # ties go to the even neighbour: 257 -> 256, 259 -> 260
    assert T.to_out(x[1:3], torch.bfloat16).tolist() == [256.0, 260.0]
    u = T.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.75, -300.0, 0.0, 1e-45], dtype=torch.float64))
    assert u.tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0, 2.0 ** -133, 2.0 ** -133]


def _gelu_parts2_f32(z):
    """csrc/gemm_nt.hip gelu_parts2 in float32: every multiply-add one fused operation (-ffp-contract=fast), rcp and exp2 rounded correctly
    (the hardware's are within 1 ulp)"""
    f = np.float32

    def fma(a, b, c):
        return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f)  # fp32 products are exact in float64

    d = fma(np.abs(z), f(0.23164189), f(1.0))
    t = (f(1.0) / d).astype(f)
    zz = (z * z).astype(f) * f(-0.72134752044448170)
    e = np.exp2(zz.astype(np.float64)).astype(f)
    poly = fma(t, f(1.061405429), f(-1.453152027))
    for c in (1.421413741, -0.284496736, 0.254829592):
        poly = fma(poly, t, f(c))
    poly = (poly * t).astype(f)
    h = fma((poly * e).astype(f), f(-0.5), f(0.5))
    cdf = (np.copysign(h, z) + f(0.5)).astype(f)
    return (z * cdf).astype(f), fma((z * e).astype(f), f(0.39894228040143268), cdf)


def test_gelu_epilogue_emulation_bounds_the_slack():
    """Where the 1e-6 max(1, |z|) of test_nt_bias_gelu_within_half_ulp comes from: a float32 emulation of gelu_parts2 over the grid of z
    the test produces (steps of 2^-8, |z| <= 12) against the float64 erf-GELU.  GELU stays within 1.42e-7 max(1, |z|); the derivative
    within 2.6e-7 = 7.5e-8 (half of Abramowitz-Stegun 7.1.26's 1.5e-7 on erf) + three half-ulps of numbers in [1, 2) (cdf, the final
    multiply-add, the polynomial's last product: 6e-8 each) — measured 1.87e-7.  Both leave the GPU test's bound a factor of four for the
    hardware's 1-ulp rcp / exp2."""
    z = (np.arange(-12 * 256, 12 * 256 + 1) / 256).astype(np.float32)
    g, gp = _gelu_parts2_f32(z)
    g64, gp64 = T.gelu64(torch.from_numpy(z.astype(np.float64)))
    scale = np.maximum(1.0, np.abs(z.astype(np.float64)))
    eg = (np.abs(g.astype(np.float64) - g64.numpy()) / scale).max()
    egp = (np.abs(gp.astype(np.float64) - gp64.numpy()) / scale).max()
    assert eg <= 1.42e-7, eg
    assert egp <= 2.6e-7, egp
    assert max(eg, egp) * 3 < T.GELU_SLACK
