"""The 256 x 384 NT GEMM on its balanced tile plan (dcv_gemm_nt384_plan: 192-row tiles in the last rounds): small problems under a grid cap, so
that a few workgroups walk rounds of both heights.  A tile's height changes neither the MFMA, nor the k order, nor the lane-to-column map, so
every output must be bit-identical (torch.equal) to the 256 x 128 kernel's, and the residual + LayerNorm entry's to its own one-round launch
(grid_cap = 0: every tile 256 rows high).  Each mixed case first asserts through the plan entry that 192-row tiles are in play.

Two of the shapes listed for this test cannot take a mixed plan: (1100, 1152, cap 8) — 15 tiles in two rounds leave room for 5 row tiles, which
cover 1100 rows only with three or more of 256 rows, and workgroup 0's second tile (tile 8 = row tile 2) is then still 256 rows high — and
(2900, 384, cap 3) — 12 tiles in four rounds, and 9 x 256 + 3 x 192 = 2880 < 2900.  The plan must answer n192 = 0 there (it may only change a
walk it shortens); they stay as bit-identity cases with that asserted, and (1100, 1152, cap 6) / (2100, 384, cap 3) stand in for what they were
meant to cover: three column tiles and three rounds on a mixed plan.  Needs an MI355X: run with -m gpu."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, N, K, grid cap, 192-row tiles expected)
SHAPES = [
    (1500, 384, 384, 4, True),
    (1500, 384, 1536, 4, True),
    (1217, 384, 1536, 4, True),
    (1408, 384, 64, 4, True),     # one k stage
    (1100, 1152, 384, 8, False),  # three column tiles; see the module docstring
    (2900, 384, 1536, 3, False),  # four rounds; see the module docstring
    (1100, 1152, 384, 6, True),   # three column tiles, 18 tiles of 192 rows in three rounds
    (2100, 384, 1536, 3, True),   # three rounds: 256, 256, 192
    (1153, 384, 384, 4, True),    # one row in the last 192-row tile
    (2624, 384, 384, 4, True),    # 8 x 256 + 3 x 192 rows: covered exactly, the last tile full
    (1000, 1152, 384, 8, True),   # (2, 3): six 256-row and two 192-row tiles share round 0
]
LN_SHAPES = [(1500, 384, 4, True), (1500, 1536, 4, True), (1217, 1536, 4, True), (2900, 384, 3, False), (2100, 1536, 3, True), (1153, 384, 4, True)]


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def _plan(hip, M, N, cap):
    """(n256, n192) of the launch dcv_gemm_nt_ex / dcv_gemm_nt_resid_ln make: the grid is min(256-row tiles, cap)"""
    tiles = -(-M // 256) * (N // 384)
    a, b = C.c_int(-1), C.c_int(-1)
    assert hip.load().dcv_gemm_nt384_plan(M, N, min(tiles, cap) if cap else tiles, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).cuda()


def _f(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _assert_plan(hip, M, N, cap, mixed):
    n256, n192 = _plan(hip, M, N, cap)
    if mixed:
        assert n192 > 0, f"M {M} N {N} cap {cap}: the plan has no 192-row tile ({n256}, {n192}) — the new path would not run"
    else:
        assert (n256, n192) == (-(-M // 256), 0), f"M {M} N {N} cap {cap}: no mixed plan shortens this walk, got ({n256}, {n192})"


@pytest.mark.parametrize("M,N,K,cap,mixed", SHAPES)
def test_balanced_plain_and_bias_match_narrow(hip, M, N, K, cap, mixed):
    _assert_plan(hip, M, N, cap, mixed)
    A, W, bias = _bf(M, K, seed=1), _bf(N, K, scale=0.05, seed=2), _f(N, scale=0.1, seed=3)
    for epi in (hip.EPI_PLAIN_BF16, hip.EPI_BIAS_BF16):
        out = {}
        for tile, c in ((hip.TILE_WIDE, cap), (hip.TILE_NARROW, 0)):
            out[tile] = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
            hip.gemm_nt(A, W, epi, out[tile], bias=bias, tile=tile, grid_cap=c)
        assert not torch.isnan(out[hip.TILE_WIDE].float()).any(), f"epilogue {epi}: rows or columns left unwritten"
        assert torch.equal(out[hip.TILE_WIDE], out[hip.TILE_NARROW]), f"epilogue {epi}: the balanced wide tile differs from the narrow tile"


@pytest.mark.parametrize("M,N,K,cap,mixed", SHAPES)
def test_balanced_bias_resid_branch_scale_matches_narrow(hip, M, N, K, cap, mixed):
    """EPI_BIAS_RESID_F32 with a per-sample branch scale (stochastic depth), out of place"""
    _assert_plan(hip, M, N, cap, mixed)
    A, W, bias = _bf(M, K, seed=1), _bf(N, K, scale=0.05, seed=2), _f(N, scale=0.1, seed=3)
    resid = _f(M, N, seed=4)
    samples = 4 if M % 4 == 0 else 1
    scale = torch.tensor([1.0, 0.0, 2.0, 1.25][:samples], device="cuda")
    out = {}
    for tile, c in ((hip.TILE_WIDE, cap), (hip.TILE_NARROW, 0)):
        out[tile] = torch.full((M, N), float("nan"), device="cuda")
        hip.gemm_nt(A, W, hip.EPI_BIAS_RESID_F32, out[tile], bias=bias, aux=resid, aux2=scale, T=M // samples, tile=tile, grid_cap=c)
    assert not torch.isnan(out[hip.TILE_WIDE]).any()
    assert torch.equal(out[hip.TILE_WIDE], out[hip.TILE_NARROW])


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("M,K,cap,mixed", LN_SHAPES)
def test_balanced_resid_ln_matches_one_round(hip, M, K, cap, mixed, with_scale):
    """gemm_nt_resid_ln under the cap (mixed rounds) against the same call with grid_cap = 0 (one round of 256-row tiles): x', u, mean, rstd"""
    N = 384
    _assert_plan(hip, M, N, cap, mixed)
    assert _plan(hip, M, N, 0)[1] == 0  # the reference launch: one round, the old plan
    A, W = _bf(M, K, seed=1), _bf(N, K, scale=0.05, seed=2)
    bias, gamma, beta = _f(N, scale=0.1, seed=3), 1.0 + _f(N, scale=0.2, seed=6), _f(N, scale=0.3, seed=7)
    x0 = _f(M, N, seed=4) * 3.0 + 5.0
    samples = 4 if M % 4 == 0 else 1
    kw = dict(branch_scale=torch.tensor([1.0, 0.0, 2.0, 1.25][:samples], device="cuda"), T=M // samples) if with_scale else {}
    got = {}
    for c in (cap, 0):
        x_out = torch.full_like(x0, float("nan"))
        u = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
        mean, rstd = torch.full((M,), float("nan"), device="cuda"), torch.full((M,), float("nan"), device="cuda")
        hip.gemm_nt_resid_ln(A, W, bias, x0, x_out, gamma, beta, 1e-6, u, mean, rstd, grid_cap=c, **kw)
        got[c] = (x_out, u, mean, rstd)
    for name, a, b in zip(("x_out", "u", "mean", "rstd"), got[cap], got[0]):
        assert not torch.isnan(a.float()).any(), f"{name}: rows left unwritten"
        assert torch.equal(a, b), f"{name}: the capped (mixed-round) launch differs from the one-round launch"


def test_plan_does_not_engage_in_one_round(hip):
    """(1000, 384, 384), no cap: four tiles on one round — the old plan, and the same bits as the narrow tile"""
    M, N, K = 1000, 384, 384
    assert _plan(hip, M, N, 0) == (4, 0)
    A, W = _bf(M, K, seed=1), _bf(N, K, scale=0.05, seed=2)
    wide, narrow = (torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(2))
    hip.gemm_nt(A, W, hip.EPI_PLAIN_BF16, wide, tile=hip.TILE_WIDE)
    hip.gemm_nt(A, W, hip.EPI_PLAIN_BF16, narrow, tile=hip.TILE_NARROW)
    assert torch.equal(wide, narrow)
