"""The weight-stationary NT GEMM (DCV_TILE_WS, gemm_nt_ws_kernel) against the tiled kernels: the same MFMA, operand orientation and
k order, so its outputs must be bit-identical to TILE_WIDE's (and TILE_NARROW's), for the four bf16-output epilogues it serves.
Needs an MI355X: run with -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HEADLINE_M = 64 * 1569


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).cuda()


def _f(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _run(hip, epi, A, W, bias, aux, tile, grid_cap=0):
    M, N = A.shape[0], W.shape[0]
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    out2 = torch.full_like(out, float("nan")) if epi == hip.EPI_BIAS_GELU_BF16 else None
    hip.gemm_nt(A, W, epi, out, bias=bias, out2=out2, aux=aux, tile=tile, grid_cap=grid_cap)
    return out, out2


def _same(hip, M, N, refs, grid_cap=0, seed=0):
    A, W = _bf(M, 384, seed=1 + seed), _bf(N, 384, scale=0.05, seed=2 + seed)
    bias = _f(N, scale=0.1, seed=3 + seed)
    aux = _bf(M, N, seed=4 + seed)
    for epi in (hip.EPI_BIAS_BF16, hip.EPI_BIAS_GELU_BF16, hip.EPI_PLAIN_BF16, hip.EPI_GELU_BWD_BF16):
        o, o2 = _run(hip, epi, A, W, bias, aux, hip.TILE_WS, grid_cap)
        for ref_tile in refs:
            r, r2 = _run(hip, epi, A, W, bias, aux, ref_tile)
            assert torch.equal(o, r), f"M {M} N {N} epi {epi} cap {grid_cap}: differs from tile {ref_tile}"
            if o2 is not None:
                assert torch.equal(o2, r2), f"M {M} N {N} epi {epi} cap {grid_cap}: out2 differs from tile {ref_tile}"


@pytest.mark.parametrize("N", [1152, 1536, 384])
def test_ws_headline_bit_identical(hip, N):
    """M = 100 416 (the headline step's rows) at the three widths of the K = 384 products."""
    _same(hip, HEADLINE_M, N, (hip.TILE_WIDE, hip.TILE_NARROW))


@pytest.mark.parametrize("M", [1, 17, 31, 32, 33, 95, 1000, 4100])
@pytest.mark.parametrize("N", [384, 1152, 1536])
def test_ws_ragged_rows(hip, M, N):
    """rows that are not a multiple of the 32-row panel, and fewer rows than one panel"""
    _same(hip, M, N, (hip.TILE_WIDE,), seed=M)


@pytest.mark.parametrize("grid_cap,N", [(c, n) for n in (384, 1152, 1536) for c in (3, 4, 7, 64, 255) if c >= n // 384])
def test_ws_grid_caps(hip, grid_cap, N):
    """capped grids: long multi-panel walks, slice counts that do not divide the grid (whole groups only; fewer workgroups than
    slices: test_ws_refusals)"""
    _same(hip, 5000, N, (hip.TILE_WIDE,), grid_cap=grid_cap)


def test_ws_refusals(hip):
    """DCV_ERR_UNSUPPORTED for a forced TILE_WS outside its domain; AUTO_WS keeps the tiled kernels there"""
    lib = hip.load()
    pick = lib.dcv_gemm_nt_pick
    assert pick(HEADLINE_M, 1152, 384, hip.EPI_BIAS_BF16, hip.TILE_WS) == hip.TILE_WS
    assert pick(HEADLINE_M, 1152, 768, hip.EPI_BIAS_BF16, hip.TILE_WS) < 0      # K != 384
    assert pick(HEADLINE_M, 1536, 1152, hip.EPI_PLAIN_BF16, hip.TILE_WS) < 0    # K != 384
    assert pick(HEADLINE_M, 768 + 8, 384, hip.EPI_PLAIN_BF16, hip.TILE_WS) < 0  # N % 384 != 0
    assert pick(HEADLINE_M, 384, 384, hip.EPI_BIAS_RESID_F32, hip.TILE_WS) < 0  # fp32 epilogue
    assert pick(64, 1536, 384, hip.EPI_BIAS_GELU_BF16, hip.TILE_AUTO_WS) == pick(64, 1536, 384, hip.EPI_BIAS_GELU_BF16, hip.TILE_AUTO)
    A, W = _bf(256, 768), _bf(384, 768)
    out = torch.empty(256, 384, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        hip.gemm_nt(A, W, hip.EPI_PLAIN_BF16, out, tile=hip.TILE_WS)
    A, W = _bf(256, 384), _bf(200, 384)
    out = torch.empty(256, 200, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        hip.gemm_nt(A, W, hip.EPI_PLAIN_BF16, out, tile=hip.TILE_WS)
    A, W = _bf(256, 384), _bf(1152, 384)
    out = torch.empty(256, 1152, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        hip.gemm_nt(A, W, hip.EPI_PLAIN_BF16, out, tile=hip.TILE_WS, grid_cap=2)  # 3 slices need 3 workgroups
