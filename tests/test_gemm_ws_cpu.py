"""dcv_gemm_nt_pick for the weight-stationary NT GEMM (DCV_TILE_WS / DCV_TILE_AUTO_WS) is host logic (no GPU call)."""


def test_ws_tile_choice():
    from diverse_channel_vit_amd import hip
    lib = hip.load()
    M = 64 * 1569
    nt = lambda m, n, k, epi, t: lib.dcv_gemm_nt_pick(m, n, k, epi, t)
    AW, WS = hip.TILE_AUTO_WS, hip.TILE_WS
    # the four K = 384 products of the headline step go to the weight-stationary kernel
    assert nt(M, 1152, 384, hip.EPI_BIAS_BF16, AW) == WS          # qkv
    assert nt(M, 1536, 384, hip.EPI_BIAS_GELU_BF16, AW) == WS     # fc1 + GELU
    assert nt(M, 1536, 384, hip.EPI_GELU_BWD_BF16, AW) == WS      # x GELU'
    assert nt(M, 384, 384, hip.EPI_PLAIN_BF16, AW) == WS          # proj input gradient
    # everything else keeps AUTO's choice: fp32 epilogues, K != 384, the tokeniser, the 64-row CLS tail
    for args in ((M, 384, 384, hip.EPI_BIAS_RESID_F32), (M, 384, 1536, hip.EPI_PLAIN_BF16), (M, 384, 1152, hip.EPI_PLAIN_BF16),
                 (M, 384, 256, hip.EPI_PATCH), (64, 1536, 384, hip.EPI_BIAS_GELU_BF16), (64, 1152, 384, hip.EPI_BIAS_BF16)):
        assert nt(*args, AW) == nt(*args, hip.TILE_AUTO)
    # AUTO itself never returns the weight-stationary kernel
    assert nt(M, 1152, 384, hip.EPI_BIAS_BF16, hip.TILE_AUTO) != WS
    # forced: legal only for K == 384, N % 384 == 0 and the four bf16-output epilogues
    assert nt(100, 384, 384, hip.EPI_PLAIN_BF16, WS) == WS
    assert nt(M, 1152, 768, hip.EPI_BIAS_BF16, WS) < 0
    assert nt(M, 776, 384, hip.EPI_PLAIN_BF16, WS) < 0
    assert nt(M, 384, 384, hip.EPI_BIAS_RESID_F32, WS) < 0
    assert nt(M, 384, 256, hip.EPI_PATCH, WS) < 0
    assert nt(M, 384, 384, hip.EPI_PLAIN_BF16, 7) < 0
