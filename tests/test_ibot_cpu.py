"""Masked patch-token distillation without a GPU: the C ABI's names, the launch plan of the patch-loss kernels against a table written out by hand,
the block mask generator's exact counts and its rows / weights, the float64 restatement against finite differences, and the centre arithmetic."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ibot_ref
from conftest import ROOT

NAMES = ("dcv_ibot_loss_fwd", "dcv_ibot_loss_bwd", "dcv_ibot_loss_ws_floats", "dcv_ibot_loss_plan")
MASK_NAMES = ("dcv_mask_tokens_fwd", "dcv_mask_tokens_bwd", "dcv_mask_tokens_bwd_ws_floats")
TILE, CHUNK, WAVES, CAP = 1024, 32, 4, 2048  # csrc/loss_rows.hpp: DL_TILE, DL_WAVES, DL_GRID_CAP; csrc/ibot_loss.hip: IB_CHUNK


@pytest.fixture(scope="module")
def hip():
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def test_names_are_exported_and_declared():
    from diverse_channel_vit_amd import hip as h
    header = open(os.path.join(ROOT, "include", "dcv.h")).read()
    assert sorted(n for n in h.EXPORTS if n.startswith("dcv_ibot_")) == sorted(NAMES)
    assert sorted(n for n in h.EXPORTS if n.startswith("dcv_mask_tokens")) == sorted(MASK_NAMES)
    for n in NAMES + MASK_NAMES:
        assert n + "(" in header, f"{n} is not declared in include/dcv.h"
    for n in ("ibot_loss_plan", "ibot_loss_ws_floats", "ibot_loss_fwd", "ibot_loss_bwd", "mask_tokens_fwd", "mask_tokens_bwd"):
        assert callable(getattr(h, n))


# (R, K, aligned) -> (vec, col_tiles, chunks, items, grid, passes, ws floats), worked out by hand from the plan's rules: col_tiles = ceil(K / 1024),
# chunks = ceil(R / 32), items = chunks * col_tiles, groups = ceil(items / 4), grid = min(groups, 2048), passes = ceil(groups / grid),
# ws = 2 (6 R col_tiles + R + chunks K) floats: everything in it is a double
PLAN = {
    (1, 1, True): (1, 1, 1, 1, 1, 1, 2 * 6 + 2 + 2),                                   # R = 1, K = 1
    (5, 1023, True): (1, 1, 1, 1, 1, 1, 2 * 30 + 10 + 2046),                           # one column tile, K % 4 != 0: 4-byte loads
    (5, 1024, True): (4, 1, 1, 1, 1, 1, 2 * 30 + 10 + 2048),                           # one full tile, 16-byte loads
    (5, 1024, False): (1, 1, 1, 1, 1, 1, 2 * 30 + 10 + 2048),                          # the same, unaligned
    (5, 1025, True): (1, 2, 1, 2, 1, 1, 2 * 60 + 10 + 2050),                           # two tiles, the second of one column
    (5, 1028, True): (4, 2, 1, 2, 1, 1, 2 * 60 + 10 + 2056),
    (32, 2048, True): (4, 2, 1, 2, 1, 1, 2 * 384 + 64 + 4096),                         # one full chunk
    (33, 2048, True): (4, 2, 2, 4, 1, 1, 2 * 396 + 66 + 8192),                         # a second chunk of one row
    (65, 4100, False): (1, 5, 3, 15, 4, 1, 2 * 1950 + 130 + 24600),                    # a partial last workgroup
    (262016, 1, True): (1, 1, 8188, 8188, 2047, 1, 2 * 1572096 + 524032 + 16376),      # one workgroup below the cap
    (262144, 1, True): (1, 1, 8192, 8192, 2048, 1, 2 * 1572864 + 524288 + 16384),      # at the cap
    (262145, 1, True): (1, 1, 8193, 8193, 2048, 2, 2 * 1572870 + 524290 + 16386),      # past it: workgroups walk
    (32736, 8192, True): (4, 8, 1023, 8184, 2046, 1, 2 * 1571328 + 65472 + 16760832),  # the same seam at the issue's K: below,
    (32768, 8192, True): (4, 8, 1024, 8192, 2048, 1, 2 * 1572864 + 65536 + 16777216),  # at,
    (32769, 8192, False): (1, 8, 1025, 8200, 2048, 2, 2 * 1572912 + 65538 + 16793600),  # and past the cap, unaligned
    (60000, 8192, True): (4, 8, 1875, 15000, 2048, 2, 2 * 2880000 + 120000 + 30720000),  # two global crops at bs 64, 30 % masked
}


@pytest.mark.parametrize("key", sorted(PLAN))
def test_plan_against_the_hand_written_table(hip, key):
    R, K, aligned = key
    vec, col_tiles, chunks, items, grid, passes, ws = PLAN[key]
    p = hip.ibot_loss_plan(R, K, aligned)
    assert p == dict(vec=vec, tile_cols=TILE, col_tiles=col_tiles, chunk_rows=CHUNK, chunks=chunks, items=items, waves_per_wg=WAVES, grid=grid,
                     passes=passes)
    assert hip.ibot_loss_ws_floats(R, K) == ws
    assert (passes == 1) == (-(-items // WAVES) <= CAP)
    # (workgroup, pass, wave) -> item: every item below `items` exactly once; item -> (chunk, tile) a bijection; the chunks cover the rows once
    wg, ps, w = np.meshgrid(np.arange(grid), np.arange(passes), np.arange(WAVES), indexing="ij")
    item = ((wg + ps * grid) * WAVES + w).ravel()
    item = item[item < items]
    assert np.array_equal(np.sort(item), np.arange(items))
    ch, tile = item // col_tiles, item % col_tiles
    assert len(set(zip(ch.tolist(), tile.tolist()))) == chunks * col_tiles and ch.max() == chunks - 1
    assert (chunks - 1) * CHUNK < R <= chunks * CHUNK
    if vec == 4:  # a 16-byte load never straddles K
        assert K % 4 == 0 and aligned


def test_plan_and_entries_refuse(hip):
    lib = hip.load()
    for R, K, word in ((0, 8, "shape"), (1, 0, "shape"), (1, -4, "shape"), (1, (1 << 29), "unsupported")):
        with pytest.raises(RuntimeError, match=f"(?i)dcv_ibot_loss_plan failed: .*{word}"):
            hip.ibot_loss_plan(R, K)
        assert lib.dcv_ibot_loss_ws_floats(R, K) < 0
    a = ctypes.c_void_p(4096)  # the launchers check before any HIP call: made-up addresses are never read
    fwd = lambda lds, ldt, R=1, K=8, ts=0.1, tt=0.04, ws=1 << 20: lib.dcv_ibot_loss_fwd(a, lds, a, ldt, a, a, R, K, ts, tt, a, None, None, None, a, ws, None)  # noqa: E731
    bwd = lambda lds, ldt, ldd, R=1: lib.dcv_ibot_loss_bwd(a, lds, a, ldt, a, a, a, a, a, R, 8, 0.1, 0.04, a, ldd, None)  # noqa: E731
    SHAPE, NULL = -1, -5
    assert fwd(7, 8) == SHAPE and fwd(8, 7) == SHAPE and fwd(8, 8, R=0) == SHAPE and fwd(8, 8, tt=0.0) == SHAPE and fwd(8, 8, ws=3) == SHAPE
    assert bwd(7, 8, 8) == SHAPE and bwd(8, 7, 8) == SHAPE and bwd(8, 8, 7) == SHAPE and bwd(8, 8, 8, R=0) == SHAPE
    assert lib.dcv_ibot_loss_fwd(a, 8, a, 8, a, None, 1, 8, 0.1, 0.04, a, None, None, None, a, 1 << 20, None) == NULL
    assert lib.dcv_ibot_loss_bwd(a, 8, a, 8, a, a, a, a, None, 1, 8, 0.1, 0.04, a, 8, None) == NULL
    assert lib.dcv_mask_tokens_fwd(a, a, a, a, None, 1, 1, 1, 8, None) == NULL and lib.dcv_mask_tokens_fwd(a, a, a, a, a, 1, 1, 1, 6, None) == SHAPE
    assert lib.dcv_mask_tokens_bwd(a, a, None, a, a, 1, 1, 1, 8, None, 0, None) == NULL
    assert lib.dcv_mask_tokens_bwd(a, a, None, a, a, 1, 1, 1, 8, a, 3, None) == SHAPE
    # parts of 256 rows, 256 / (D / 4) sub-lanes each, D floats per partial
    assert lib.dcv_mask_tokens_bwd_ws_floats(128, 8, 196, 384) == 784 * 2 * 384 and lib.dcv_mask_tokens_bwd_ws_floats(3, 2, 5, 192) == 1 * 5 * 192


# ------------------------------------------------------------------------------------------------------------------------------------------
GRIDS = [(14, 14), (6, 6), (2, 2)]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("per_channel", [True, False])
def test_mask_generator_counts_rows_and_weights(grid, per_channel):
    from diverse_channel_vit_amd import BlockMaskGenerator
    gh, gw = grid
    C, B = 3, 40
    gen = BlockMaskGenerator(grid, channels=C, mask_ratio=(0.1, 0.5), mask_prob=0.5, per_channel=per_channel, seed=11, device=None)
    m = gen(B)
    assert m.mask.shape == (B, C, gh, gw) and m.mask.dtype == torch.bool and m.mask_dev.shape == (B, C * gh * gw) and m.mask_dev.dtype == torch.uint8
    counts = m.mask.flatten(2).sum(-1)  # [B, C]
    lo, hi = round(0.1 * gh * gw), round(0.5 * gh * gw)
    for b in range(B):
        assert len(set(counts[b].tolist())) == 1, "every plane of an image holds the image's target count"
        assert counts[b, 0] == 0 or lo <= counts[b, 0] <= hi
        if not per_channel:
            assert all(torch.equal(m.mask[b, 0], m.mask[b, c]) for c in range(C))
    masked = counts[:, 0] > 0
    assert 0 < int(masked.sum()) < B  # mask_prob 0.5 over 40 images
    if per_channel and gh * gw >= 36:
        assert any(not torch.equal(m.mask[b, 0], m.mask[b, 1]) for b in range(B) if masked[b]), "the channel planes are drawn independently"
    assert torch.equal(m.mask_dev.bool(), m.mask.flatten(1))
    assert m.rows.dtype == torch.int64 and torch.equal(m.rows, m.mask.flatten().nonzero().flatten())
    assert bool((m.rows[1:] > m.rows[:-1]).all())
    per_image = counts.sum(1)
    want = 1.0 / (per_image.clamp(min=1).float() * B)
    assert m.weights.dtype == torch.float32 and torch.equal(m.weights, want[m.rows // (C * gh * gw)])
    assert abs(m.weights.double().sum().item() - int(masked.sum()) / B) <= 1e-6
    again = BlockMaskGenerator(grid, channels=C, mask_ratio=(0.1, 0.5), mask_prob=0.5, per_channel=per_channel, seed=11, device=None)(B)
    assert torch.equal(again.mask, m.mask) and torch.equal(again.rows, m.rows) and torch.equal(again.weights, m.weights)
    other = BlockMaskGenerator(grid, channels=C, mask_ratio=(0.1, 0.5), mask_prob=0.5, per_channel=per_channel, seed=12, device=None)(B)
    assert not torch.equal(other.mask, m.mask)


@pytest.mark.parametrize("ratio", [(0.1, 0.1), (0.3, 0.3), (0.5, 0.5), (1.0, 1.0)])
@pytest.mark.parametrize("grid", GRIDS)
def test_mask_generator_hits_the_exact_target(grid, ratio):
    from diverse_channel_vit_amd import BlockMaskGenerator
    gh, gw = grid
    m = BlockMaskGenerator(grid, channels=2, mask_ratio=ratio, mask_prob=1.0, seed=3, device=None)(6)
    assert bool((m.mask.flatten(2).sum(-1) == round(ratio[0] * gh * gw)).all())


def test_mask_generator_edges():
    from diverse_channel_vit_amd import BlockMaskGenerator
    m = BlockMaskGenerator((1, 1), channels=4, mask_ratio=(0.5, 1.0), mask_prob=1.0, seed=0, device=None)(16)  # round(u) is 0 or 1
    assert m.mask.shape == (16, 4, 1, 1) and set(m.mask.flatten(1).sum(1).tolist()) <= {0, 4}
    none = BlockMaskGenerator((6, 6), channels=2, mask_prob=0.0, seed=0, device=None)(5)
    assert not none.mask.any() and none.rows.numel() == 0 and none.weights.numel() == 0
    every = BlockMaskGenerator((6, 6), channels=2, mask_prob=1.0, seed=0, device=None)(5)
    assert bool((every.mask.flatten(1).sum(1) > 0).all()) and abs(every.weights.sum().item() - 1.0) <= 1e-6
    with pytest.raises(ValueError):
        BlockMaskGenerator((6, 6), channels=2, mask_ratio=(0.5, 0.1))
    with pytest.raises(ValueError):
        BlockMaskGenerator((0, 6), channels=2)


# ------------------------------------------------------------------------------------------------------------------------------------------
def test_restatement_gradient_matches_finite_differences():
    R, K, ts, tt = 3, 7, 0.1, 0.04
    g = torch.Generator().manual_seed(5)
    S, T, c = torch.randn(R, K, generator=g, dtype=torch.float64), torch.randn(R, K, generator=g, dtype=torch.float64), torch.randn(K, generator=g, dtype=torch.float64)
    w = torch.tensor([0.5, 0.0, 0.25], dtype=torch.float64)
    loss, dS = ibot_ref.paired(S, T, c, w, ts, tt)
    l2, d2 = ibot_ref.closed_form(S, T, c, w, ts, tt)
    assert abs(loss.item() - l2.item()) <= 1e-12 * max(1.0, abs(loss.item())) and (dS - d2).abs().max().item() <= 1e-13
    h = 1e-6
    fd = torch.zeros_like(S)
    for r in range(R):
        for k in range(K):
            up, dn = S.clone(), S.clone()
            up[r, k] += h
            dn[r, k] -= h
            fd[r, k] = (ibot_ref.closed_form(up, T, c, w, ts, tt)[0] - ibot_ref.closed_form(dn, T, c, w, ts, tt)[0]) / (2 * h)
    assert (fd - dS).abs().max().item() <= 1e-7  # central differences: h^2 f''' / 6 ~ 1e-12 * 1e3, rounding 1e-16 / 1e-6
    assert not dS[1].any(), "a row of weight 0 has no gradient"
    _, dg = ibot_ref.paired(S, T, c, w, ts, tt, g=0.5)
    assert torch.allclose(dg, 0.5 * dS, rtol=0, atol=1e-15)


def test_exact_cases_are_exact_in_the_float32_restatement():
    ts, tt, K = 0.125, 0.0625, 2048
    cols = [0, 3, 4, 255, 256, 1023, 1024, K - 1]
    R = 12
    w = torch.tensor([2.0 ** -(r % 5) for r in range(R)])
    _, d = ibot_ref.closed_form(torch.zeros(R, K), torch.zeros(R, K), torch.zeros(K), w, ts, tt, torch.float32)
    assert not d.any()
    tp, sp = ibot_ref.peaks(R, K, cols)
    assert bool((tp == sp).any()) and bool((tp != sp).any()), "the rule must make some peaks coincide and some not"
    _, d = ibot_ref.closed_form(ibot_ref.one_hot_logits(sp, K), ibot_ref.one_hot_logits(tp, K), torch.zeros(K), w, ts, tt, torch.float32)
    assert torch.equal(d, ibot_ref.one_hot_grad(tp, sp, w, K, ts))


def test_centre_arithmetic_on_cpu_tensors():
    from diverse_channel_vit_amd.ssl import IBOTPatchLoss, center_update
    c, tsum = torch.tensor([1.0, -2.0, 0.5]), torch.tensor([8.0, 0.0, -4.0])
    assert torch.allclose(center_update(c, tsum, 8, 0.9), 0.9 * c + 0.1 * tsum / 8, rtol=0, atol=1e-7)
    loss = IBOTPatchLoss(3, center_momentum=0.5)
    assert loss.center.shape == (3,) and not loss.center.any() and "center" in loss.state_dict()
    with pytest.raises(RuntimeError, match="no forward"):
        loss.update_center()
    loss._tsum, loss._rows = tsum, 8
    loss.update_center()
    assert torch.equal(loss.center, torch.tensor([0.5, 0.0, -0.25]))
    with pytest.raises(RuntimeError, match="no forward"):
        loss.update_center()
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        loss(torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4), 0.04)
