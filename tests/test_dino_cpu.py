"""DINO self-distillation without a GPU: the C ABI's names, the launch plan of the loss kernels (every column of every row owned once), the
restatement against its own autograd, the exact cases' inputs, the schedule, the head, the centre arithmetic, and forward_views' refusal."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import dino_ref
from conftest import ROOT, load_golden

NAMES = ("dcv_dino_loss_fwd", "dcv_dino_loss_bwd", "dcv_dino_loss_ws_floats", "dcv_dino_loss_plan")
TILE, WAVES, CAP = 1024, 4, 2048  # csrc/dino_loss.hip: DL_TILE, DL_WAVES, DL_GRID_CAP


@pytest.fixture(scope="module")
def hip():
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def test_names_are_exported_and_declared():
    from diverse_channel_vit_amd import hip as h
    header = open(os.path.join(ROOT, "include", "dcv.h")).read()
    assert sorted(n for n in h.EXPORTS if n.startswith("dcv_dino_")) == sorted(NAMES)
    for n in NAMES:
        assert n + "(" in header, f"{n} is not declared in include/dcv.h"


# (V, B, K): the issue's cross, then the plan's seams — one column tile / two (K = 1024 | 1025), a partial last tile (2047, 4099), the grid cap
# (B * col_tiles = 4 * 2048: 8188 below, 8192 at, 8193 and 8197 past it, the last with a partial workgroup), a partial last workgroup below the cap
CROSS = [(V, B, K) for K in (1, 3, 4, 7, 64, 1000, 4099, 65536) for V in (2, 3, 10) for B in (1, 3, 64)]
SEAMS = [(2, 1, 1023), (2, 1, 1024), (2, 1, 1025), (3, 2, 2047), (3, 2, 2048), (3, 2, 2049), (2, 8188, 1), (2, 8192, 1), (2, 8193, 1), (2, 8197, 5),
         (2, 4096, 1025), (2, 4097, 1025), (3, 5, 1), (3, 6, 1030)]


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("V,B,K", CROSS + SEAMS)
def test_plan_owns_every_column_once(hip, V, B, K, aligned):
    p = hip.dino_loss_plan(V, B, K, aligned)
    assert p["tile_cols"] == TILE and p["waves_per_wg"] == WAVES
    assert p["vec"] == (4 if aligned and K % 4 == 0 else 1)
    assert p["col_tiles"] == -(-K // TILE) and p["items"] == B * p["col_tiles"]
    groups = -(-p["items"] // WAVES)
    assert p["grid"] == min(groups, CAP) and p["passes"] == -(-groups // p["grid"])
    assert (p["passes"] == 1) == (groups <= CAP)
    assert hip.dino_loss_ws_floats(V, B, K) == p["items"] * (6 + 4 * V) + 2 * B
    # (workgroup, pass, wave) -> item: every item below `items` exactly once
    wg, ps, w = np.meshgrid(np.arange(p["grid"]), np.arange(p["passes"]), np.arange(WAVES), indexing="ij")
    item = ((wg + ps * p["grid"]) * WAVES + w).ravel()
    item = item[item < p["items"]]
    assert np.array_equal(np.sort(item), np.arange(p["items"]))
    # item -> (batch row, tile): a bijection onto B x col_tiles
    b, tile = item // p["col_tiles"], item % p["col_tiles"]
    assert len(set(zip(b.tolist(), tile.tolist()))) == B * p["col_tiles"] and b.max() == B - 1
    # (lane, slot 4 u + e) -> column of the tile, loaded vec at a time: the columns below K of every tile exactly once
    lane, u, e = np.meshgrid(np.arange(64), np.arange(4), np.arange(4), indexing="ij")
    within = ((64 * u + lane) * 4 + e).ravel()
    assert np.array_equal(np.sort(within), np.arange(TILE))
    if p["vec"] == 4:  # a 16-byte load never straddles K
        assert K % 4 == 0
    for t in {0, p["col_tiles"] - 1}:
        cols = t * TILE + within
        cols = cols[cols < K]
        assert np.array_equal(np.sort(cols), np.arange(t * TILE, min(K, (t + 1) * TILE)))


def test_plan_and_entries_refuse(hip):
    lib = hip.load()
    for V, B, K, word in ((1, 1, 8, "shape"), (2, 0, 8, "shape"), (2, 1, 0, "shape"), (2, 1, -4, "shape"), (2, 1, (1 << 29), "unsupported")):
        with pytest.raises(RuntimeError, match=f"(?i)dcv_dino_loss_plan failed: .*{word}"):
            hip.dino_loss_plan(V, B, K)
        assert lib.dcv_dino_loss_ws_floats(V, B, K) < 0
    # the launchers check before any HIP call: made-up addresses are never read
    a = ctypes.c_void_p(4096)
    fwd = lambda lds, ldt, V=2, B=1, K=8, ts=0.1, tt=0.04, ws=1 << 20: lib.dcv_dino_loss_fwd(a, lds, a, ldt, a, V, B, K, ts, tt, a, None, None, None, a, ws, None)
    bwd = lambda lds, ldt, ldd, V=2: lib.dcv_dino_loss_bwd(a, lds, a, ldt, a, a, a, a, V, 1, 8, 0.1, 0.04, a, ldd, None)
    SHAPE, NULL = -1, -5
    assert fwd(7, 8) == SHAPE and fwd(8, 7) == SHAPE and fwd(8, 8, V=1) == SHAPE and fwd(8, 8, ts=0.0) == SHAPE and fwd(8, 8, ws=3) == SHAPE
    assert bwd(7, 8, 8) == SHAPE and bwd(8, 7, 8) == SHAPE and bwd(8, 8, 7) == SHAPE and bwd(8, 8, 8, V=1) == SHAPE
    assert lib.dcv_dino_loss_fwd(None, 8, a, 8, a, 2, 1, 8, 0.1, 0.04, a, None, None, None, a, 1 << 20, None) == NULL
    assert lib.dcv_dino_loss_bwd(a, 8, a, 8, a, a, a, None, 2, 1, 8, 0.1, 0.04, a, 8, None) == NULL


@pytest.mark.parametrize("V,B,K", [(2, 1, 7), (3, 3, 100), (10, 4, 257)])
def test_closed_form_matches_its_autograd_in_float64(V, B, K):
    g = torch.Generator().manual_seed(V * 100 + K)
    S, T, c = 3 * torch.randn(V, B, K, generator=g), 3 * torch.randn(2, B, K, generator=g), torch.randn(K, generator=g)
    l0, d0 = dino_ref.pairwise(S, T, c, 0.1, 0.04)
    l1, d1 = dino_ref.closed_form(S, T, c, 0.1, 0.04)
    assert abs(l0.item() - l1.item()) <= 1e-12 * max(1.0, abs(l0.item()))
    assert (d0 - d1).abs().max().item() <= 1e-14


@pytest.mark.parametrize("V", [2, 3, 5, 9])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_exact_cases_are_exact_in_the_float32_restatement(V, B):
    ts, tt, K = 0.125, 0.0625, 2048
    scale = (2 * V - 2) * B * ts
    assert math.frexp(scale)[0] == 0.5, "n B ts must be a power of two"
    zero = torch.zeros
    _, d = dino_ref.closed_form(zero(V, B, K), zero(2, B, K), zero(K), ts, tt, torch.float32)
    assert not d.any()
    tp, sp = dino_ref.peaks(V, B, K, [0, K - 1, 1023, 1024, 3, 4, 255, 256])
    _, d = dino_ref.closed_form(dino_ref.one_hot_logits(sp, K), dino_ref.one_hot_logits(tp, K), zero(K), ts, tt, torch.float32)
    want = dino_ref.one_hot_grad(tp, sp, K, ts)
    assert torch.equal(d, want)
    assert set((want * scale).unique().tolist()) <= {0.0, 1.0, -1.0, 2.0}
    if V > 2 and B > 1:
        assert {1.0, -1.0, 2.0} <= set((want * scale).unique().tolist()), "the rule must make some peaks coincide and some not"


def test_teacher_temp_schedule():
    from diverse_channel_vit_amd import teacher_temp_schedule
    s = teacher_temp_schedule(0.04, 0.07, 4, 10)
    assert len(s) == 10 and s[0] == 0.04 and s[3:] == [0.07] * 7
    assert np.allclose(s[:4], np.linspace(0.04, 0.07, 4), rtol=0, atol=1e-15)
    assert teacher_temp_schedule(0.04, 0.07, 0, 3) == [0.07] * 3
    assert teacher_temp_schedule(0.04, 0.07, 1, 3) == [0.04, 0.07, 0.07]
    assert len(teacher_temp_schedule(0.04, 0.07, 30, 10)) == 10


def test_head():
    from diverse_channel_vit_amd import DINOHead, update_teacher_head
    torch.manual_seed(0)
    head = DINOHead(24, out_dim=96, hidden_dim=32, bottleneck_dim=16)
    x = torch.randn(5, 24)
    assert head(x).shape == (5, 96)
    assert torch.allclose(head.bottleneck(x).norm(dim=-1), torch.ones(5), atol=1e-6)
    assert not head.last_layer.weight_g.requires_grad and bool((head.last_layer.weight_g == 1).all())
    assert head.last_layer.bias is None and [type(m).__name__ for m in head.mlp] == ["Linear", "GELU", "Linear", "GELU", "Linear"]
    assert DINOHead(24, 96, 32, 16, norm_last_layer=False).last_layer.weight_g.requires_grad
    w = head.mlp[0].weight
    assert w.abs().max().item() <= 2.0 and 0.017 < w.std().item() < 0.023 and not head.mlp[0].bias.any()  # trunc_normal_(std=0.02), cut at +-2 as DINO's
    assert isinstance(DINOHead(24, 96, 32, 16, nlayers=1).mlp, torch.nn.Linear)
    teacher = DINOHead(24, out_dim=96, hidden_dim=32, bottleneck_dim=16)
    before = [p.detach().clone() for p in teacher.parameters()]
    update_teacher_head(teacher, head, 0.75)
    for b, t, s in zip(before, teacher.parameters(), head.parameters()):
        assert torch.allclose(t, 0.75 * b + 0.25 * s.detach(), rtol=0, atol=1e-7)


def test_centre_arithmetic_on_cpu_tensors():
    from diverse_channel_vit_amd.ssl import DINOLoss, center_update
    c, tsum = torch.tensor([1.0, -2.0, 0.5]), torch.tensor([8.0, 0.0, -4.0])
    assert torch.allclose(center_update(c, tsum, 8, 0.9), 0.9 * c + 0.1 * tsum / 8, rtol=0, atol=1e-7)
    loss = DINOLoss(3, center_momentum=0.5)
    assert loss.center.shape == (3,) and not loss.center.any() and "center" in loss.state_dict()
    with pytest.raises(RuntimeError, match="no forward"):
        loss.update_center()
    loss._tsum, loss._rows = tsum, 8
    loss.update_center()
    assert torch.equal(loss.center, torch.tensor([0.5, 0.0, -0.25]))
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        loss(torch.zeros(4, 3), torch.zeros(4, 3), 0.04, n_views=2)


def test_forward_views_raises_off_the_gpu():
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("tiny_e2e")

    class Cfg(dict):
        __getattr__ = dict.get

    cfg = Cfg(meta["cfg"], in_channel_names=[f"c{i}" for i in range(meta["n_channels"])], img_size=[meta["img"]], num_classes=meta["num_classes"])
    model = dcv.dichavit(cfg, mapper={k: list(v) for k, v in meta["mapper"].items()})
    with pytest.raises(RuntimeError, match="runs only on an MI355X"):
        model.forward_views([torch.zeros(2, 3, 32, 32), torch.zeros(4, 3, 16, 16)], "train")
