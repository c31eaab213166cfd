"""The float64 restatement of gradient-weighted attention relevance (tests/attention_relevance_ref.py) on closed forms and against the explicit
relevance matrix, the fixture's meta and shapes, and the C ABI's two new entries.  No GPU."""
import os
import re

import numpy as np
import torch

from attention_relevance_ref import normalised_patches, relevance, relevance_step_ref, tv
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy(L=5, B=2, H=3, N=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    maps = [torch.softmax(torch.randn(B, H, N, N, generator=g, dtype=torch.float64) * 2, -1) for _ in range(L)]
    grads = [torch.randn(B, H, N, N, generator=g, dtype=torch.float64) for _ in range(L)]
    return maps, grads


def _matrix(maps, grads, start_layer):
    """R = I; R <- R + A^_l R, blocks ascending from start_layer."""
    B, _, N, _ = maps[0].shape
    R = torch.eye(N, dtype=torch.float64).expand(B, N, N).clone()
    for l in range(start_layer, len(maps)):
        R = R + (grads[l] * maps[l]).clamp(min=0).mean(1) @ R
    return R


def test_relevance_is_the_cls_row_of_the_matrix_recursion():
    maps, grads = _toy()
    for s in range(5):
        R = _matrix(maps, grads, s)
        assert torch.allclose(relevance(maps, grads, s), R[:, 0], rtol=1e-13, atol=0)
    assert torch.equal(relevance(maps, grads, -2), relevance(maps, grads, 3))
    # any start vector is that combination of rows; and the order of the blocks matters
    g = torch.Generator().manual_seed(3)
    start = torch.rand(2, 7, generator=g, dtype=torch.float64)
    assert torch.allclose(relevance(maps, grads, 1, start), torch.einsum("bq,bqk->bk", start, _matrix(maps, grads, 1)), rtol=1e-13, atol=0)
    assert (relevance(maps, grads) - relevance(maps[::-1], grads[::-1])).abs().max() > 1e-3
    assert (relevance(maps, grads)[:, 0] >= 1).all() and (relevance(maps, grads) >= 0).all()


def test_closed_forms():
    maps, grads = _toy()
    g = torch.Generator().manual_seed(4)
    start = torch.rand(2, 7, generator=g, dtype=torch.float64)
    # a gradient that is negative everywhere: relu removes every block
    neg = [-gr.abs() - 0.1 for gr in grads]
    assert torch.equal(relevance(maps, neg, 0, start), start)
    e0 = torch.zeros(2, 7, dtype=torch.float64)
    e0[:, 0] = 1
    assert torch.equal(relevance(maps, neg), e0)
    # uniform A = 1 / N and a constant positive gradient g: A^ = (g / N) 1 1^T, so with c = g / N and S_0 = 1 the sum grows by (1 + N c) per
    # block and r = e_0 + c (1 + (1 + N c) + ... + (1 + N c)^(L - 1)) 1 = e_0 + ((1 + g)^L - 1) / N 1
    L, N, gv = 4, 7, 0.3
    U = [torch.full((2, 3, N, N), 1.0 / N, dtype=torch.float64)] * L
    Gc = [torch.full((2, 3, N, N), gv, dtype=torch.float64)] * L
    want = e0 + ((1 + gv) ** L - 1) / N
    assert torch.allclose(relevance(U, Gc), want, rtol=1e-13, atol=0)
    assert tv(normalised_patches(relevance(U, Gc)), torch.full((2, N - 1), 1.0 / (N - 1), dtype=torch.float64)) < 1e-15


def test_step_ref_is_one_block_of_relevance():
    g = torch.Generator().manual_seed(5)
    B, H, N = 2, 3, 9
    q, k, v, dO = (torch.randn(B, H, N, 64, generator=g).to(torch.bfloat16) for _ in range(4))
    w = torch.rand(B, N, generator=g)
    w[:, 4] = 0
    scale = 64 ** -0.5
    P = torch.softmax(q.double() @ k.double().transpose(-1, -2) * scale, -1)
    G = dO.double() @ v.double().transpose(-1, -2)
    out, mag = relevance_step_ref(q, k, v, dO, w, N, scale, magnitude=True)
    assert torch.allclose(out, relevance([P], [G], 0, w), rtol=1e-13, atol=0)
    assert (mag >= out).all() and (out >= w.double()).all()
    # rows at or past nq: their weight never enters, and neither they nor the rows of weight 0 are read
    cut = w.clone()
    cut[:, 5:] = 0
    out5 = relevance_step_ref(q, k, v, dO, w, 5, scale)
    assert torch.allclose(out5 - w.double(), relevance([P], [G], 0, cut) - cut.double(), rtol=1e-12, atol=1e-15)
    poisoned = dO.clone()
    poisoned[:, :, 5:] = float("nan")
    poisoned[:, :, 4] = float("inf")
    assert torch.equal(relevance_step_ref(q, k, v, poisoned, w, 5, scale), out5)
    # nq = 1 with the one-hot start: the CLS row of mean_h relu(G P)
    e0 = torch.zeros(B, N)
    e0[:, 0] = 1
    assert torch.allclose(relevance_step_ref(q, k, v, dO, e0, 1, scale), e0.double() + (G * P).clamp(min=0).mean(1)[:, 0], rtol=1e-13, atol=0)


def test_fixture_meta_and_shapes():
    meta, a = load_golden("attn_relevance")
    assert [c["name"] for c in meta["cases"]] == ["small", "sub", "tiny48", "base"]
    for c in meta["cases"]:
        r = a[f"{c['name']}/relevance"]
        assert r.dtype == np.float32 and r.shape == (2, c["depth"], c["B"], c["N"]) and c["B"] == 2 and c["depth"] == 12
        t = np.array(c["targets"])
        assert t.shape == (2, c["B"]) and (t >= 0).all() and (t < c["num_classes"]).all() and (t[0] != t[1]).all()
        assert np.isfinite(r).all() and (r >= 0).all() and (r[:, :, :, 0] >= 1).all()
        # one block rolled leaves little on the patches, twelve a third and more
        s_all, s_last = r[:, 0, :, 1:].sum(-1), r[:, -1, :, 1:].sum(-1)
        assert (s_all > 0.3).all() and (s_all < 0.5).all() and (s_last > 0).all() and (s_last < 0.05).all()
        # the emulation distance the GPU test is held to three times of, and how far the other target lies
        assert 1e-4 < c["emu_tv"] < 2e-2 and 0 < c["emu_cls_rel"] < 1e-3 and 0 < c["emu_sum_rel"] < 2e-2
        for s in range(c["depth"]):
            other = tv(normalised_patches(torch.from_numpy(r[0, s])), normalised_patches(torch.from_numpy(r[1, s])))
            assert other > 5 * 3 * c["emu_tv"], (c["name"], s, other)


def test_the_new_symbols_are_declared_and_exported():
    from diverse_channel_vit_amd import hip
    hdr = open(os.path.join(ROOT, "include", "dcv.h")).read()
    for name, nargs in (("dcv_attn_relevance_step", 12), ("dcv_attn_relevance_step_ps", 11)):
        assert name in hip.EXPORTS and len(hip._SIGS[name][0]) == nargs
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", hdr)
        assert m and len(m.group(1).split(",")) == nargs
    assert callable(hip.attn_relevance_step)
    assert os.path.exists(os.path.join(ROOT, "diverse_channel_vit_amd", "csrc", "attn_rollout.hip"))  # attn_keysweep_kernel<PS, GRAD = true>
