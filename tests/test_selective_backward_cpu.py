"""The selective backward without a GPU: dcv_bias_grad's exports, error codes and launch plan (host logic of csrc/bias_grad.hip, held against
its restatement and the case table of tests/test_selective_backward_gpu.py), a numpy emulation of that plan on exact operands, the gradient
plan function on flag vectors, and set_trainable() on a CPU-constructed model.  No kernel is launched: every refused call returns before
its first HIP call, and the plan and workspace queries are pure functions."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import diverse_channel_vit_amd as dcv
from diverse_channel_vit_amd import hip
from test_selective_backward_gpu import BG_GRID_CAP, BIAS_CASES, WIDTHS, bias_plan, visited_rows

dichavit = importlib.import_module("diverse_channel_vit_amd.dichavit")  # the package attribute of that name is the factory function
OK, SHAPE, ALIGN, UNSUPPORTED, NULL = 0, -1, -2, -3, -5


def _lib_plan(lib, M, P):
    got = [C.c_int() for _ in range(5)]
    rc = lib.dcv_bias_grad_plan(M, P, *[C.byref(g) for g in got])
    return rc, tuple(g.value for g in got)


def test_exports_signatures_and_error_codes():
    lib = hip.load()
    assert {"dcv_bias_grad", "dcv_bias_grad_ws_floats", "dcv_bias_grad_plan"} <= set(hip.EXPORTS)
    assert len(hip._SIGS["dcv_bias_grad"][0]) == 8 and len(hip._SIGS["dcv_bias_grad_plan"][0]) == 7 and callable(hip.bias_grad)
    Y, db, ws = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)  # aligned addresses nobody dereferences: every call below is refused
    M, P = 100, 384
    for bad in ((None, db, ws), (Y, None, ws), (Y, db, None)):
        assert lib.dcv_bias_grad(bad[0], P, M, P, bad[1], bad[2], 1 << 30, None) == NULL
    assert lib.dcv_bias_grad(Y, P, 0, P, db, ws, 1 << 30, None) == SHAPE
    assert lib.dcv_bias_grad(Y, P, M, 0, db, ws, 1 << 30, None) == SHAPE
    assert lib.dcv_bias_grad(Y, P - 8, M, P, db, ws, 1 << 30, None) == SHAPE   # rows would overlap
    for k in range(3):
        ptrs = [Y, db, ws]
        ptrs[k] = C.c_void_p(ptrs[k].value + 4)
        assert lib.dcv_bias_grad(ptrs[0], P, M, P, ptrs[1], ptrs[2], 1 << 30, None) == ALIGN, k
    assert lib.dcv_bias_grad(Y, P + 4, M, P, db, ws, 1 << 30, None) == ALIGN      # a row stride off the 16-byte multiple
    assert lib.dcv_bias_grad(Y, 16, M, 12, db, ws, 1 << 30, None) == UNSUPPORTED  # P % 8 != 0
    need = lib.dcv_bias_grad_ws_floats(M, P)
    assert need == bias_plan(M, P).row_wgs * P
    assert lib.dcv_bias_grad(Y, P, M, P, db, ws, need - 1, None) == SHAPE         # a workspace one float short
    assert lib.dcv_bias_grad_ws_floats(0, P) == SHAPE and lib.dcv_bias_grad_ws_floats(M, 12) == UNSUPPORTED
    a = C.c_int()
    assert lib.dcv_bias_grad_plan(M, P, None, C.byref(a), C.byref(a), C.byref(a), C.byref(a)) == NULL
    assert _lib_plan(lib, 0, P)[0] == SHAPE and _lib_plan(lib, M, 0)[0] == SHAPE and _lib_plan(lib, M, 20)[0] == UNSUPPORTED


def test_plan_against_the_case_table():
    """The library's plan equals the restatement at every case, and the table sits on the seams it claims: spelled-out values at the widths
    the model uses, one pass up to the rows a grid pass covers and two right above."""
    lib = hip.load()
    assert {c.P for c in BIAS_CASES} == set(WIDTHS) and any(c.M == 1 for c in BIAS_CASES)
    for c in BIAS_CASES:
        rc, got = _lib_plan(lib, c.M, c.P)
        p = bias_plan(c.M, c.P)
        assert rc == OK and got == (p.col_chunks, p.rows_per_wave, p.rows_per_wg, p.row_wgs, p.passes), c.name
        assert lib.dcv_bias_grad_ws_floats(c.M, c.P) == p.row_wgs * c.P
        assert p.row_wgs * p.col_chunks <= BG_GRID_CAP and p.lpc * p.s <= 64 and p.lpc * p.col_chunks * 8 >= c.P
    # (col_chunks, rows_per_wave, rows_per_wg) per width
    assert {P: bias_plan(1, P)[:1] + bias_plan(1, P)[3:5] for P in WIDTHS} == {8: (1, 512, 2048), 192: (1, 16, 64), 384: (1, 8, 32), 1152: (3, 8, 32),
                                                                             1536: (3, 8, 32)}
    for P in WIDTHS:
        p1 = bias_plan(1, P)
        cap = BG_GRID_CAP // p1.col_chunks
        at = {c.name.split(" ", 1)[1]: bias_plan(c.M, c.P) for c in BIAS_CASES if c.P == P}
        assert (at["wave -1"].row_chunks, at["wave +0"].row_chunks, at["wave +1"].row_chunks) == (1, 1, 1)
        assert (at["workgroup -1"].row_wgs, at["workgroup +0"].row_wgs, at["workgroup +1"].row_wgs) == (1, 1, 2)
        assert (at["grid pass -1"].row_wgs, at["grid pass +0"].row_wgs, at["grid pass +1"].row_wgs) == (cap, cap, cap)
        assert (at["grid pass -1"].passes, at["grid pass +0"].passes, at["grid pass +1"].passes) == (1, 1, 2)
        assert at["grid pass +1"].row_chunks == cap + 1  # workgroup 0 walks two chunks, every other workgroup one
    # the headline shapes: 100 416 token rows
    assert bias_plan(100416, 384)[5:] == (3138, 512, 7) and bias_plan(100416, 1536)[5:] == (3138, 170, 19)


@pytest.mark.parametrize("P", [192, 384, 1152])  # two rows per wave load; one column chunk; three
def test_emulated_plan_sees_a_dropped_or_repeated_row(P):
    """The plan emulated in numpy on operands from {1, 2, 3}: every row is added exactly once, the per-workgroup partials add up to the exact
    column sums — and a walk that drops or repeats any single row at a seam (the first and last row of a wave step, of a workgroup's chunk
    and of a grid pass) gives another integer in every column, so the exact comparison of the GPU test cannot miss such a defect."""
    p1 = bias_plan(1, P)
    cap = BG_GRID_CAP // p1.col_chunks
    M = (cap + 2) * p1.rows_per_wg + p1.rows_per_wave + 1  # past the cap: workgroups 0 .. 2 walk two chunks, the last one ragged
    rs = np.random.RandomState(P)
    ncol = 8  # the rows a column sees do not depend on the column: eight columns stand for all
    Y = rs.randint(1, 4, size=(M, ncol)).astype(np.int64)
    walk = visited_rows(M, P)
    p = bias_plan(M, P)
    assert len(walk) == p.row_wgs == cap and p.passes == 2 and len(walk[0]) == 2 * p.rows_per_wg and len(walk[3]) == p.rows_per_wg
    count = np.zeros(M, dtype=np.int64)
    for rows in walk:
        np.add.at(count, rows, 1)
    assert (count == 1).all()
    parts = np.stack([Y[rows].sum(0) for rows in walk])
    exact = Y.sum(0)
    assert (parts.sum(0) == exact).all()
    seams = sorted({0, M - 1} | {r for at in (p.rows_per_wave, p.rows_per_wg, cap * p.rows_per_wg) for r in (at - 1, at)})
    owner = {r: b for b, rows in enumerate(walk) for r in rows}
    for r in seams:
        b = owner[r]
        for defect in ([q for q in walk[b] if q != r], walk[b] + [r]):  # the row dropped, the row added twice
            total = parts.sum(0) - parts[b] + Y[defect].sum(0)
            assert (total != exact).all(), r


def _need(depth, x=False, E=False, pos=False, params=()):
    """needs_input_grad of _EncoderFn.forward: six non-tensor arguments, x, E, the positional table, then 3 + 12 depth + 2 parameters."""
    flags = [False] * (3 + 12 * depth + 2)
    for i in params:
        flags[i] = True
    return [False] * 6 + [x, E, pos] + flags


def test_gradient_plan_on_flag_vectors():
    depth = 12
    n = 3 + 12 * depth + 2
    plan = dichavit._grad_plan(_need(depth, E=True, pos=True, params=range(n)), depth, None)
    assert plan.frozen_k is None and not plan.data_only and all(plan.asked) and plan.patch == (True, True)
    assert all(b == {"qkv": (True, True), "proj": (True, True), "fc1": (True, True), "fc2": (True, True)} for b in plan.blocks)  # today's plan
    plan = dichavit._grad_plan(_need(depth, x=True), depth, None)
    assert plan.data_only and plan.frozen_k is None and not any(plan.params) and plan.patch == (False, False)
    assert all(v == (False, False) for b in plan.blocks for v in b.values())
    assert not dichavit._grad_plan(_need(depth, x=True), depth, object()).data_only  # with a reducer the full backward runs
    # the prefix cases: the same k as _frozen_prefix
    for k in (0, 1, 6, 11, 12):
        params = list(range(3 + 12 * k, n))
        plan = dichavit._grad_plan(_need(depth, params=params), depth, None)
        assert plan.frozen_k == k == dichavit._frozen_prefix(False, [bi >= k for bi in range(depth)], True, None)
        assert [all(v == (True, True) for v in b.values()) for b in plan.blocks] == [bi >= k for bi in range(depth)]
        assert dichavit._grad_plan(_need(depth, x=True, params=params), depth, None).frozen_k is None
    # channel embedding only: E asks, no parameter of the node does — no product anywhere and no prefix
    plan = dichavit._grad_plan(_need(depth, E=True), depth, None)
    assert plan.frozen_k is None and not plan.data_only and not any(plan.params) and plan.patch == (False, False)
    assert all(v == (False, False) for b in plan.blocks for v in b.values())
    # a bias alone, a weight alone: fc1 of block 7 is parameters 8 and 9 of that block's twelve
    plan = dichavit._grad_plan(_need(depth, E=True, params=[3 + 12 * 7 + 9, 3 + 12 * 2 + 2, 2]), depth, None)
    assert plan.blocks[7]["fc1"] == (False, True) and plan.blocks[2]["qkv"] == (True, False) and plan.patch == (False, True)
    assert sum(v != (False, False) for b in plan.blocks for v in b.values()) == 2
    # under a DataParallel reducer everything is computed, and the node still returns gradients only to those who asked
    plan = dichavit._grad_plan(_need(depth, E=True, params=[5]), depth, object())
    assert all(plan.params) and sum(plan.asked) == 1 and plan.asked[5] and plan.patch == (True, True)


class Cfg(dict):
    __getattr__ = dict.get


def _model(**over):
    cfg = Cfg(dict(name="dichavit", pretrained_model_name="tiny", patch_size=8, temperature=0.07, learnable_temp=False, enable_sample=False,
                   use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False,
                   block_type="block", hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.1, ortho_loss_v1_lambda=0.0,
                   drop_path_rate=0.0, gamma_s=1.0, gamma_d=4.0, reverse_pos_pairs=True, use_square=False, in_channel_names=["a", "b", "c"],
                   img_size=[32], num_classes=5), **over)
    torch.manual_seed(0)
    return dcv.dichavit(cfg, mapper={"train": [0, 1, 2]})


def _flags(model):
    return {n for n, p in model.named_parameters() if p.requires_grad}


def test_set_trainable_presets_union_and_errors():
    model = _model()
    names = [n for n, _ in model.named_parameters()]
    depth = 12
    assert model.set_trainable("all") == sorted(names) and _flags(model) == set(names)
    bias = model.set_trainable("bias")
    assert set(bias) == {n for n in names if n.endswith(".bias")} == _flags(model) and len(bias) == 6 * depth + 3
    norm = model.set_trainable("norm")
    assert set(norm) == _flags(model) and len(norm) == 4 * depth + 2 and all(".norm" in n for n in norm)
    ce = {"feature_extractor.patch_embed.channel_embed.weight", "feature_extractor.patch_embed.channel_emb_proxies"}
    assert set(model.set_trainable("channel_embed")) == ce == _flags(model)
    tok = set(model.set_trainable("tokeniser"))
    assert tok == ce | {"feature_extractor.cls_token", "feature_extractor.pos_embed", "feature_extractor.patch_embed.proj.weight",
                        "feature_extractor.patch_embed.proj.bias"} == _flags(model)
    head = set(model.set_trainable("head"))
    assert head == {"proxies", "classifer_head.weight", "classifer_head.bias", "feature_extractor.norm.weight", "feature_extractor.norm.bias"} == _flags(model)
    both = model.set_trainable("head", "norm", "feature_extractor.blocks.7.mlp.fc1.*")
    assert set(both) == head | set(norm) | {"feature_extractor.blocks.7.mlp.fc1.weight", "feature_extractor.blocks.7.mlp.fc1.bias"} == _flags(model)
    assert both == sorted(both)
    assert len(model.set_trainable("feature_extractor.blocks.*.attn.qkv.weight")) == depth
    # the host-side twin of the gradient plan reads these flags
    plan = model._host_grad_plan(torch.zeros(1))
    assert all(b["qkv"] == (True, False) and b["fc2"] == (False, False) for b in plan.blocks) and plan.frozen_k == 0
    before = _flags(model)
    for bad in (("no.such.parameter",), ("bias", "blocks.99.*"), ()):
        with pytest.raises(ValueError):
            model.set_trainable(*bad)
        assert _flags(model) == before
    with pytest.raises(ValueError):
        model.set_trainable(7)
    assert _flags(model) == before
    model.set_trainable("channel_embed")
    plan = model._host_grad_plan(torch.zeros(1))
    assert plan.frozen_k is None and not any(plan.params) and model._host_frozen_prefix(torch.zeros(1)) is None


def test_set_trainable_respects_freeze_channel_emb():
    model = _model(freeze_channel_emb=True)
    ce = "feature_extractor.patch_embed.channel_embed.weight"
    assert ce not in model.set_trainable("all") and ce not in _flags(model)
    assert model.set_trainable("channel_embed") == ["feature_extractor.patch_embed.channel_emb_proxies"]
    assert model.set_trainable(ce) == [] and not _flags(model)  # the spec matched, and the configuration keeps its only match frozen
    model.freeze_prefix(0, tokeniser=False)
    assert ce not in _flags(model)
