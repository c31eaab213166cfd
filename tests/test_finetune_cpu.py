"""Host side of fine-tuning (no GPU): HipAdamW takes parameter groups, param_groups() / freeze_prefix() on the tiny model, the run table
of dcv_adamw_groups (optim.build_segments) against a brute-force per-float4 map, the kernel's index mapping restated
(tests/test_finetune_gpu.py: groups_plan / groups_visits) over the case table of the GPU kernel test, and the state_dict layout of a
multi-group HipAdamW against torch.optim.AdamW."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_finetune_gpu as T  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.get


def tiny():
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("tiny_e2e")
    cfg = Cfg(meta["cfg"], in_channel_names=[f"c{i}" for i in range(meta["n_channels"])], img_size=[meta["img"]], num_classes=meta["num_classes"])
    model = dcv.dichavit(cfg, mapper={k: list(v) for k, v in meta["mapper"].items()})
    assert len(model.feature_extractor.blocks) == 12
    return model


TOKENISER = ["feature_extractor.cls_token", "feature_extractor.pos_embed", "feature_extractor.patch_embed.channel_emb_proxies",
             "feature_extractor.patch_embed.proj.weight", "feature_extractor.patch_embed.proj.bias",
             "feature_extractor.patch_embed.channel_embed.weight"]
HEAD = ["feature_extractor.norm.weight", "feature_extractor.norm.bias", "classifer_head.weight", "classifer_head.bias", "proxies"]
BLOCK = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias",
         "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"]


def test_hipadamw_takes_parameter_groups():
    """2 and 28 groups construct, 33 are refused (the parent refused 2)."""
    import diverse_channel_vit_amd as dcv
    ps = [torch.nn.Parameter(torch.zeros(4)) for _ in range(33)]
    two = dcv.HipAdamW([dict(params=ps[:1], weight_decay=0.04), dict(params=ps[1:2], weight_decay=0.0)], lr=1e-3)
    assert [g["weight_decay"] for g in two.param_groups] == [0.04, 0.0] and two._gsteps == [0, 0]
    many = dcv.HipAdamW([dict(params=[p], lr=1e-3 * 0.9 ** i) for i, p in enumerate(ps[:28])])
    assert len(many.param_groups) == 28
    assert len(dcv.HipAdamW([dict(params=[p]) for p in ps[:32]]).param_groups) == 32
    with pytest.raises(ValueError, match="at most 32"):
        dcv.HipAdamW([dict(params=[p]) for p in ps])


def test_param_groups_on_the_tiny_model():
    import diverse_channel_vit_amd as dcv
    model = tiny()
    names = {id(p): n for n, p in model.named_parameters()}
    assert sorted(names.values()) == sorted(TOKENISER + HEAD + [f"feature_extractor.blocks.{i}.{b}" for i in range(12) for b in BLOCK])
    groups = dcv.param_groups(model, lr=1e-3, weight_decay=0.05, layer_decay=0.75)
    listed = [id(p) for g in groups for p in g["params"]]
    assert len(listed) == len(set(listed)) and set(listed) == {id(p) for p in model.parameters()}  # every parameter exactly once
    assert len(groups) == 28  # 14 layer ids x (decay, no decay)
    decay, plain = groups[:14], groups[14:]
    assert all(g["weight_decay"] == 0.05 for g in decay) and all(g["weight_decay"] == 0.0 for g in plain)  # regularised groups first
    for half in (decay, plain):
        assert [g["layer_id"] for g in half] == list(range(14))
        for g in half:
            assert g["lr_scale"] == 0.75 ** (13 - g["layer_id"]) and g["lr"] == 1e-3 * g["lr_scale"]
    got = lambda g: sorted(names[id(p)] for p in g["params"])  # noqa: E731
    assert got(decay[0]) == ["feature_extractor.patch_embed.channel_emb_proxies", "feature_extractor.patch_embed.proj.weight"]
    assert got(plain[0]) == sorted(["feature_extractor.cls_token", "feature_extractor.pos_embed", "feature_extractor.patch_embed.proj.bias",
                                    "feature_extractor.patch_embed.channel_embed.weight"])
    for i in range(12):
        pre = f"feature_extractor.blocks.{i}."
        assert got(decay[i + 1]) == sorted(pre + b for b in BLOCK if b.endswith("weight") and "norm" not in b)
        assert got(plain[i + 1]) == sorted(pre + b for b in BLOCK if b.endswith("bias") or "norm" in b)
    assert got(decay[13]) == ["classifer_head.weight", "proxies"]
    assert got(plain[13]) == ["classifer_head.bias", "feature_extractor.norm.bias", "feature_extractor.norm.weight"]
    # layer_decay = 1: exactly the two-group split, group 0 the regularised one
    two = dcv.param_groups(model, lr=1e-3, weight_decay=0.05)
    assert len(two) == 2 and two[0]["weight_decay"] == 0.05 and two[1]["weight_decay"] == 0.0
    assert all(g["lr"] == 1e-3 and g["lr_scale"] == 1.0 for g in two)
    assert all(p.ndim >= 2 for p in two[0]["params"]) and len(two[0]["params"]) == 2 + 4 * 12 + 2
    assert len(dcv.param_groups(model, 1e-3, 0.05, no_decay_1d=False)) == 1
    # frozen parameters are absent, empty groups dropped
    model.freeze_prefix(8)
    fr = dcv.param_groups(model, lr=1e-3, weight_decay=0.05, layer_decay=0.75)
    assert [g["layer_id"] for g in fr] == [9, 10, 11, 12, 13] * 2
    assert all(p.requires_grad for g in fr for p in g["params"]) and sum(len(g["params"]) for g in fr) == 4 * 12 + 5


def test_freeze_prefix_sets_the_documented_flags():
    model = tiny()
    assert model.freeze_prefix(5) is model
    flags = {n: p.requires_grad for n, p in model.named_parameters()}
    for n in TOKENISER:
        assert flags[n] is False, n
    for n in HEAD:
        assert flags[n] is True, n
    for i in range(12):
        for b in BLOCK:
            assert flags[f"feature_extractor.blocks.{i}.{b}"] is (i >= 5)
    model.freeze_prefix(3, tokeniser=False)
    flags = {n: p.requires_grad for n, p in model.named_parameters()}
    assert all(flags[n] for n in TOKENISER) and not flags["feature_extractor.blocks.2.mlp.fc2.bias"] and flags["feature_extractor.blocks.3.norm1.weight"]
    model.freeze_prefix(0, tokeniser=False)
    assert all(p.requires_grad for p in model.parameters())
    model.freeze_prefix(12)
    assert [n for n, p in model.named_parameters() if p.requires_grad] == [n for n, _ in model.named_parameters() if n in HEAD]
    with pytest.raises(ValueError):
        model.freeze_prefix(13)


def _brute(offsets, numels, total, rows):
    """Row of every float4 of [0, total / 4): a tensor's floats, and the padding behind them, take the tensor's row."""
    m = np.full(total // 4, -7, dtype=np.int64)
    for i, (o, n) in enumerate(zip(offsets, numels)):
        end = offsets[i + 1] if i + 1 < len(offsets) else total
        assert o % 4 == 0 and o + n <= end and end - (o + n) < 4
        m[o // 4:end // 4] = rows[i]
    assert (m != -7).all()
    return m


def _expand(ends4, groups, total):
    assert ends4 == sorted(set(ends4)) and ends4[0] > 0 and ends4[-1] == total // 4 and len(ends4) == len(groups)  # sorted, covering
    assert all(a != b for a, b in zip(groups, groups[1:]))  # adjacent runs of one row were merged
    m = np.empty(total // 4, dtype=np.int64)
    lo = 0
    for e, g in zip(ends4, groups):
        m[lo:e] = g
        lo = e
    return m


def test_segment_table_against_a_brute_force_map():
    import diverse_channel_vit_amd as dcv
    from diverse_channel_vit_amd.optim import build_segments
    model = tiny()
    model._ensure_arena(torch.device("cpu"))
    enc, offs, total = model._enc_params, model._enc_off, model._enc_size
    numels = [p.numel() for p in enc]
    assert len(enc) == 3 + 12 * 12 + 2 and total % 4 == 0
    names = {id(p): n for n, p in model.named_parameters()}

    def rows_of(groups):
        gid = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
        return [gid.get(id(p), -1) for p in enc]

    def check(rows):
        ends4, grps = build_segments(offs, total, rows)
        assert (_expand(ends4, grps, total) == _brute(offs, numels, total, rows)).all()
        return ends4, grps

    # all parameters in one group: one run
    assert check([0] * len(enc)) == ([total // 4], [0])
    # decay / no-decay split: the runs alternate.  cls_token (plain) | proj.weight (decay) | proj.bias + norm1 (plain) | qkv.weight | qkv.bias |
    # proj.weight | proj.bias + norm2 | fc1.weight | fc1.bias | fc2.weight | fc2.bias + next norm1 ... : 3 + 8 per block + 1
    two = dcv.param_groups(model, 1e-3, 0.05)
    ends4, grps = check(rows_of(two))
    assert len(grps) == 2 + 8 * 12 + 1 and grps[:4] == [1, 0, 1, 0] and set(grps) == {0, 1}
    # LLRD: 28 groups, no merge across a block's seam
    llrd = dcv.param_groups(model, 1e-3, 0.05, layer_decay=0.75)
    ends4, grps = check(rows_of(llrd))
    assert len(grps) == 3 + 9 * 12 + 1 and len(set(grps)) == 28 - 1  # `proxies`' group mate classifer_head.weight sits outside the range: 27 rows inside
    # a frozen prefix: ONE leading -1 run up to block 8's first float4
    model.freeze_prefix(8)
    ends4, grps = check(rows_of(dcv.param_groups(model, 1e-3, 0.05)))
    b8 = offs[[names[id(p)] for p in enc].index("feature_extractor.blocks.8.norm1.weight")]
    assert grps[0] == -1 and ends4[0] == b8 // 4 and -1 not in grps[1:]
    model.freeze_prefix(0, tokeniser=False)
    # a lone frozen tensor in the middle
    lone = model.feature_extractor.blocks[5].attn.proj.weight
    lone.requires_grad_(False)
    rows = rows_of([dict(params=[p for p in model.parameters() if p.requires_grad])])
    ends4, grps = check(rows)
    assert grps == [0, -1, 0] and (ends4[1] - ends4[0]) * 4 == lone.numel()
    # padding floats belong to the preceding run: a layout whose slots are rounded up, every tensor a row of its own
    offs2, numels2, rows2 = [0, 4, 12, 16], [3, 6, 1, 8], [0, 1, -1, 2]
    ends4, grps = build_segments(offs2, 24, rows2)
    assert (ends4, grps) == ([1, 3, 4, 6], [0, 1, -1, 2]) and (_expand(ends4, grps, 24) == _brute(offs2, numels2, 24, rows2)).all()
    for bad in (([4, 8], 12, [0, 0]), ([0, 6], 12, [0, 0]), ([0, 4], 10, [0, 0]), ([0, 4], 12, [0])):
        with pytest.raises(ValueError):
            build_segments(*bad)


def test_groups_kernel_mapping_visits_every_float4_once():
    """The restated loops of adamw_groups_kernel reach every float4 of [0, n / 4) exactly once in every regime of the case table, and the
    table holds every regime."""
    regimes = [T.groups_regime(c.n4) for c in T.GROUPS_CASES]
    assert {"below cap", "at cap", "cap + 1", "rounds + ragged"} <= set(regimes), regimes
    assert regimes == ["below cap"] * 6 + ["at cap", "cap + 1", "rounds + ragged"]
    assert T.groups_plan(T.GRID_CAP * T.CHUNK4) == (2048, 2048, 1, 1, 0) and T.groups_plan((T.GRID_CAP + 1) * T.CHUNK4) == (2048, 2049, 1, 2, 0)
    assert T.groups_plan(T.ROUNDS_N4) == (2048, 4102, 2, 3, 777) and T.groups_plan(1500) == (2, 2, 1, 1, 476)
    for n4 in sorted({c.n4 for c in T.GROUPS_CASES} | {1, 255, 256, 1023, 1024, 1025}):
        seen = T.groups_visits(n4)
        assert seen.min() == 1 and seen.max() == 1, n4
    # the tables themselves: sorted runs covering [0, n4), rows inside [-1, n_groups), within the library's limits
    for c in T.GROUPS_CASES:
        assert c.ends == sorted(set(c.ends)) and c.ends[-1] == c.n4 and len(c.ends) == len(c.groups) <= T.MAX_SEGS
        assert all(-1 <= g < c.n_groups for g in c.groups) and 1 <= c.n_groups <= T.MAX_GROUPS
    by = {c.name: c for c in T.GROUPS_CASES}
    assert len(by["max runs"].ends) == T.MAX_SEGS and len(by["one run"].ends) == 1
    assert by["skipped first run"].groups[0] == -1 and by["skipped last run"].groups[-1] == -1
    s = by["seams"].ends
    assert s[0] == 1 and T.CHUNK4 in s and 2 * T.CHUNK4 + 1 in s and 3 * T.CHUNK4 - 1 in s  # a run of one float4; on, after and before a seam
    inner = [e for e in by["40 runs in a chunk"].ends[:-1]]
    # 41 cuts bound 40 runs of 1 to 3 float4 (the run before the first cut and the one after the last are long), all in the second chunk
    assert len(inner) - 1 == 40 and len(by["40 runs in a chunk"].ends) == 42 and inner[0] // T.CHUNK4 == inner[-1] // T.CHUNK4 and all(1 <= b - a <= 3 for a, b in zip(inner, inner[1:]))
    assert max(4 * c.n4 * 4 * 7 for c in T.GROUPS_CASES) < 1e9  # p, g, m, v, three references: below a gigabyte


def test_state_dict_layout_is_torch_adamws():
    """Keys, group order and parameter indices of a multi-group HipAdamW's state_dict() are torch.optim.AdamW's for the same groups; loading
    that optimizer's state after CPU steps restores the per-group step counts and hands the moments to the parameters."""
    import diverse_channel_vit_amd as dcv
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7)), torch.nn.Parameter(torch.randn(2, 2)), torch.nn.Parameter(torch.randn(3))]
    mk = lambda: [dict(params=[ps[0], ps[2]], lr=1e-3, weight_decay=0.05), dict(params=[ps[1]], lr=5e-4, weight_decay=0.0),  # noqa: E731
                  dict(params=[ps[3]], lr=2e-4, weight_decay=0.0)]
    ref = torch.optim.AdamW(mk(), betas=(0.9, 0.999), eps=1e-8)
    for step in range(3):
        for i, p in enumerate(ps):
            p.grad = None if (i == 3 and step < 2) else torch.randn_like(p)  # the last group joins at step 3: its count is 1
        ref.step()
    mine = dcv.HipAdamW(mk(), betas=(0.9, 0.999), eps=1e-8)
    a, b = mine.state_dict(), ref.state_dict()
    assert set(a) == set(b) == {"state", "param_groups"} and a["state"] == {}
    assert [g["params"] for g in a["param_groups"]] == [g["params"] for g in b["param_groups"]] == [[0, 1], [2], [3]]
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert all(ga[k] == gb[k] for k in ("lr", "betas", "eps", "weight_decay"))
    mine.load_state_dict(b)
    assert mine._gsteps == [3, 3, 1]
    a = mine.state_dict()
    assert set(a["state"]) == set(b["state"]) == {0, 1, 2, 3}
    for k in b["state"]:
        assert set(a["state"][k]) == set(b["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        assert torch.equal(a["state"][k]["exp_avg"], b["state"][k]["exp_avg"]) and int(a["state"][k]["step"]) == int(b["state"][k]["step"])
