"""DiChaViT.forward_with_features without a GPU: the C ABI of the channel-pool adjoint (dcv_ln_pool_channels_bwd: host logic only, no launch),
the refusals the call makes before any device work, and — with every hip.* wrapper replaced by a recorder, as in test_launch_sequence_cpu — where
the taps' launches stand in the forward and in the hand-written backward."""
import ctypes as C
import os
import re

import pytest
import torch

from test_intermediate_layers_cpu import _model as _cpu_model
from test_launch_sequence_cpu import DEPTH, _model as _rec_model, _run, calls  # noqa: F401  (calls: the recorder fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_SHAPE, ERR_ALIGN, ERR_NULL = 0, -1, -2, -5
ENTRIES = ("dcv_ln_pool_channels_bwd", "dcv_ln_pool_channels_bwd_ws_floats")


def test_header_binding_and_library_agree_on_the_entries():
    src = open(os.path.join(ROOT, "include", "dcv.h")).read()
    assert re.search(r"\bint\s+dcv_ln_pool_channels_bwd\s*\(", src) and re.search(r"\blong\s+dcv_ln_pool_channels_bwd_ws_floats\s*\(", src)
    from diverse_channel_vit_amd import hip
    assert set(ENTRIES) <= set(hip.EXPORTS) and callable(hip.ln_pool_channels_bwd)
    lib = hip.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_workspace_sizes_follow_the_plan_and_refusals_on_the_host():
    """Host logic only: every call below returns before any launch (placeholder addresses are never dereferenced).  The plan: ceil(2048 / (B C))
    splits per segment, at least 8 rows each; one workgroup per (segment, split) plus one per four CLS rows; D floats of dgamma partial each."""
    from diverse_channel_vit_amd import hip
    lib = hip.load()
    ws = lib.dcv_ln_pool_channels_bwd_ws_floats
    assert ws(64, 8, 196, 384) == (64 * 8 * 4 + 16) * 384   # 512 segments: 4 splits of 49 rows; 16 CLS workgroups
    assert ws(2, 4, 7, 192) == (2 * 4 * 1 + 1) * 192         # whole segments (fewer than 2 x 8 rows): one workgroup each
    assert ws(1, 3, 196, 384) == (3 * 22 + 1) * 384          # one image: capped at 196 // 8 = 24 -> 9 rows each -> 22 splits
    assert ws(64, 3, 196, 384) == (64 * 3 * 11 + 16) * 384   # 192 segments: 11 asked for, 18 rows each -> 11 splits
    assert ws(5, 1, 197, 1024) == (5 * 22 + 2) * 1024        # 197 rows: 21 splits of 9 and a last one of 8; 5 images: two CLS workgroups
    for bad in ((0, 3, 16, 384), (2, 0, 16, 384), (2, 3, 0, 384), (2, 3, 16, 0), (2, 3, 16, 6 + 384), (2, 3, 16, 1028)):
        assert ws(*bad) == ERR_SHAPE, bad
    p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    need = ws(2, 3, 16, 384)

    def call(x=256, g=512, dout=768, dx=1024, dg=1280, db=1536, B=2, C_=3, n_p=16, D=384, w=2048, wf=1 << 30):
        return lib.dcv_ln_pool_channels_bwd(p(x), p(g), 1e-6, p(dout), p(dx), p(dg), p(db), B, C_, n_p, D, p(w), wf, None)

    for kw in (dict(x=None), dict(g=None), dict(dout=None), dict(dx=None), dict(w=None)):
        assert call(**kw) == ERR_NULL, kw
    for kw in (dict(D=6), dict(D=1028), dict(D=0), dict(B=0), dict(C_=0), dict(n_p=0), dict(wf=need - 1)):
        assert call(**kw) == ERR_SHAPE, kw
    for kw in (dict(x=260), dict(g=516), dict(dout=772), dict(dx=1028), dict(dg=1284), dict(db=1540), dict(w=2052)):
        assert call(**kw) == ERR_ALIGN, kw


@pytest.mark.parametrize("layers", [0, 13, True, 1.5, "4", None, [], [12], [3, 3], [[1]]])
def test_bad_layers_raise_before_any_device_work(layers):
    """The CPU tensor would raise RuntimeError in the input check: ValueError shows that the argument is checked first."""
    with pytest.raises(ValueError):
        _cpu_model().forward_with_features(torch.zeros(1, 3, 32, 32), "train", layers=layers)


def test_bad_pool_raises_before_any_device_work():
    model = _cpu_model()
    for pool in ("mean", "token", 1, True):
        with pytest.raises(ValueError, match="pool"):
            model.forward_with_features(torch.zeros(1, 3, 32, 32), "train", pool=pool)
    for pool in ("channel", "cls", None):  # the valid ones get as far as the input check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.forward_with_features(torch.zeros(1, 3, 32, 32), "train", pool=pool)


def test_tap_below_a_frozen_prefix_raises_before_any_device_work():
    model = _cpu_model().freeze_prefix(3)
    depth = len(model.feature_extractor.blocks)
    x = torch.zeros(1, 3, 32, 32)
    for layers in ([0], [1, depth - 1], depth):
        with pytest.raises(ValueError, match="frozen prefix"):
            model.forward_with_features(x, "train", layers=layers)
    for layers in ([2], [2, depth - 1], 1):  # block k - 1 = 2 and above are accepted: they reach the input check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.forward_with_features(x, "train", layers=layers)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):  # no gradient, nothing to refuse
        model.forward_with_features(x, "train", layers=[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # x requires a gradient: there is no frozen prefix
        model.forward_with_features(x.clone().requires_grad_(), "train", layers=[0])


def test_only_dichavit_has_the_method():
    from diverse_channel_vit_amd.dichavit import ChannelVisionTransformer, DiChaViT
    assert hasattr(DiChaViT, "forward_with_features") and not hasattr(ChannelVisionTransformer, "forward_with_features")


# ---- launch sequences (recorder; 4 blocks, D = 192, 3 channels, B = 2, N = 49) -------------------------------------------------------------
def _train_model(tail):
    model = _rec_model().train()
    model.cls_only_tail = tail
    model.stochastic_weight_rounding = False
    return model


def _names(log):
    return [c[0] for c in log]


def _step(model, x, taps=None, weights=None, use_out=True):
    """one forward + backward; weights: per tap 1 (it enters the loss) or 0 (it receives no gradient)"""
    model.zero_grad(set_to_none=True)
    if taps is None:
        out, extra = model(x, "train")
        (out.sum() + extra).backward()
        return
    (out, extra), feats = model.forward_with_features(x, "train", **taps)
    loss = sum(f.sum() for f, w in zip(feats, weights) if w)
    if use_out:
        loss = loss + out.sum() + extra
    loss.backward()


@pytest.mark.parametrize("tail", [False, True])
def test_plain_step_is_unchanged_by_a_preceding_tapped_step(calls, tail):
    x = torch.zeros(2, 3, 32, 32)
    model = _train_model(tail)
    before = _run(calls, lambda: _step(model, x))
    _step(model, x, dict(layers=[1, DEPTH - 1], pool="channel"), (1, 1))
    assert _run(calls, lambda: _step(model, x)) == before
    assert "ln_pool_channels" not in _names(before) and "ln_pool_channels_bwd" not in _names(before)


@pytest.mark.parametrize("pool", ["channel", "cls", None])
@pytest.mark.parametrize("tail", [False, True])
def test_inner_taps_add_their_launches_and_nothing_else(calls, tail, pool):
    """Inner taps leave the plain step's launches as they are — the CLS-only tail included — and add one forward launch per tap and one backward
    launch per tap that has a gradient.  The backward launch stands between the norm2 and the norm1 LayerNorm backward of the block above."""
    x = torch.zeros(2, 3, 32, 32)
    model = _train_model(tail)
    plain = _run(calls, lambda: _step(model, x))
    fwd_name = "ln_pool_channels" if pool == "channel" else "ln_fwd"
    bwd_name = "ln_pool_channels_bwd" if pool == "channel" else "ln_bwd"
    tapped = _run(calls, lambda: _step(model, x, dict(layers=[0, 2], pool=pool), (1, 1)))
    one = _run(calls, lambda: _step(model, x, dict(layers=[0, 2], pool=pool), (0, 1)))
    none = _run(calls, lambda: _step(model, x, dict(layers=[0, 2], pool=pool), (0, 0)))
    assert len(tapped) == len(plain) + 4 and len(one) == len(plain) + 3 and len(none) == len(plain) + 2
    # taking the taps' launches out leaves the plain step
    rows = {"channel": None, "cls": 2, None: 2 * 49}[pool]

    def is_tap(c):
        if pool == "channel":
            return c[0] in (fwd_name, bwd_name)
        if c[0] == "ln_fwd":  # the tap's LayerNorm writes fp32 with the final norm's weight; the final norm itself comes last in the forward
            return c[1][3][1] == "torch.float32" and c[1][6] == rows and c is not last_f32_fwd
        return c[0] == "ln_bwd" and c[1][0][1] == "torch.float32" and c[1][7] is None and c is not first_bwd

    for log in (tapped, one, none):
        f32 = [c for c in log if c[0] == "ln_fwd" and c[1][3][1] == "torch.float32"]
        last_f32_fwd = f32[-1]
        first_bwd = next(c for c in log if c[0] == "ln_bwd")
        assert [c for c in log if not is_tap(c)] == plain
    # where the backward launches stand: counted in LayerNorm backwards from the top, block 3 has two (norm2, norm1), then block 2's, ...
    names = _names(tapped)
    if pool == "channel":
        seq = [n for n in names if n in ("ln_bwd", bwd_name)]
        # final norm; block 3: norm2, TAP(2), norm1; block 2: norm2, norm1; block 1: norm2, TAP(0), norm1; block 0: norm2, norm1
        assert seq == ["ln_bwd", "ln_bwd", bwd_name, "ln_bwd", "ln_bwd", "ln_bwd", "ln_bwd", bwd_name, "ln_bwd", "ln_bwd", "ln_bwd"]
    else:
        bw = [c for c in tapped if c[0] == "ln_bwd"]
        first_bwd = bw[0]
        assert [is_tap(c) for c in bw] == [False, False, True, False, False, False, False, True, False, False, False]
    # no cast pass is added: the bf16 copy comes out of the norm1 backward that follows
    assert names.count("cast_bf16") == _names(plain).count("cast_bf16")


@pytest.mark.parametrize("pool", ["channel", None])
def test_tapping_the_last_block_runs_it_on_all_rows(calls, pool):
    x = torch.zeros(2, 3, 32, 32)
    model = _train_model(True)
    full = _train_model(False)
    plain_full = _run(calls, lambda: _step(full, x))
    tapped = _run(calls, lambda: _step(model, x, dict(layers=[DEPTH - 1], pool=pool), (1,)))
    assert len(tapped) == len(plain_full) + 2  # the step without the CLS-only tail, the tap and its backward
    names = _names(tapped)
    bwd_name = "ln_pool_channels_bwd" if pool == "channel" else "ln_bwd"
    lnb = [i for i, n in enumerate(names) if n in ("ln_bwd", "ln_pool_channels_bwd")]
    # the tap's backward follows the final norm's directly and precedes the bf16 cast of the stream gradient
    assert names[lnb[1]] == bwd_name and lnb[1] == lnb[0] + 1 and names[lnb[1] + 1] == "cast_bf16"
    # pool="cls" keeps the tail
    tail_plain = _run(calls, lambda: _step(model, x))
    cls = _run(calls, lambda: _step(model, x, dict(layers=[DEPTH - 1], pool="cls"), (1,)))
    assert len(cls) == len(tail_plain) + 2


def test_a_loss_on_the_taps_alone_runs_the_backward(calls):
    x = torch.zeros(2, 3, 32, 32)
    model = _train_model(True)
    log = _run(calls, lambda: _step(model, x, dict(layers=[1], pool="channel"), (1,), use_out=False))
    names = _names(log)
    assert names.count("ln_pool_channels_bwd") == 1 and "patch_bwd" in names
    assert all(p.grad is not None for p in model.feature_extractor.blocks[0].parameters())
    assert model.classifer_head.weight.grad is None  # `out` received no gradient


def test_frozen_prefix_tap_at_the_boundary_block(calls):
    x = torch.zeros(2, 3, 32, 32)
    model = _train_model(True).freeze_prefix(2)
    plain = _run(calls, lambda: _step(model, x))
    log = _run(calls, lambda: _step(model, x, dict(layers=[1, 2], pool="channel"), (1, 1)))
    assert len(log) == len(plain) + 4 and _names(log).count("ln_pool_channels_bwd") == 2 and "patch_bwd" not in _names(log)
    with pytest.raises(ValueError, match="frozen prefix"):
        model.forward_with_features(x, "train", layers=[0])
