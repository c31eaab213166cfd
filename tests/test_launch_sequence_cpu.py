"""One block body for every path (dichavit.py: _block_attention / _block_residuals): the launch sequence of each inspection call is the eval
forward's, cut at that call's tap point, plus what the call adds.  Every hip.* wrapper is replaced by a recorder and the model runs on CPU
tensors (4 blocks, D = 192, 3 channels, 32 x 32 images, patch 8: B = 2, N = 49), so no kernel and no GPU is involved."""
import importlib

import pytest
import torch

import diverse_channel_vit_amd as dcv
from diverse_channel_vit_amd import hip

dichavit = importlib.import_module("diverse_channel_vit_amd.dichavit")  # the package attribute of that name is the factory function
DEPTH = 4


class Cfg(dict):
    __getattr__ = dict.get


def _sig(v):
    if torch.is_tensor(v):
        return (tuple(v.shape), str(v.dtype), v.stride())
    if isinstance(v, (list, tuple)):
        return tuple(_sig(e) for e in v)
    return tuple(sorted((k, _sig(e)) for k, e in v.items())) if isinstance(v, dict) else v


@pytest.fixture
def calls(monkeypatch):
    log = []
    for name in dir(hip):
        fn = getattr(hip, name)
        if callable(fn) and not name.startswith("_") and not isinstance(fn, type) and getattr(fn, "__module__", "") == hip.__name__:
            monkeypatch.setattr(hip, name, lambda *a, _n=name, **k: log.append((_n, _sig(a), _sig(k))))
    monkeypatch.setattr(dichavit.DiChaViT, "_check_input", staticmethod(lambda x: None))
    monkeypatch.setitem(dichavit._SIZES, "tiny", (192, DEPTH, 3))
    return log


def _model():
    cfg = Cfg(name="dichavit", pretrained_model_name="tiny", patch_size=8, temperature=0.07, learnable_temp=False, enable_sample=False,
              use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False,
              block_type="block", hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.0, ortho_loss_v1_lambda=0.0,
              drop_path_rate=0.0, gamma_s=1.0, gamma_d=4.0, reverse_pos_pairs=True, use_square=False,
              in_channel_names=["a", "b", "c"], img_size=[32], num_classes=5)
    torch.manual_seed(0)
    model = dcv.dichavit(cfg, mapper={"train": [0, 1, 2]}).eval()
    model.cls_only_tail, model.attn_prescaled = False, True
    return model


def _run(log, fn):
    del log[:]
    fn()
    return list(log)


def test_inspection_calls_run_the_forwards_blocks(calls):
    x = torch.zeros(2, 3, 32, 32)
    model = _model()
    fe = model.feature_extractor
    with torch.no_grad():
        ev = _run(calls, lambda: model(x, "train"))
    # eval forward: 3 operand-copy casts, the tokeniser (im2col, patch GEMM, CLS fill), DEPTH equal blocks, the final norm
    assert [c[0] for c in ev[:6]] == ["cast_bf16", "cast_transpose_bf16", "cast_scaled_ranges", "im2col", "gemm_nt", "fill_cls"]
    body = ev[3:-1]
    per, rest = divmod(len(body) - 3, DEPTH)
    assert rest == 0 and all(body[3 + per * k:3 + per * (k + 1)] == body[3:3 + per] for k in range(DEPTH))
    att = [c[0] for c in body[3:3 + per]].index("attn_fwd")  # the attention's place in a block
    for k in range(DEPTH):
        for pool, last in ((None, "ln_fwd"), ("channel", "ln_pool_channels")):
            t = _run(calls, lambda: fe.get_intermediate_layers(x, n=[k], chunk="train", pool=pool))
            assert [c[0] for c in t[:2]] == ["cast_bf16", "cast_scaled_ranges"]  # the scratch operand copies
            assert t[2:-1] == body[:3 + per * (k + 1)] and t[-1][0] == last, (k, pool)
        for queries in ("channel", "token"):
            t = _run(calls, lambda: fe.get_channel_attention(x, n=[k], chunk="train", queries=queries))
            assert [c[0] for c in t[:2]] == ["cast_bf16", "cast_scaled_ranges"]
            assert t[2:-1] == body[:3 + per * k + att + 1] and t[-1][0] == "attn_channel_mass", (k, queries)
        for rows in (None, 1):
            t = _run(calls, lambda: fe.get_last_selfattention(x, chunk="train", layer_idx=k, query_rows=rows))
            assert [c[0] for c in t[:2]] == ["cast_bf16", "cast_scaled_ranges"]
            assert t[2:-2] == body[:3 + per * k + att] and [c[0] for c in t[-2:]] == ["attn_fwd", "attn_probs"], (k, rows)
            assert dict(t[-2][2])["nq"] == dict(t[-1][2])["nq"] == (49 if rows is None else 1)
