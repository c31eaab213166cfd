"""ChannelVisionTransformer.get_intermediate_layers (models/dichavit.py:665-673) without a GPU: the method's signature, the checks it makes
before any device work, the input check it shares with forward(), and the C ABI it runs on (dcv_ln_pool_channels: host logic only, no launch)."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_SHAPE, ERR_ALIGN, ERR_NULL = 0, -1, -2, -5
ENTRIES = ("dcv_ln_pool_channels", "dcv_ln_pool_channels_ws_floats")


class Cfg(dict):
    """A DictConfig stand-in that copy.deepcopy / pickle can take apart (dunder lookups are not keys)."""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return self.get(k)


def _model(C_=3):
    import diverse_channel_vit_amd as dcv
    base = dict(name="dichavit", pretrained_model_name="tiny", patch_size=8, temperature=0.07, learnable_temp=False, enable_sample=False,
                use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False,
                block_type="block", hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.001, ortho_loss_v1_lambda=0.1,
                drop_path_rate=0.0, gamma_s=0.5, gamma_d=4.0, reverse_pos_pairs=True, use_square=False)
    cfg = Cfg(base, in_channel_names=list(range(C_)), img_size=[32], num_classes=5)
    return dcv.dichavit(cfg, mapper={"train": list(range(C_))})


def test_method_signature_is_the_references():
    from diverse_channel_vit_amd.dichavit import ChannelVisionTransformer
    sig = inspect.signature(ChannelVisionTransformer.get_intermediate_layers)
    ps = list(sig.parameters.values())
    # models/dichavit.py:665: def get_intermediate_layers(self, x, extra_tokens={}, n=1)
    assert [p.name for p in ps] == ["self", "x", "extra_tokens", "n", "chunk", "training_chunks", "new_channel_init", "pool"]
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in ps[:4])
    assert ps[1].default is inspect.Parameter.empty and ps[2].default == {} and ps[3].default == 1
    # the extensions are keyword-only
    assert all(p.kind == p.KEYWORD_ONLY for p in ps[4:])
    assert [p.default for p in ps[4:]] == ["", None, None, None]


def test_cpu_input_raises_as_forward_does():
    model = _model()
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback") as fwd:
        model(x, "train", None)
    with pytest.raises(RuntimeError, match="no CPU fallback") as probe:
        model.feature_extractor.get_intermediate_layers(x, n=2, chunk="train", pool="channel")
    assert str(probe.value) == str(fwd.value)


def test_unlinked_encoder_raises():
    import pickle
    lone = pickle.loads(pickle.dumps(_model().feature_extractor))  # the encoder alone: no owner to run through
    with pytest.raises(RuntimeError, match="not linked"):
        lone.get_intermediate_layers(torch.zeros(1, 3, 32, 32), chunk="train")


@pytest.mark.parametrize("n", [0, 13, -1, True, 1.5, "4", None, [], [12], [-13], [11, -1], [3, 3], [0, 1.0], [[1]]])
def test_bad_n_raises_before_any_device_work(n):
    """The CPU tensor would raise RuntimeError in the input check: ValueError shows that n is checked first."""
    fe = _model().feature_extractor
    with pytest.raises(ValueError):
        fe.get_intermediate_layers(torch.zeros(1, 3, 32, 32), n=n, chunk="train")


def test_bad_pool_raises_before_any_device_work():
    fe = _model().feature_extractor
    for pool in ("cls", "mean", 1, True):
        with pytest.raises(ValueError, match="pool"):
            fe.get_intermediate_layers(torch.zeros(1, 3, 32, 32), chunk="train", pool=pool)


def test_layer_lists():
    from diverse_channel_vit_amd.dichavit import _parse_layers
    assert _parse_layers(1, 12) == [11] and _parse_layers(4, 12) == [8, 9, 10, 11] and _parse_layers(12, 12) == list(range(12))
    assert _parse_layers([11], 12) == [11] and _parse_layers((-1, 0, -4), 12) == [0, 8, 11] and _parse_layers(range(3), 12) == [0, 1, 2]


def test_header_binding_and_library_agree_on_the_entries():
    src = open(os.path.join(ROOT, "include", "dcv.h")).read()
    assert re.search(r"\bint\s+dcv_ln_pool_channels\s*\(", src) and re.search(r"\blong\s+dcv_ln_pool_channels_ws_floats\s*\(", src)
    from diverse_channel_vit_amd import hip
    assert set(ENTRIES) <= set(hip.EXPORTS) and callable(hip.ln_pool_channels)
    lib = hip.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_workspace_sizes_and_refusals_on_the_host():
    """Host logic only: every call below returns before any launch (placeholder addresses are never dereferenced)."""
    from diverse_channel_vit_amd import hip
    lib = hip.load()
    ws = lib.dcv_ln_pool_channels_ws_floats
    # the plan is a function of the shape alone: ceil(2048 / (B C)) splits, at least 8 rows each
    assert ws(64, 8, 196, 384) == 64 * 8 * 4 * 384          # 512 segments: 4 splits of 49 rows
    assert ws(64, 3, 196, 384) == 64 * 3 * 11 * 384         # 192 segments: 11 asked for, 18 rows each -> 11 splits
    assert ws(1, 3, 196, 384) == 3 * 22 * 384               # one image: capped at 196 // 8 = 24 -> 9 rows each -> 22 splits
    assert ws(64, 18, 16, 384) == 64 * 18 * 2 * 384         # 1152 segments of 16 rows: 2 splits
    assert ws(4096, 8, 196, 384) == 0 and ws(2, 3, 1, 192) == 0 and ws(2, 3, 15, 768) == 0  # one workgroup per segment: no workspace
    for bad in ((0, 3, 16, 384), (2, 0, 16, 384), (2, 3, 0, 384), (2, 3, 16, 0), (2, 3, 16, 386), (2, 3, 16, 1028)):
        assert ws(*bad) == ERR_SHAPE, bad
    p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731

    def call(x=256, g=512, b=768, out=1024, B=2, C_=3, n_p=16, D=384, w=2048, wf=1 << 30):
        return lib.dcv_ln_pool_channels(p(x), p(g), p(b), 1e-6, p(out), B, C_, n_p, D, p(w), wf, None)

    for kw in (dict(x=None), dict(g=None), dict(b=None), dict(out=None), dict(w=None)):
        assert call(**kw) == ERR_NULL, kw
    for kw in (dict(D=386), dict(D=1028), dict(D=0), dict(B=0), dict(C_=0), dict(n_p=0), dict(wf=2 * 3 * 2 * 384 - 1)):
        assert call(**kw) == ERR_SHAPE, kw
    for kw in (dict(x=260), dict(g=516), dict(b=772), dict(out=1032), dict(w=2052)):
        assert call(**kw) == ERR_ALIGN, kw


def test_dump_features_defaults_are_unchanged():
    import diverse_channel_vit_amd as dcv
    ps = inspect.signature(dcv.dump_features).parameters
    assert list(ps)[:9] == ["model", "loaders", "feature_dir", "feature_file", "training_chunks", "new_channel_init", "init_first_layer",
                            "channel_combinations", "device"]
    assert list(ps)[9:] == ["layers", "pool"] and ps["layers"].default is None and ps["pool"].default is None
    assert ps["feature_file"].default == "features.npy" and ps["device"].default is None
    with pytest.raises(ValueError, match="pool"):
        dcv.dump_features(_model(), {}, "unused", pool="channel")
    with pytest.raises(ValueError, match="pool"):
        dcv.dump_features(_model(), {}, "unused", layers=2, pool="mean")
