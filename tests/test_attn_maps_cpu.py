"""ChannelVisionTransformer.get_last_selfattention (models/dichavit.py:654-663) without a GPU: the method's signature, the input check it shares
with forward(), and the C ABI it runs on."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Cfg(dict):
    """A DictConfig stand-in that copy.deepcopy / pickle can take apart (dunder lookups are not keys)."""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return self.get(k)


def _model(C=3):
    import diverse_channel_vit_amd as dcv
    base = dict(name="dichavit", pretrained_model_name="tiny", patch_size=8, temperature=0.07, learnable_temp=False, enable_sample=False,
                use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False,
                block_type="block", hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.001, ortho_loss_v1_lambda=0.1,
                drop_path_rate=0.0, gamma_s=0.5, gamma_d=4.0, reverse_pos_pairs=True, use_square=False)
    cfg = Cfg(base, in_channel_names=list(range(C)), img_size=[32], num_classes=5)
    return dcv.dichavit(cfg, mapper={"train": list(range(C))})


def test_method_signature_is_the_references():
    from diverse_channel_vit_amd.dichavit import ChannelVisionTransformer
    assert hasattr(ChannelVisionTransformer, "get_last_selfattention")
    sig = inspect.signature(ChannelVisionTransformer.get_last_selfattention)
    ps = list(sig.parameters.values())
    # models/dichavit.py:654: def get_last_selfattention(self, x, extra_tokens={}, chunk="", layer_idx=-1)
    assert [p.name for p in ps] == ["self", "x", "extra_tokens", "chunk", "layer_idx", "query_rows"]
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in ps[:5])
    assert ps[1].default is inspect.Parameter.empty
    assert ps[2].default == {} and ps[3].default == "" and ps[4].default == -1
    # the one extension is keyword-only
    assert ps[5].kind == ps[5].KEYWORD_ONLY and ps[5].default is None


def test_cpu_input_raises_as_forward_does():
    model = _model()
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback") as fwd:
        model(x, "train", None)
    with pytest.raises(RuntimeError, match="no CPU fallback") as probe:
        model.feature_extractor.get_last_selfattention(x, chunk="train", layer_idx=0)
    assert str(probe.value) == str(fwd.value)


def test_owner_link_is_not_state_and_follows_copies():
    import copy
    import pickle
    model = _model()
    keys = sorted(model.state_dict().keys())
    fe = model.feature_extractor
    assert fe._owner() is model
    assert "_owner" not in dict(fe.named_modules()) and not any("owner" in k for k in keys)
    cp = copy.deepcopy(model)
    assert cp.feature_extractor._owner() is cp and sorted(cp.state_dict().keys()) == keys
    back = pickle.loads(pickle.dumps(model))
    assert back.feature_extractor._owner() is back
    lone = pickle.loads(pickle.dumps(fe))  # the encoder alone: no owner to run through
    with pytest.raises(RuntimeError, match="not linked"):
        lone.get_last_selfattention(torch.zeros(1, 3, 32, 32), chunk="train")


def test_header_declares_the_probability_entries():
    src = open(os.path.join(ROOT, "include", "dcv.h")).read()
    for name in ("dcv_attn_probs_rows", "dcv_attn_probs_rows_ps"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    from diverse_channel_vit_amd import hip
    assert {"dcv_attn_probs_rows", "dcv_attn_probs_rows_ps"} <= set(hip.EXPORTS)
