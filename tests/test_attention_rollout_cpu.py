"""ChannelVisionTransformer.get_attention_rollout without a GPU: the method's signature and the checks it makes before any device work, the C
ABI it runs on (dcv_attn_rollout_step / _ps: host logic only, no launch), the float64 helper the GPU tests take their expected values from
(attention_rollout_ref.py) on closed forms, and the fixture rolled from the real reference's maps (tests/golden/attn_rollout.npz)."""
import ctypes as C
import inspect
import os
import pickle
import re

import pytest
import torch

from attention_rollout_ref import rollout, tv
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED, ERR_NULL = 0, -1, -2, -3, -5
ENTRIES = ("dcv_attn_rollout_step", "dcv_attn_rollout_step_ps")


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


def test_method_signature():
    from diverse_channel_vit_amd.dichavit import ChannelVisionTransformer, DiChaViT
    ps = list(inspect.signature(ChannelVisionTransformer.get_attention_rollout).parameters.values())
    assert [p.name for p in ps] == ["self", "x", "extra_tokens", "chunk", "training_chunks", "new_channel_init", "start_layer", "residual", "start"]
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in ps[:3]) and all(p.kind == p.KEYWORD_ONLY for p in ps[3:])
    assert ps[2].default == {} and [p.default for p in ps[3:]] == ["", None, None, 0, 0.5, None]
    assert callable(DiChaViT._probe_rollout)
    doc = ChannelVisionTransformer.get_attention_rollout.__doc__
    assert "1 + c * n_p + i" in doc and "view(B, C, gh, gw)" in doc  # the token order and how to read the per-channel maps


def test_bad_arguments_raise_before_any_device_work(monkeypatch):
    """On a CPU-built model, without loading the library: hip.load would be the first step of the input check."""
    from diverse_channel_vit_amd import hip
    fe = _model().feature_extractor

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(hip, "load", no_load)
    x = torch.zeros(1, 3, 32, 32)
    for r in (1.0, -0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="residual"):
            fe.get_attention_rollout(x, chunk="train", residual=r)
    for s in (12, -13, 1.0, None, "0", True):
        with pytest.raises(ValueError, match="start_layer"):
            fe.get_attention_rollout(x, chunk="train", start_layer=s)
    with pytest.raises(ValueError, match="start"):
        fe.get_attention_rollout(x, chunk="train", start=[1.0, 0.0])


def test_cpu_input_raises_as_forward_does():
    model = _model()
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback") as fwd:
        model(x, "train", None)
    with pytest.raises(RuntimeError, match="no CPU fallback") as probe:
        model.feature_extractor.get_attention_rollout(x, chunk="train")
    assert str(probe.value) == str(fwd.value)


def test_unlinked_encoder_raises():
    lone = pickle.loads(pickle.dumps(_model().feature_extractor))  # the encoder alone: no owner to run through
    with pytest.raises(RuntimeError, match="not linked"):
        lone.get_attention_rollout(torch.zeros(1, 3, 32, 32), chunk="train")


def test_header_binding_and_library_agree_on_the_entries():
    src = open(os.path.join(ROOT, "include", "dcv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    from diverse_channel_vit_amd import hip
    assert set(ENTRIES) <= set(hip.EXPORTS) and callable(hip.attn_rollout_step)
    lib = hip.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_refusals_on_the_host():
    """Host logic only: every call below returns before any launch (placeholder addresses are never dereferenced)."""
    from diverse_channel_vit_amd import hip
    lib = hip.load()
    p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    nbytes = 2 * 81 * 4  # B N floats

    def call(ps, qkv=256, lse=1 << 20, w=2 << 20, out=3 << 20, B=2, N=81, H=6, hd=64, alpha=0.5):
        if ps:
            return lib.dcv_attn_rollout_step_ps(p(qkv), p(lse), p(w), p(out), B, N, H, hd, alpha, None)
        return lib.dcv_attn_rollout_step(p(qkv), p(lse), p(w), p(out), B, N, H, hd, 0.125, alpha, None)

    for ps in (False, True):
        for kw in (dict(qkv=None), dict(lse=None), dict(w=None), dict(out=None)):
            assert call(ps, **kw) == ERR_NULL, kw
        assert call(ps, hd=32) == ERR_UNSUPPORTED
        for kw in (dict(N=0), dict(N=-1), dict(B=0), dict(H=0), dict(B=1 << 30, N=1 << 30)):
            assert call(ps, **kw) == ERR_SHAPE, kw
        for kw in (dict(qkv=264), dict(lse=(1 << 20) + 2), dict(w=(2 << 20) + 1), dict(out=(3 << 20) + 2)):
            assert call(ps, **kw) == ERR_ALIGN, kw
        for alpha in (-0.1, 1.0, float("nan"), float("inf")):
            assert call(ps, alpha=alpha) == ERR_UNSUPPORTED, alpha
        # out must not overlap w: the same buffer, and either one starting inside the other
        for kw in (dict(out=2 << 20), dict(out=(2 << 20) + 4), dict(out=(2 << 20) + nbytes - 4), dict(out=(2 << 20) - nbytes + 4), dict(out=(2 << 20) - 4)):
            assert call(ps, **kw) == ERR_UNSUPPORTED, kw


def _perm(idx):
    P = torch.zeros(len(idx), len(idx), dtype=torch.float64)
    P[torch.arange(len(idx)), torch.tensor(idx)] = 1.0
    return P


def test_helper_on_permutation_matrices():
    """residual = 0 and permutation maps: the one-hot start is carried exactly, last block first."""
    p1, p2, p3 = [1, 2, 3, 0], [2, 0, 3, 1], [0, 3, 1, 2]  # token q attends to token p[q] only
    maps = [_perm(p).expand(2, 3, 4, 4) for p in (p1, p2, p3)]
    r = rollout(maps, 0, 0.0)
    assert r.shape == (2, 4) and r.dtype == torch.float64
    want = torch.zeros(4, dtype=torch.float64)
    want[p1[p2[p3[0]]]] = 1.0  # CLS -> block 2 -> block 1 -> block 0
    assert torch.equal(r[0], want) and torch.equal(r[1], want)
    assert rollout(maps, 1, 0.0)[0].argmax().item() == p2[p3[0]] and rollout(maps, -1, 0.0)[0].argmax().item() == p3[0]
    assert torch.equal(rollout(maps, 2, 0.0), rollout(maps, -1, 0.0))
    start = torch.tensor([[0.0, 0.25, 0.0, 0.75], [1.0, 0.0, 0.0, 0.0]])
    r = rollout(maps, 2, 0.0, start)
    assert r[0].tolist() == [0.0, 0.0, 0.75, 0.25] and r[1].tolist() == [1.0, 0.0, 0.0, 0.0]


def test_helper_on_uniform_attention():
    N = 7
    maps = [torch.full((1, 2, N, N), 1.0 / N, dtype=torch.float64) for _ in range(5)]
    for residual in (0.5, 0.25, 0.0):
        for s in range(5):
            # every step keeps `residual` of what it has and spreads the rest evenly: the e_0 part shrinks by `residual` per block rolled
            k = residual ** (5 - s)
            want = torch.full((N,), (1 - k) / N, dtype=torch.float64)
            want[0] += k
            assert torch.allclose(rollout(maps, s, residual)[0], want, rtol=0, atol=1e-15), (residual, s)
    one = rollout(maps[:1], 0, 0.3)[0]  # one block: residual e_0 + (1 - residual) / N
    assert abs(one[0].item() - (0.3 + 0.7 / N)) <= 1e-15 and torch.allclose(one[1:], torch.full((N - 1,), 0.7 / N, dtype=torch.float64), rtol=0, atol=1e-15)


def test_helper_is_order_sensitive():
    A = torch.tensor([[0.5, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    Bm = torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]], dtype=torch.float64)
    assert not torch.equal(A @ Bm, Bm @ A)
    as4 = lambda M: M.view(1, 1, 3, 3)  # noqa: E731
    e0 = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
    ab = rollout([as4(A), as4(Bm)], 0, 0.0)[0]  # blocks (A, B): the last block B first
    ba = rollout([as4(Bm), as4(A)], 0, 0.0)[0]
    assert torch.equal(ab, e0 @ Bm @ A) and torch.equal(ba, e0 @ A @ Bm) and not torch.equal(ab, ba)
    assert ab.tolist() == [0.0, 0.0, 1.0] and ba.tolist() == [0.0, 0.5, 0.5]
    assert tv(ab.view(1, 3), ba.view(1, 3)) == 0.5 and tv(ab.view(1, 3), ab.view(1, 3)) == 0.0


def test_fixture_sanity():
    meta, a = load_golden("attn_rollout")
    assert [c["name"] for c in meta["cases"]] == ["small", "sub", "tiny48", "base"]
    for case in meta["cases"]:
        r = torch.from_numpy(a[f"{case['name']}/rollout"])
        n_p = (case["img_in"] // case["cfg"]["patch_size"]) ** 2
        N = 1 + len(case["mapper"][case["chunk"]]) * n_p
        assert r.dtype == torch.float32 and tuple(r.shape) == (12, 2, N) and case["B"] == 2 and case["N"] == N and case["depth"] == 12
        assert (r >= 0).all()
        dev = (r.double().sum(-1) - 1).abs().max().item()
        print(f"{case['name']}: N {N}, max |row sum - 1| {dev:.2e}, rollout[11][:, 0] {r[11][:, 0].tolist()}")
        assert dev <= 1e-6
        assert (r[11][:, 0] >= 0.5).all()  # one block rolled: 0.5 e_0 + 0.5 (head-mean CLS row)
        # the start layers differ: the fixture can tell how many blocks were rolled
        assert all(tv(r[s], r[s + 1]) > 1e-3 for s in range(8, 11))
