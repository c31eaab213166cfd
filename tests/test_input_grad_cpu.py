"""Input-image gradients without a GPU: the argument checks of dcv_patch_dgrad (host logic only, no device call), and the fp64 oracle's
autograd x.grad against the real reference's (tests/golden/input_grad.npz, written by make_golden_input_grad.py) — which pins the oracle the
GPU tests compare the model with."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import dichavit_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED, ERR_NULL = 0, -1, -2, -3, -5


@pytest.fixture(scope="module")
def lib():
    from diverse_channel_vit_amd import hip
    return hip.load()


def _call(lib, dY=256, W=512, ch=768, scale=None, dx=1024, B=2, Ct=3, Cc=3, H=32, Wimg=32, P=8, D=384):
    """Placeholder device addresses (never dereferenced: every case below fails on the host before any launch)."""
    p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    return lib.dcv_patch_dgrad(p(dY), p(W), p(ch), p(scale), p(dx), B, Ct, Cc, H, Wimg, P, D, None)


def test_header_and_binding_declare_the_entry():
    src = open(os.path.join(ROOT, "include", "dcv.h")).read()
    assert re.search(r"\bint\s+dcv_patch_dgrad\s*\(", src)
    from diverse_channel_vit_amd import hip
    assert "dcv_patch_dgrad" in hip.EXPORTS and callable(hip.patch_dgrad)


def test_entry_null_arguments(lib):
    assert _call(lib, dY=None) == ERR_NULL
    assert _call(lib, W=None) == ERR_NULL
    assert _call(lib, ch=None) == ERR_NULL
    assert _call(lib, dx=None) == ERR_NULL


@pytest.mark.parametrize("kw", [dict(B=0), dict(Cc=0), dict(Ct=0), dict(Ct=2, Cc=3), dict(P=0), dict(P=6), dict(Wimg=30), dict(H=7),
                                dict(Wimg=4), dict(P=16, H=12), dict(D=0), dict(B=-1)])
def test_entry_shape_errors(lib, kw):
    assert _call(lib, **kw) == ERR_SHAPE


@pytest.mark.parametrize("kw", [dict(P=4), dict(P=12), dict(P=32, H=64, Wimg=64), dict(D=256), dict(D=96), dict(D=1024), dict(D=385)])
def test_entry_unsupported(lib, kw):
    assert _call(lib, **kw) == ERR_UNSUPPORTED


def test_entry_alignment(lib):
    assert _call(lib, dY=264) == ERR_ALIGN
    assert _call(lib, dx=1032) == ERR_ALIGN


def test_python_wrapper_refuses_cpu_tensors():
    from diverse_channel_vit_amd import hip
    dY = torch.zeros(2 * 16, 384, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        hip.patch_dgrad(dY, torch.zeros(384, 64, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.int32), torch.zeros(2, 1, 32, 32), 2, 1, 1,
                        32, 32, 8)


def case_input(case):
    """x (requires grad) and labels of a fixture case: make_batch on the larger side, cropped to H x W."""
    x, y = orc.make_batch(case["batch_seed"], case["B"], len(case["mapper"][case["chunk"]]), max(case["H"], case["W"]), case["num_classes"])
    return x[:, :, :case["H"], :case["W"]].contiguous(), y


def oracle_input_grad(case, sd, x, y):
    """x.grad of the fixture's loss through the oracle (dtype of sd / x)."""
    cfg, mapper, chunk = case["cfg"], case["mapper"], case["chunk"]
    x = x.clone().requires_grad_(True)
    ch = list(mapper[chunk])
    idx = list(range(len(ch)))
    if case["train"]:
        loss = orc.train_loss(sd, x, y, cfg, ch, idx)[0]
    else:
        rows = None
        if case["training_chunks"] is not None:
            rows = orc.eval_channel_embed(sd["feature_extractor.patch_embed.channel_embed.weight"], mapper, chunk, case["training_chunks"],
                                          case["new_channel_init"])
        out, _ = orc.forward(sd, x, cfg, ch, idx, channel_embed_rows=rows)
        loss = out.gather(1, y[:, None]).sum()
    g, = torch.autograd.grad(loss, x)
    return g, loss


def fixture_grad(arrays, case):
    return arrays[case["name"] + "/grad"].astype(np.float64) * float(arrays[case["name"] + "/scale"])


def grad_agreement(g, ref):
    """per (image, channel): relative L2 error and cosine of g against ref (both [B, C, H, W] float64 arrays)"""
    B, Cc = ref.shape[:2]
    g, ref = g.reshape(B, Cc, -1), ref.reshape(B, Cc, -1)
    rel = np.linalg.norm(g - ref, axis=-1) / np.linalg.norm(ref, axis=-1)
    cos = (g * ref).sum(-1) / (np.linalg.norm(g, axis=-1) * np.linalg.norm(ref, axis=-1))
    return rel, cos


def test_oracle_matches_the_reference_fixture():
    meta, arrays = load_golden("input_grad")
    assert [c["name"] for c in meta["cases"]] == ["so2sat", "sub", "jumpcp", "ragged", "base"]
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    for case in meta["cases"]:
        st = orc.make_state(orc.state_shapes(case["cfg"], case["n_channels"], case["img"], case["num_classes"]), case["seed"], dtype=torch.float64)
        x, y = case_input(case)
        g, loss = oracle_input_grad(case, st, x.double(), y)
        g = g.numpy()
        if case["rows"] is not None:
            g = g[:, :, :case["rows"]]
        ref = fixture_grad(arrays, case)
        assert g.shape == ref.shape, case["name"]
        rel, cos = grad_agreement(g, ref)
        print(f"{case['name']}: loss {loss.item():.6f} (reference {float(arrays[case['name'] + '/loss']):.6f}), rel L2 max {rel.max():.2e}, "
              f"cosine min {cos.min():.8f}")
        assert abs(loss.item() - float(arrays[case["name"] + "/loss"])) <= 1e-4 * max(1.0, abs(loss.item())), case["name"]
        # float16 storage (2^-11 relative) plus fp32-vs-fp64 summation order
        assert rel.max() <= 2e-3 and cos.min() >= 0.99999, (case["name"], rel.max(), cos.min())
        if case["name"] == "ragged":  # the border the conv drops (36 = 4*8 + 4 rows, 44 = 5*8 + 4 columns) gets exactly 0
            P = case["cfg"]["patch_size"]
            Hh, Ww = case["H"] // P * P, case["W"] // P * P
            assert not ref[:, :, Hh:].any() and not ref[:, :, :, Ww:].any() and not g[:, :, Hh:].any() and not g[:, :, :, Ww:].any()
