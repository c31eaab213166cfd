"""get_last_selfattention on the MI355X: the attention-probabilities kernel (dcv_attn_probs_rows / _ps) against fp32 torch, its consistency with
the forward kernel, and the model method against the real reference's maps (tests/golden/attn_maps.npz, written by make_golden_attn.py).

Bounds.  Kernel: |P - P_ref| <= 3e-4 P_ref + 1e-4 rowmax(P_ref) and every row sum within 1e-4 of 1 (fp32 softmax of the same bf16 q, k; the
kernel's error is the forward's LSE and one exp2).  Model: max |P - P_ref| <= 3e-2 max P_ref per (layer, head), as the eval-logit checks, and
the mean per-row total variation 1/2 sum_k |P - P_ref| <= 1e-2: a CPU emulation on the reference that rounds every Linear's operands and output
to bf16 stays at <= 1.8e-2 relative max error and <= 5.6e-3 mean total variation on these (sharpened) maps, while a wrong layer, a transposed map,
a head swap or a uniform map is at 0.27-0.84."""
import copy
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import dichavit_oracle as orc

pytestmark = pytest.mark.gpu

TV_BOUND = 1e-2


class Cfg(dict):
    """A DictConfig stand-in that copy.deepcopy can take apart (dunder lookups are not keys)."""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return self.get(k)


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def _qkv(B, N, H, seed, prescaled):
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = H * 64
    qkv = torch.randn(B, N, 3 * D, generator=g) * 1.5
    if prescaled:
        qkv[..., :D] *= 64 ** -0.5 * math.log2(math.e)  # q' = q scale log2(e), as the model's pre-scaled operand copies deliver it
    qkv = qkv.to(torch.bfloat16).cuda()
    if N > 1:  # one spiked key against one query (as test_attention_fwd_bwd): a late tile raises the row maximum
        qkv[0, N // 2, :64] *= 4
        qkv[0, N - 1, D:D + 64] = qkv[0, N // 2, :64]
    return qkv


def _probs_ref(qkv, B, N, H, prescaled, nq):
    D = H * 64
    t = qkv.float().view(B, N, 3, H, 64)
    q, k = t[:, :nq, 0].transpose(1, 2), t[:, :, 1].transpose(1, 2)
    s = q @ k.transpose(-1, -2) * (math.log(2.0) if prescaled else 64 ** -0.5)
    return torch.softmax(s, dim=-1)


def _run(hip, qkv, B, N, H, prescaled, nq=None, P=None):
    D = H * 64
    nq_ = N if nq is None else nq
    o = torch.empty(B, N, D, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, N, device="cuda")
    hip.attn_fwd(qkv, o, lse, B, N, H, 64, 64 ** -0.5, nq=nq, prescaled=prescaled)
    if P is None:
        P = torch.empty(B, H, nq_, N, device="cuda")
    hip.attn_probs(qkv, lse, P, B, N, H, 64, 64 ** -0.5, nq=nq, prescaled=prescaled)
    return P, o


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
@pytest.mark.parametrize("B,N,H,Nq", [(2, 1, 6, 1), (2, 33, 6, 33), (1, 64, 3, 64), (2, 65, 6, 65), (2, 81, 12, 81), (1, 200, 6, 1),
                                      (2, 1569, 6, 1569)])
def test_probs_kernel_against_torch(hip, B, N, H, Nq, prescaled):
    qkv = _qkv(B, N, H, seed=N + 7 * H, prescaled=prescaled)
    P, _ = _run(hip, qkv, B, N, H, prescaled, nq=Nq)
    ref = _probs_ref(qkv, B, N, H, prescaled, Nq)
    tol = 3e-4 * ref + 1e-4 * ref.amax(-1, keepdim=True)
    err = (P - ref).abs()
    assert not (err > tol).any(), f"{int((err > tol).sum())} off, max err {err.max().item():.3g}, max rel {(err / ref.clamp_min(1e-30)).max().item():.3g}"
    rs = P.double().sum(-1)
    assert (rs - 1).abs().max().item() <= 1e-4


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
def test_probs_kernel_consistency(hip, prescaled):
    B, N, H = 2, 200, 6
    D = H * 64
    qkv = _qkv(B, N, H, seed=99, prescaled=prescaled)
    P, o = _run(hip, qkv, B, N, H, prescaled)
    # P V against the forward kernel's O
    v = qkv.float().view(B, N, 3, H, 64)[:, :, 2].transpose(1, 2)
    pv = (P @ v).transpose(1, 2).reshape(B, N, D)
    err, tol = (o.float() - pv).abs(), 2e-2 + 2e-2 * pv.abs()
    assert not (err > tol).any(), err.max().item()
    # the CLS row alone equals row 0 of the full map, bit for bit; two calls agree bit for bit
    P1, _ = _run(hip, qkv, B, N, H, prescaled, nq=1)
    assert torch.equal(P1[:, :, 0], P[:, :, 0])
    P2, _ = _run(hip, qkv, B, N, H, prescaled)
    assert torch.equal(P, P2)
    # the kernel writes exactly its [B, H, Nq, N] block: NaN-filled buffer with guard regions before and after
    nq, G = 70, 4096
    buf = torch.full((G + B * H * nq * N + G,), float("nan"), device="cuda")
    inner = buf[G:G + B * H * nq * N].view(B, H, nq, N)
    _run(hip, qkv, B, N, H, prescaled, nq=nq, P=inner)
    torch.cuda.synchronize()
    assert torch.isfinite(inner).all()
    assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + B * H * nq * N:]).all()
    assert torch.equal(inner, P[:, :, :nq])


def _build(case, qk_mult, device):
    import diverse_channel_vit_amd as dcv
    cfg = Cfg(case["cfg"], in_channel_names=[f"c{i}" for i in range(case["n_channels"])], img_size=[case["img"]],
              num_classes=case["num_classes"])
    model = dcv.dichavit(cfg, mapper={k: list(v) for k, v in case["mapper"].items()})
    st = orc.make_state(orc.state_shapes(case["cfg"], case["n_channels"], case["img"], case["num_classes"]), case["seed"])
    D = model.dim
    for k in st:
        if k.endswith("attn.qkv.weight"):
            st[k] = st[k].clone()
            st[k][:2 * D] *= qk_mult  # the fixture's sharpened maps (make_golden_attn.py)
    model.load_state_dict({**st, "adaptive_interface.0": st["proxies"]}, strict=True)
    return model.to(device).eval()


def _batch(case, device):
    x, _ = orc.make_batch(case["batch_seed"], case["B"], len(case["mapper"][case["chunk"]]), case["img_in"], case["num_classes"])
    return x.to(device)


def _mean_tv(P, ref):
    return 0.5 * (P - ref).abs().sum(-1).mean().item()


def test_model_maps_against_the_reference(gpu_device):
    meta, a = load_golden("attn_maps")
    tvs = {}
    for case in meta["cases"]:
        model = _build(case, case["qk_mult"], gpu_device)
        fe = model.feature_extractor
        x = _batch(case, gpu_device)
        for li in case["layers"]:
            ref = torch.from_numpy(a[f"{case['name']}/layer{li}"]).to(gpu_device).float()  # stored in float16
            P = fe.get_last_selfattention(x, chunk=case["chunk"], layer_idx=li)
            assert P.dtype == torch.float32 and P.shape == ref.shape and P.device == x.device and not P.requires_grad
            err = (P - ref).abs().amax(dim=(0, 2, 3))
            bound = 3e-2 * ref.amax(dim=(0, 2, 3))
            assert (err <= bound).all(), f"{case['name']} layer {li}: max err per head {err.tolist()} > {bound.tolist()}"
            tv = _mean_tv(P, ref)
            tvs[(case["name"], li)] = tv
            assert tv <= TV_BOUND, f"{case['name']} layer {li}: mean total variation {tv:.3e}"
        if case["name"] == "small":
            last = fe.get_last_selfattention(x, chunk=case["chunk"], layer_idx=-1)
            assert torch.equal(last, fe.get_last_selfattention(x, chunk=case["chunk"], layer_idx=11))  # the departure: -1 is the last block
            assert case["none_for"] == [-1, 12]  # the reference's answers
            assert fe.get_last_selfattention(x, chunk=case["chunk"], layer_idx=12) is None
            assert fe.get_last_selfattention(x, chunk=case["chunk"], layer_idx=-13) is None
            cls = fe.get_last_selfattention(x, chunk=case["chunk"], layer_idx=11, query_rows=1)
            assert cls.shape == (case["B"], 6, 1, 81) and torch.equal(cls[:, :, 0], last[:, :, 0])
            with pytest.raises(KeyError):
                fe.get_last_selfattention(x)  # the reference's chunk="" default is no mapper key
            # the bound separates: the map of another layer is far outside it
            wrong = _mean_tv(last, torch.from_numpy(a["small/layer5"]).to(gpu_device).float())
            assert wrong >= 10 * TV_BOUND, wrong
        del model
    print("mean total variation per (case, layer):", {k: f"{v:.2e}" for k, v in tvs.items()})


def test_probe_leaves_the_training_step_alone(gpu_device):
    """A probe between loss = ... and loss.backward() must not touch what the backward reads (the stochastically rounded operand copies,
    the pre-scaled q bias, the rounding seed): gradients and the next step's loss are bit-identical to the same sequence without it."""
    from diverse_channel_vit_amd import hip
    from diverse_channel_vit_amd.optim import HipAdamW
    assert hip.is_deterministic()
    meta, _ = load_golden("attn_maps")
    case = meta["cases"][0]
    x = _batch(case, gpu_device)
    y = torch.arange(case["B"], device=gpu_device) % case["num_classes"]
    runs = []
    for probe in (False, True):
        model = _build(case, case["qk_mult"], gpu_device).train()
        assert model.stochastic_weight_rounding
        opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=0.04, model=model)
        out, extra = model(x, case["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss = torch.nn.functional.cross_entropy(out, y) + extra
        if probe:
            model.eval()
            P = model.feature_extractor.get_last_selfattention(x, chunk=case["chunk"], layer_idx=5)
            assert P is not None and torch.isfinite(P).all()
            model.train()
        loss.backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        opt.step()
        opt.zero_grad(set_to_none=True)
        out2, extra2 = model(x, case["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss2 = torch.nn.functional.cross_entropy(out2, y) + extra2
        loss2.backward()
        grads2 = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        runs.append((grads, loss2.detach().clone(), grads2))
        del model, opt
    (g0, l0, h0), (g1, l1, h1) = runs
    assert g0.keys() == g1.keys() and len(g0) > 100
    assert not [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert torch.equal(l0, l1)
    assert not [n for n in h0 if not torch.equal(h0[n], h1[n])]


def test_deepcopy_runs_on_the_copys_weights(gpu_device):
    meta, _ = load_golden("attn_maps")
    case = meta["cases"][0]
    model = _build(case, case["qk_mult"], gpu_device)
    x = _batch(case, gpu_device)
    P0 = model.feature_extractor.get_last_selfattention(x, chunk=case["chunk"], layer_idx=0)
    cp = copy.deepcopy(model)
    assert torch.equal(cp.feature_extractor.get_last_selfattention(x, chunk=case["chunk"], layer_idx=0), P0)
    with torch.no_grad():
        cp.feature_extractor.blocks[0].attn.qkv.weight.mul_(1.5)
    Pc = cp.feature_extractor.get_last_selfattention(x, chunk=case["chunk"], layer_idx=0)
    assert _mean_tv(Pc, P0) > 1e-2
    assert torch.equal(model.feature_extractor.get_last_selfattention(x, chunk=case["chunk"], layer_idx=0), P0)


def test_cls_row_at_12545_tokens(gpu_device):
    """DiChaViT-B, 64 channels at 224 x 224, batch 1 (N = 12 545): the CLS row of the last block's map alone (query_rows=1), against row 0 of
    the full map (7.55 GB)."""
    meta, _ = load_golden("base64_fwd")
    case = dict(cfg=meta["cfg"], n_channels=64, img=224, num_classes=meta["num_classes"], seed=meta["seed"], mapper=meta["mapper"])
    model = _build(case, 1.0, gpu_device)
    x, _ = orc.make_batch(112, 1, 64, 224, meta["num_classes"])
    x = x.to(gpu_device)
    fe = model.feature_extractor
    cls = fe.get_last_selfattention(x, chunk="train", query_rows=1)
    assert cls.shape == (1, 12, 1, 12545)
    assert (cls.double().sum(-1) - 1).abs().max().item() <= 1e-4
    full = fe.get_last_selfattention(x, chunk="train")
    assert full.shape == (1, 12, 12545, 12545)
    row0 = full[:, :, 0].clone()
    del full
    assert torch.equal(row0, cls[:, :, 0])
