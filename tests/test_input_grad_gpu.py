"""Input-image gradients on the MI355X: the dcv_patch_dgrad kernel against fp32 torch on the same bf16 operands, and x.grad of the model — in a
training step, in a frozen-weight saliency call (data-only backward), through channel sampling, token drop and the input affine, for other
dtypes and layouts — against the fp64 oracle's autograd and the real reference's (tests/golden/input_grad.npz).

Bounds.  Kernel: |dx - ref| <= 1e-5 (|dY| |W|) |scale| elementwise against fp64, the fp32-summation level of a K <= 768 dot product.  Model: per image and
channel, relative L2 <= 5e-2 and cosine >= 0.998 (DESIGN.md §4's gradient bounds).  Everything that should not change is compared bit for bit."""
import random

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import dichavit_oracle as orc
from test_input_grad_cpu import case_input, fixture_grad, grad_agreement, oracle_input_grad

pytestmark = pytest.mark.gpu

REL_BOUND, COS_BOUND = 5e-2, 0.998


class Cfg(dict):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return self.get(k)


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _dgrad_ref(dY, W, ch_idx, scale, B, Ct, H, Wimg, P):
    """fp64 torch on the same bf16 operands: the GEMM, the per-channel scale and the col2im; plus the elementwise error scale |dY| |W| |s|."""
    Cc = ch_idx.numel()
    hp, wp = H // P, Wimg // P
    s = scale if scale is not None else torch.ones(Cc, device=dY.device)

    def col2im(G, sc):
        G = G.view(B, Cc, hp, wp, P, P).permute(0, 1, 2, 4, 3, 5).reshape(B, Cc, hp * P, wp * P) * sc.view(1, Cc, 1, 1)
        out = torch.zeros(B, Ct, H, Wimg, dtype=torch.float64, device=dY.device)
        out[:, ch_idx.long(), :hp * P, :wp * P] = G
        return out

    s = s.double()
    return col2im(dY.double() @ W.double(), s), col2im(dY.double().abs() @ W.double().abs(), s.abs())


# (P, D, B, Ct, channel positions, H, W, scale): both patch sizes and all widths; borders (H, W not multiples of P), H != W; channel subsets in
# permuted order; M = B*C*n never a multiple of a 16-token tile or of the workgroup count; patch rows of 1, 2 and 3 tiles (w = 17, 21, 34)
KCASES = [
    (16, 384, 2, 8, list(range(8)), 224, 224, False),
    (8, 192, 3, 5, [4, 0, 2], 36, 44, True),
    (16, 768, 1, 4, [3, 1], 40, 52, False),
    (8, 768, 2, 3, [2, 0, 1], 72, 40, True),
    (16, 192, 2, 2, [1], 48, 272, True),
    (8, 384, 1, 6, [5, 1, 3, 0], 136, 168, False),
    (8, 384, 3, 2, [1, 0], 20, 276, True),
    (16, 384, 5, 3, [2, 0], 33, 20, True),
]


@pytest.mark.parametrize("P,D,B,Ct,chans,H,Wimg,use_scale", KCASES)
def test_patch_dgrad_against_torch(hip, P, D, B, Ct, chans, H, Wimg, use_scale):
    g = torch.Generator(device="cpu").manual_seed(P * 1000 + D + H)
    Cc = len(chans)
    n = (H // P) * (Wimg // P)
    dY = (torch.randn(B * Cc * n, D, generator=g) * 1e-3).to(torch.bfloat16).cuda()
    W = (torch.randn(D, P * P, generator=g) * 0.05).to(torch.bfloat16).cuda()
    ch_idx = torch.tensor(chans, dtype=torch.int32, device="cuda")
    scale = (torch.rand(Cc, generator=g) * 2 - 0.5).cuda() if use_scale else None
    ref, mag = _dgrad_ref(dY, W, ch_idx, scale, B, Ct, H, Wimg, P)
    # NaN-prefilled output between guard regions: every element is written, nothing outside
    G, numel = 4096, B * Ct * H * Wimg
    buf = torch.full((G + numel + G,), float("nan"), device="cuda")
    dx = buf[G:G + numel].view(B, Ct, H, Wimg)
    hip.patch_dgrad(dY, W, ch_idx, dx, B, Ct, Cc, H, Wimg, P, scale=scale)
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all(), f"{int((~torch.isfinite(dx)).sum())} elements not written"
    assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + numel:]).all(), "guard region overwritten"
    unused = [c for c in range(Ct) if c not in chans]
    if unused:
        assert not dx[:, unused].any(), "channels outside ch_idx must be exactly 0"
    Hh, Ww = H // P * P, Wimg // P * P
    assert not dx[:, :, Hh:].any() and not dx[:, :, :, Ww:].any(), "the border the conv drops must be exactly 0"
    err = (dx.double() - ref).abs()
    tol = 1e-5 * mag
    assert not (err > tol).any(), f"{int((err > tol).sum())} off, max err {err.max().item():.3g} (max |ref| {ref.abs().max().item():.3g})"
    dx2 = torch.empty_like(dx)
    hip.patch_dgrad(dY, W, ch_idx, dx2, B, Ct, Cc, H, Wimg, P, scale=scale)
    assert torch.equal(dx, dx2), "two calls differ"


def test_patch_dgrad_rejects_unsupported_shapes(hip):
    dY = torch.zeros(2 * 16, 256, dtype=torch.bfloat16, device="cuda")
    W = torch.zeros(256, 64, dtype=torch.bfloat16, device="cuda")
    ch = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="dcv_patch_dgrad failed: .*unsupported"):
        hip.patch_dgrad(dY, W, ch, torch.empty(2, 1, 32, 32, device="cuda"), 2, 1, 1, 32, 32, 8)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _model(case, device, **cfg_over):
    import diverse_channel_vit_amd as dcv
    base = dict(case["cfg"], **cfg_over)
    cfg = Cfg(base, in_channel_names=[f"c{i}" for i in range(case["n_channels"])], img_size=[case["img"]], num_classes=case["num_classes"])
    model = dcv.dichavit(cfg, mapper={k: list(v) for k, v in case["mapper"].items()})
    st = orc.make_state(orc.state_shapes(base, case["n_channels"], case["img"], case["num_classes"]), case["seed"])
    model.load_state_dict({**st, "adaptive_interface.0": st["proxies"]})
    return model.to(device).train(bool(case["train"])), st


def _encoder_node(out):
    """the _EncoderFn node of a model output's graph (its ctx: the saved state)"""
    todo, seen = [out.grad_fn], set()
    while todo:
        node = todo.pop()
        if node is None or id(node) in seen:
            continue
        seen.add(id(node))
        if type(node).__name__ == "_EncoderFnBackward":
            return node
        todo.extend(f for f, _ in node.next_functions)
    raise AssertionError("no encoder node in the graph")


def _case(name):
    meta, arrays = load_golden("input_grad")
    return {c["name"]: c for c in meta["cases"]}[name], arrays


def _model_loss(model, case, x, y):
    """the fixture's loss: CE + extra in training, sum_b logits[b, y_b] in eval"""
    if case["train"]:
        out, extra = model(x, case["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        return torch.nn.functional.cross_entropy(out, y) + extra
    out = model(x, case["chunk"], case["training_chunks"], init_first_layer=None, new_channel_init=case["new_channel_init"])
    return out.gather(1, y[:, None]).sum()


def _check_against(name, g, ref):
    rel, cos = grad_agreement(np.asarray(g, dtype=np.float64), np.asarray(ref, dtype=np.float64))
    print(f"{name}: x.grad per (image, channel) rel L2 max {rel.max():.3e}, cosine min {cos.min():.6f}")
    assert rel.max() <= REL_BOUND and cos.min() >= COS_BOUND, (name, rel.max(), cos.min())


def test_reference_fixture_all_cases(gpu_device):
    meta, arrays = load_golden("input_grad")
    for case in meta["cases"]:
        model, _ = _model(case, gpu_device)
        x, y = case_input(case)
        x = x.to(gpu_device).requires_grad_(True)
        _model_loss(model, case, x, y.to(gpu_device)).backward()
        g = x.grad.detach().cpu().double().numpy()
        if case["rows"] is not None:
            g = g[:, :, :case["rows"]]
        if case["name"] == "ragged":
            P = case["cfg"]["patch_size"]
            assert not g[:, :, case["H"] // P * P:].any() and not g[:, :, :, case["W"] // P * P:].any()
        _check_against("fixture " + case["name"], g, fixture_grad(arrays, case))


def test_train_step_input_grad_and_bit_identical_params(gpu_device):
    case, _ = _case("so2sat")
    x, y = case_input(case)
    yd = y.to(gpu_device)
    m1, st = _model(case, gpu_device)
    m2, _ = _model(case, gpu_device)
    xg = x.to(gpu_device).requires_grad_(True)
    loss1 = _model_loss(m1, case, xg, yd)
    loss1.backward()
    loss2 = _model_loss(m2, case, x.to(gpu_device), yd)
    loss2.backward()
    assert torch.equal(loss1.detach(), loss2.detach())
    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert n1 == n2 and (p1.grad is None) == (p2.grad is None), n1
        if p1.grad is not None:
            assert torch.equal(p1.grad, p2.grad), f"{n1}: gradient changed by x.requires_grad"
    sd = {k: v.double() for k, v in st.items()}
    ref, _ = oracle_input_grad(case, sd, x.double(), y)
    _check_against("train step vs oracle", xg.grad.cpu().double().numpy(), ref.numpy())


def test_eval_saliency_frozen_weights_is_data_only(gpu_device, monkeypatch):
    from diverse_channel_vit_amd import hip as h
    case, _ = _case("sub")
    model, st = _model(case, gpu_device)
    x, y = case_input(case)
    yd = y.to(gpu_device)
    # weights requiring grad: the full backward (weight gradients computed and dropped by autograd.grad)
    xa = x.to(gpu_device).requires_grad_(True)
    dx_full, = torch.autograd.grad(_model_loss(model, case, xa, yd), xa)
    for p in model.parameters():
        p.requires_grad_(False)

    def forbidden(*a, **k):
        raise AssertionError("a weight-gradient GEMM ran in a data-only backward")

    monkeypatch.setattr(h, "gemm_tn_acc", forbidden)
    monkeypatch.setattr(h, "gemm_tn_acc_group", forbidden)
    arena_before = model._grad_arena
    new_arena = []
    monkeypatch.setattr(model, "_new_grad_arena", lambda: new_arena.append(1))
    xb = x.to(gpu_device).requires_grad_(True)
    dx, = torch.autograd.grad(_model_loss(model, case, xb, yd), xb)
    assert not new_arena and model._grad_arena is arena_before
    assert all(p.grad is None for p in model.parameters())
    assert torch.equal(dx, dx_full), "the data-only backward changed the input gradient"
    sd = {k: v.double() for k, v in st.items()}
    ref, _ = oracle_input_grad(case, sd, x.double(), y)
    _check_against("frozen saliency vs oracle", dx.cpu().double().numpy(), ref.numpy())


def test_data_only_backward_keeps_no_im2col_rows(gpu_device):
    case, _ = _case("base")
    model, _ = _model(case, gpu_device)
    for p in model.parameters():
        p.requires_grad_(False)
    x, _ = case_input(case)
    x = x.to(gpu_device).requires_grad_(True)
    out = model(x, "train", None)
    st = _encoder_node(out).st
    assert st["data_only"] and "Xp" not in st and st["dx_req"]
    out.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()


def test_no_input_grad_saves_nothing_new(gpu_device):
    case, _ = _case("so2sat")
    model, _ = _model(case, gpu_device)
    x, y = case_input(case)
    out, extra = model(x.to(gpu_device), "train", None)
    st = _encoder_node(out).st
    assert "Xp" in st and "data_only" not in st and "dx_req" not in st and "Wp" not in st


def test_create_graph_raises(gpu_device):
    case, _ = _case("sub")
    model, _ = _model(case, gpu_device)
    x, y = case_input(case)
    x = x.to(gpu_device).requires_grad_(True)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(_model_loss(model, case, x, y.to(gpu_device)), x, create_graph=True)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# channel routing
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_hcs_pinned_subset_unsampled_channels_zero(gpu_device):
    case, _ = _case("so2sat")
    model, st = _model(case, gpu_device, enable_sample=True)
    picked = [3, 1]
    model.hcs_sampler = lambda m, chunk, cur: ([cur[i] for i in picked], list(picked))
    x, y = case_input(case)
    xg = x.to(gpu_device).requires_grad_(True)
    out, extra = model(xg, "train", None)
    (torch.nn.functional.cross_entropy(out, y.to(gpu_device)) + extra).backward()
    g = xg.grad
    rest = [c for c in range(x.shape[1]) if c not in picked]
    assert not g[:, rest].any(), "unsampled channels must get exactly 0"
    assert g[:, picked].abs().amax(dim=(2, 3)).min() > 0
    sd = {k: v.double().requires_grad_(False) for k, v in st.items()}
    xr = x.double().requires_grad_(True)
    loss = orc.train_loss(sd, xr, y, case["cfg"], picked, picked)[0]
    ref, = torch.autograd.grad(loss, xr)
    _check_against("hcs", g[:, picked].cpu().double().numpy(), ref[:, picked].numpy())


def test_token_drop_keeps_ortho_gradient_of_dropped_patches(gpu_device):
    case, _ = _case("so2sat")
    model, st = _model(case, gpu_device, dropout_tokens_hcs="channel")
    x, y = case_input(case)
    Cc, P = x.shape[1], case["cfg"]["patch_size"]
    n = (x.shape[2] // P) * (x.shape[3] // P)
    seed = next(s for s in range(1000) if len(orc.token_keep("channel", Cc, n, random.Random(s))) < 1 + Cc * n)  # a draw that drops channels
    keep = orc.token_keep("channel", Cc, n, random.Random(seed))
    dropped = [c for c in range(Cc) if 1 + c * n not in keep]
    random.seed(seed)
    xg = x.to(gpu_device).requires_grad_(True)
    out, extra = model(xg, "train", None)
    (torch.nn.functional.cross_entropy(out, y.to(gpu_device)) + extra).backward()
    g = xg.grad
    assert dropped and g[:, dropped].abs().amax(dim=(2, 3)).min() > 0, "dropped tokens still carry the ortho-loss gradient"
    sd = {k: v.double() for k, v in st.items()}
    xr = x.double().requires_grad_(True)
    cfg = dict(case["cfg"], dropout_tokens_hcs="channel")
    loss = orc.train_loss(sd, xr, y, cfg, list(range(Cc)), list(range(Cc)), keep=keep)[0]
    ref, = torch.autograd.grad(loss, xr)
    _check_against("token drop", g.cpu().double().numpy(), ref.numpy())


def test_input_normalisation_chain_rule(gpu_device):
    case, _ = _case("sub")
    model, st = _model(case, gpu_device)
    mean = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], dtype=np.float32)
    std = np.array([0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5], dtype=np.float32)
    model.set_input_normalisation(mean, std)
    x, y = case_input(case)
    raw = (x * 40 + 128).clamp(0, 255)  # raw float pixels
    xg = raw.to(gpu_device).requires_grad_(True)
    dx, = torch.autograd.grad(_model_loss(model, case, xg, y.to(gpu_device)), xg)
    ids = case["mapper"][case["chunk"]]  # the affine is indexed by global channel id
    m, s = torch.from_numpy(mean[ids]).double().view(1, -1, 1, 1), torch.from_numpy(std[ids]).double().view(1, -1, 1, 1)
    xr = raw.double().requires_grad_(True)
    sd = {k: v.double() for k, v in st.items()}
    g_norm, _ = oracle_input_grad(case, sd, ((xr / 255.0 - m) / s).detach(), y)
    ref = g_norm / (255.0 * s)
    _check_against("input affine", dx.cpu().double().numpy(), ref.numpy())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# dtype and layout
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_dtype_layout_reuse_and_accumulation(gpu_device):
    case, _ = _case("ragged")
    model, _ = _model(case, gpu_device)
    x, y = case_input(case)
    yd = y.to(gpu_device)
    x32 = x.to(gpu_device).requires_grad_(True)
    g32, = torch.autograd.grad(_model_loss(model, case, x32, yd), x32)
    # float64 input: the gradient comes back in float64, the same values
    x64 = x.double().to(gpu_device).requires_grad_(True)
    g64, = torch.autograd.grad(_model_loss(model, case, x64, yd), x64)
    assert g64.dtype == torch.float64 and torch.equal(g64, g32.double())
    # non-contiguous input: same values, the caller's layout
    xnc = x.to(gpu_device).transpose(2, 3).contiguous().transpose(2, 3).requires_grad_(True)
    assert not xnc.is_contiguous()
    gnc, = torch.autograd.grad(_model_loss(model, case, xnc, yd), xnc)
    assert torch.equal(gnc, g32)
    # x used twice in the graph: the model's gradient plus that of the other use
    x2 = x.to(gpu_device).requires_grad_(True)
    loss = _model_loss(model, case, x2, yd) + x2.pow(2).sum()
    loss.backward()
    assert torch.equal(x2.grad, g32 + 2 * x2.detach())
    # two backwards accumulate into x.grad
    x3 = x.to(gpu_device).requires_grad_(True)
    _model_loss(model, case, x3, yd).backward()
    _model_loss(model, case, x3, yd).backward()
    assert torch.equal(x3.grad, g32 + g32)
