"""Masked patch tokens on the MI355X: the two kernels of csrc/mask_tokens.hip bit for bit, the model with masks= against the fp64 oracle with
the masking restated in float64, and the invariants of forward_views(masks=, patch_views=).

Bounds.  Kernels: torch.equal (the forward against the EPI_PATCH epilogue itself; the backward on small integers, whose sums are exact).  Model:
the bounds tests/test_feature_taps_gpu.py states for the same quantities on the same fixture — 3e-2 of max |ref| for the logits and the patch
tokens, check_grads' rel L2 <= 5e-2 and cos >= 0.998 for every parameter gradient (mask_token.grad among them), test_input_grad_gpu's per
(image, channel) bounds for x.grad.  The loss is CE + extra + s <W, patch tokens> with a fixed random W and s chosen on the oracle's numbers so
that the patch term alone gives blocks.0.attn.qkv.weight at least the gradient norm of the rest."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle import dichavit_oracle as orc
from switch_pairs import install_recorder
from test_input_grad_cpu import grad_agreement
from test_model_gpu import build, check_grads

pytestmark = pytest.mark.gpu

EPS = 1e-6
QKV0 = "feature_extractor.blocks.0.attn.qkv.weight"
MT = "feature_extractor.mask_token"


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).cuda()


def _kernel_mask(B, C, n):
    """the first and the last token, a whole channel, a whole image, nothing in one image (B >= 3, C >= 2)"""
    m = torch.zeros(B, C * n, dtype=torch.uint8)
    m[0, 0] = m[0, C * n - 1] = 1
    m[0, n:2 * n] = 1  # channel 1 of image 0
    m[1] = 1           # image 1 whole; image 2: nothing
    return m.cuda()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_token", [False, True], ids=["channel_pos", "per_token_pos"])
@pytest.mark.parametrize("D", [384, 192])
def test_forward_kernel_bit_for_bit(hip, D, per_token):
    B, C, n, K = 3, 2, 5, 64
    T = C * n
    Ct, nt = (1, T) if per_token else (C, n)  # the per-token positional mode: one pseudo-channel of C n positions
    Xp = _rand(B * T, K, seed=1).bfloat16()
    W = _rand(D, K, seed=2, scale=0.1).bfloat16()
    bias, mt = _rand(D, seed=3), _rand(D, seed=4)
    E = torch.zeros(1, D, device="cuda") if per_token else _rand(C, D, seed=5)
    pos = _rand(1 + nt, D, seed=6)
    mask = _kernel_mask(B, C, n)

    def project(w, b):
        xs = torch.full((B, 1 + T, D), 7.0, device="cuda")
        Y = torch.empty(B * T, D, device="cuda")
        hip.gemm_nt(Xp, w, hip.EPI_PATCH, xs, bias=b, out2=Y, aux=E, aux2=pos, T=T, n=nt, ldo=D, ldo2=D, ldaux=D)
        return xs, Y

    want_masked, _ = project(torch.zeros_like(W), mt)  # every row holds what a masked row must hold
    plain, Y0 = project(W, bias)
    xs, Y = project(W, bias)
    hip.mask_tokens_fwd(xs, mask, mt, E, pos, B, Ct, nt, D)
    torch.cuda.synchronize()
    mb = mask.bool()
    assert torch.equal(xs[:, 1:][mb], want_masked[:, 1:][mb])
    assert torch.equal(xs[:, 1:][~mb], plain[:, 1:][~mb]) and not torch.equal(xs[:, 1:][mb], plain[:, 1:][mb])
    assert torch.equal(xs[:, 0], plain[:, 0]) and bool((xs[:, 0] == 7.0).all()) and torch.equal(Y, Y0)
    hip.mask_tokens_fwd(plain, mask.bool(), mt, E, pos, B, Ct, nt, D)  # a bool mask is taken as it is
    assert torch.equal(plain, xs)


@pytest.mark.parametrize("kind", ["mixed", "none", "all"])
@pytest.mark.parametrize("ortho", [True, False], ids=["ortho", "no_ortho"])
@pytest.mark.parametrize("B,D", [(3, 384), (3, 192), (30, 384)])  # (30, ...): 300 rows, two parts of the fixed partition
def test_backward_kernel_bit_for_bit(hip, reduction_mode, B, D, ortho, kind):
    C, n = 2, 5
    T = C * n
    g = torch.Generator().manual_seed(B + D)
    dx = torch.randint(-8, 9, (B, 1 + T, D), generator=g).float().cuda()  # small integers: every sum is exact
    dYl = torch.randint(-4, 5, (B * T, D), generator=g).float().cuda() if ortho else None
    mask = {"mixed": _kernel_mask(B, C, n), "none": torch.zeros(B, T, dtype=torch.uint8, device="cuda"),
            "all": torch.ones(B, T, dtype=torch.uint8, device="cuda")}[kind]
    dYb = torch.empty(B * T, D, dtype=torch.bfloat16, device="cuda")
    dE, dpos, dcls = torch.zeros(C, D, device="cuda"), torch.zeros(1 + n, D, device="cuda"), torch.zeros(1, 1, D, device="cuda")
    hip.patch_bwd(dx, dYl, dYb, dE, dpos, dcls, B, C, n, D)
    before = dYb.clone()
    dmt = torch.zeros(D, device="cuda")
    hip.mask_tokens_bwd(dx, mask, dYl, dYb, dmt, B, C, n, D)
    torch.cuda.synchronize()
    mb = mask.bool().view(-1)
    assert torch.equal(dmt, dx[:, 1:].reshape(B * T, D)[mb].sum(0))
    want = dYl[mb].bfloat16() if ortho else torch.zeros(int(mb.sum()), D, dtype=torch.bfloat16, device="cuda")
    assert torch.equal(dYb[mb], want) and torch.equal(dYb[~mb], before[~mb])
    assert torch.equal(dE, dx[:, 1:].view(B, C, n, D).sum((0, 2))) and torch.equal(dpos[1:], dx[:, 1:].view(B, C, n, D).sum((0, 1)))  # patch_bwd's: untouched
    dmt2 = torch.zeros(D, device="cuda")
    hip.mask_tokens_bwd(dx, mask, dYl, before.clone(), dmt2, B, C, n, D, ws=torch.empty(hip.load().dcv_mask_tokens_bwd_ws_floats(B, C, n, D), device="cuda"))
    assert torch.equal(dmt2, dmt)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the model against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _model_mask(B, C, n, seed=77):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(B, C * n, generator=g) < 0.3
    m[0, :n] = True   # a whole channel
    m[B - 1] = False  # nothing in the last image
    return m


def _mask_token_value(D):
    return 0.05 * torch.randn(1, 1, D, generator=torch.Generator().manual_seed(99), dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _oracle(name="so2sat_s", ortho=True):
    """The oracle's forward with the masking restated in float64, computed ONCE: Z[:, 1:] += m (mask_token - Y), orc.block_forward in a loop, the
    final norm.  Returns the values and the gradients of the rest of the loss (CE + extra) and of the patch term <W, patch tokens> separately."""
    meta, _ = load_golden(name)
    cfg = meta["cfg"] if ortho else dict(meta["cfg"], ortho_loss_v1_lambda=0)
    meta = dict(meta, cfg=cfg)
    shapes = orc.state_shapes(cfg, meta["n_channels"], meta["img"], meta["num_classes"])
    sd = orc.make_state(shapes, meta["seed"], dtype=torch.float64)
    D, depth, heads = orc.MODEL_SIZES[cfg["pretrained_model_name"]]
    sd[MT] = _mask_token_value(D)
    for v in sd.values():
        v.requires_grad_(True)
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    x64 = x.double().requires_grad_()
    ch = meta["mapper"][meta["chunk"]]
    C = len(ch)
    Z, extra = orc.tokenise(sd, x64, cfg, ch, list(range(C)))
    Y = orc.patch_tokens(sd, x64[:, list(range(C))], cfg["patch_size"])
    n = Y.shape[1] // C
    m = _model_mask(meta["B"], C, n)
    Z = torch.cat([Z[:, :1], Z[:, 1:] + m[..., None].double() * (sd[MT] - Y)], dim=1)
    for i in range(depth):
        Z = orc.block_forward(sd, f"feature_extractor.blocks.{i}.", Z, heads, None)
    f = F.layer_norm(Z, (D,), sd["feature_extractor.norm.weight"], sd["feature_extractor.norm.bias"], EPS)
    logits = f[:, 0] @ sd["classifer_head.weight"].t() + sd["classifer_head.bias"]
    rest = F.cross_entropy(logits, y) + extra
    patches = f[:, 1:]
    W = torch.randn(*patches.shape, generator=torch.Generator().manual_seed(1234), dtype=torch.float64)
    tap = (W * patches).sum()
    names = list(sd)
    leaves = [sd[k] for k in names] + [x64]
    g_tap = torch.autograd.grad(tap, leaves, retain_graph=True, allow_unused=True)
    g_rest = torch.autograd.grad(rest, leaves, allow_unused=True)
    s = 2.0 * g_rest[names.index(QKV0)].norm().item() / g_tap[names.index(QKV0)].norm().item()
    grads = {}
    for k, gt, gr in zip(names + ["x"], g_tap, g_rest):
        parts = [p for p in ((None if gt is None else s * gt), gr) if p is not None]
        grads[k] = sum(parts) if parts else None
    return dict(meta=meta, x=x, y=y, W=W, s=s, mask=m, n=n, C=C, patches=patches.detach(), logits=logits.detach(), grads=grads)


class _Ref:
    def __init__(self, grad):
        self.grad = grad


def _masked_model(meta, dev, train=True):
    model, _ = build(meta, dev, train=train)
    mt = model.add_mask_token()
    with torch.no_grad():
        mt.copy_(_mask_token_value(model.dim).float())
    return model


def _masked_step(o, dev, masks="oracle"):
    model = _masked_model(o["meta"], dev)
    x, y = o["x"].to(dev).requires_grad_(), o["y"].to(dev)
    kw = {} if masks is None else dict(masks=(o["mask"] if masks == "oracle" else masks).to(dev))
    (out, extra), feats = model.forward_with_features(x, o["meta"]["chunk"], None, layers=1, pool=None, init_first_layer=None,
                                                      new_channel_init=None, cur_epoch=0, **kw)
    patches = feats[0][:, 1:]
    loss = F.cross_entropy(out, y) + extra + o["s"] * (o["W"].to(dev).float() * patches).sum()
    loss.backward()
    torch.cuda.synchronize()
    return model, x, out, extra, patches


def test_masked_train_step_against_the_oracle(gpu_device):
    o = _oracle()
    model, x, out, extra, patches = _masked_step(o, gpu_device)
    err = (out.detach().cpu().double() - o["logits"]).abs().max().item()
    assert err <= 3e-2 * o["logits"].abs().max().item()
    perr, pscale = (patches.detach().cpu().double() - o["patches"]).abs().max().item(), o["patches"].abs().max().item()
    print(f"masked step: logits {err:.3e}, patch tokens {perr / pscale:.3e} of max |ref|")
    assert patches.dtype == torch.float32 and perr <= 3e-2 * pscale
    mt = model.feature_extractor.mask_token
    assert mt.grad is not None and mt.grad.shape == (1, 1, model.dim) and mt.grad.abs().max().item() > 0
    worst = check_grads(model, {k: _Ref(g) for k, g in o["grads"].items()})  # mask_token, the patch projection, every block, channel_embed, pos_embed
    rel, cos = grad_agreement(x.grad.detach().cpu().double().numpy(), o["grads"]["x"].numpy())
    print(f"masked step: worst parameter gradient {worst}; x.grad per (image, channel) rel L2 max {rel.max():.3e}, cosine min {cos.min():.6f}")
    assert rel.max() <= 5e-2 and cos.min() >= 0.998


def test_input_gradient_is_zero_under_masked_patches_without_the_ortho_term(gpu_device):
    o = _oracle(ortho=False)
    model, x, out, extra, patches = _masked_step(o, gpu_device)
    B, C, n, P = o["meta"]["B"], o["C"], o["n"], o["meta"]["cfg"]["patch_size"]
    gh = o["meta"]["img"] // P
    gx = x.grad.view(B, C, gh, P, gh, P).permute(0, 1, 2, 4, 3, 5).reshape(B, C * n, P * P)
    m = o["mask"].to(gpu_device)
    assert not gx[m].any() and bool(gx[~m].any(-1).all())
    # per (image, channel), as above — but a channel masked whole (channel 0 of image 0) has no gradient at all, in the oracle either
    g, ref = x.grad.detach().cpu().double(), o["grads"]["x"].clone()
    whole = m.view(B, C, n).all(-1).cpu()
    assert bool(whole.any()) and not ref[whole].any() and not g[whole].any()
    g[whole], ref[whole] = 1.0, 1.0  # out of the comparison: equal placeholders
    rel, cos = grad_agreement(g.numpy(), ref.numpy())
    assert rel.max() <= 5e-2 and cos.min() >= 0.998
    check_grads(model, {k: _Ref(g) for k, g in o["grads"].items()})


# ---------------------------------------------------------------------------------------------------------------------------------------------
# invariants
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_an_all_false_mask_has_the_bits_of_no_mask(gpu_device):
    o = _oracle()
    runs = []
    for masks in (None, torch.zeros_like(o["mask"])):
        model, x, out, extra, patches = _masked_step(o, gpu_device, masks=masks)
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        runs.append(([out.detach(), extra.detach(), patches.detach(), x.grad], grads))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert MT not in runs[0][1] and not runs[1][1].pop(MT).any()  # without masks the token is not in the graph; with none set its gradient is 0
    assert runs[0][1].keys() == runs[1][1].keys() and not [k for k in runs[0][1] if not torch.equal(runs[0][1][k], runs[1][1][k])]


def _views(meta, dev):
    x, _ = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    xl, _ = orc.make_batch(meta["seed"] + 2, 2 * meta["B"], meta["C_in"], meta["img"] // 2, meta["num_classes"])
    return x.to(dev), xl.to(dev)


def test_forward_views_without_masks_is_what_it_was(gpu_device, monkeypatch):
    meta, _ = load_golden("tiny_e2e")
    model = _masked_model(meta, gpu_device, train=False)
    xg, xl = _views(meta, gpu_device)
    with torch.no_grad():
        want = [model.forward_with_features(x, meta["chunk"], None, layers=1, pool="cls")[1][0] for x in (xg, xl)]
        log = install_recorder(monkeypatch.setattr)
        res = model.forward_views([xg, xl], meta["chunk"])
        together = [n for n, _ in log]
        del log[:]
        model._refresh_own_copies(False)
        refresh = [n for n, _ in log]
        singles = []
        for x in (xg, xl):
            del log[:]
            model.forward_with_features(x, meta["chunk"], None, layers=1, pool="cls")
            singles.append([n for n, _ in log])
    assert isinstance(res, tuple) and len(res) == 2 and torch.equal(res[0], torch.cat(want)) and res[1].shape == () and not res[1].any()
    assert not [n for n in together if n.startswith(("mask_tokens", "ibot"))], "a new entry point in the plain call"
    # what it always launched: one refresh of the operand copies, then each view's forward as that view launches it alone, less its own refresh
    # (`load` is the library handle's lookup, not a launch: left out of the sequences)
    launches = lambda names: [n for n in names if n != "load"]  # noqa: E731
    together, refresh, singles = launches(together), launches(refresh), [launches(s) for s in singles]

    def without_refresh(s):
        at = next(i for i in range(len(s) - len(refresh) + 1) if s[i:i + len(refresh)] == refresh)
        return s[:at] + s[at + len(refresh):]

    assert refresh and len(singles[0]) > len(refresh)
    assert together == refresh + without_refresh(singles[0]) + without_refresh(singles[1])


def test_patch_views_are_get_intermediate_layers_bit_for_bit(gpu_device):
    meta, _ = load_golden("tiny_e2e")
    model = _masked_model(meta, gpu_device, train=False)
    xg, xl = _views(meta, gpu_device)
    with torch.no_grad():
        feats, extra, patches = model.forward_views([xg, xl], meta["chunk"], patch_views=(0,))
        want = model.feature_extractor.get_intermediate_layers(xg, n=1, chunk=meta["chunk"], pool=None)[0]
        both = model.forward_views([xg, xl], meta["chunk"], patch_views=(0, 1))[2]
    assert patches[1] is None and torch.equal(patches[0], want[:, 1:]) and torch.equal(feats[:xg.shape[0]], want[:, 0])
    assert patches[0].dtype == torch.float32 and feats.shape == (xg.shape[0] + xl.shape[0], model.dim)
    n_local = (meta["img"] // 2 // meta["cfg"]["patch_size"]) ** 2
    assert torch.equal(both[0], patches[0]) and both[1].shape == (xl.shape[0], meta["C_in"] * n_local, model.dim)


def test_student_step_with_a_masked_global_and_a_local_view(gpu_device):
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("tiny_e2e")
    model = _masked_model(meta, gpu_device)
    mt = model.feature_extractor.mask_token
    opt = dcv.HipAdamW(model.parameters(), lr=1e-2, weight_decay=0.0, model=model)
    xg, xl = _views(meta, gpu_device)
    C = meta["C_in"]
    g = meta["img"] // meta["cfg"]["patch_size"]
    gen = dcv.BlockMaskGenerator((g, g), channels=C, mask_prob=1.0, seed=4)
    m = gen(xg.shape[0])
    K = 96
    head = dcv.DINOHead(model.dim, out_dim=K, hidden_dim=64, bottleneck_dim=32).to(gpu_device)
    crit = dcv.IBOTPatchLoss(K).to(gpu_device)
    feats, extra, patches = model.forward_views([xg, xl], meta["chunk"], masks=[m.mask_dev, None], patch_views=(0,), cur_epoch=0)
    assert patches[1] is None and patches[0].shape == (xg.shape[0], C * g * g, model.dim)
    s_plog = head(patches[0].flatten(0, 1).index_select(0, m.rows))
    t_plog = torch.randn(m.rows.numel(), K, device=gpu_device, generator=torch.Generator(device=gpu_device).manual_seed(0))
    loss = crit(s_plog, t_plog, m.weights, 0.04) + head(feats).square().mean() + extra
    before = mt.detach().clone()
    loss.backward()
    assert torch.isfinite(loss) and mt.grad is not None and mt.grad.abs().max().item() > 0
    opt.step()
    crit.update_center()
    torch.cuda.synchronize()
    assert not torch.equal(mt.detach(), before) and torch.isfinite(mt).all() and bool(crit.center.any())
    assert MT in model.state_dict()


def test_only_the_mask_token_trainable_still_runs_the_tokeniser_backward(gpu_device):
    meta, _ = load_golden("tiny_e2e")
    model = _masked_model(meta, gpu_device)
    for p in model.parameters():
        p.requires_grad_(False)
    mt = model.feature_extractor.mask_token.requires_grad_(True)
    xg, _ = _views(meta, gpu_device)
    n = (meta["img"] // meta["cfg"]["patch_size"]) ** 2
    masks = _model_mask(xg.shape[0], meta["C_in"], n).to(gpu_device)
    out, extra = model(xg, meta["chunk"], None, masks=masks, cur_epoch=0)
    out.square().sum().backward()
    assert mt.grad is not None and mt.grad.abs().max().item() > 0
    assert all(p.grad is None for k, p in model.named_parameters() if k != MT)


def test_raises(gpu_device):
    import random
    meta, _ = load_golden("so2sat_s")
    x, _ = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    x = x.to(gpu_device)
    n = (meta["img"] // meta["cfg"]["patch_size"]) ** 2
    good = torch.zeros(meta["B"], meta["C_in"] * n, dtype=torch.uint8, device=gpu_device)
    plain, _ = build(meta, gpu_device)
    keys = set(plain.state_dict())
    with pytest.raises(ValueError, match="add_mask_token"):
        plain(x, "train", None, masks=good)
    model, _ = build(meta, gpu_device)
    model.add_mask_token()
    assert set(model.state_dict()) == keys | {MT} and not model.state_dict()[MT].any()
    for bad in (good[:, :-1], good[:-1], good.float(), good.cpu(), good.view(-1)):
        with pytest.raises(ValueError, match="masks: expected"):
            model(x, "train", None, masks=bad)
    with pytest.raises(ValueError, match="one entry per view"):
        model.forward_views([x], "train", masks=[good, None])
    with pytest.raises(ValueError, match="patch_views"):
        model.forward_views([x], "train", patch_views=(1,))
    # token drop active in train mode
    model_d, _ = build(dict(meta, cfg=dict(meta["cfg"], dropout_tokens_hcs="random")), gpu_device)
    model_d.add_mask_token()
    random.seed(5)
    with pytest.raises(ValueError, match="dropout_tokens_hcs"):
        model_d(x, "train", None, masks=good)
    # HCS channel sampling active in this forward (train mode, enable_sample): refused before the draw; in eval mode the same model takes masks
    model_h, _ = build(meta, gpu_device)
    model_h.add_mask_token()
    model_h.feature_extractor.patch_embed.enable_sample = True
    state = random.getstate()
    with pytest.raises(ValueError, match="HCS"):
        model_h(x, "train", None, masks=good)
    assert random.getstate() == state
    model_h.eval()
    with torch.no_grad():
        assert torch.isfinite(model_h(x, "train", None, masks=good)).all()

    class _Reducer:  # stands in for dp.DataParallel: the check comes before anything of the reducer is called
        pass
    model._dp = _Reducer()
    with pytest.raises(NotImplementedError, match="DataParallel"):
        model(x, "train", None, masks=good)
    model._dp = None
