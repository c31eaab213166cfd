"""DiChaViT.forward_with_features on the MI355X: the channel-pool adjoint kernel (dcv_ln_pool_channels_bwd) against float64 autograd on the
CPU, and the model method — values, every parameter gradient, x.grad — against the fp64 oracle with the taps restated in float64.

Bounds.  Kernel: test_layernorm's standing ones (dx rtol 1e-4 / atol 1e-4; dgamma, dbeta rtol 1e-4 / atol 1e-3), with dout = unit normal times n_p
so that a row's d x^ is of order 1 as du is there.  Model: check_grads' rel L2 <= 5e-2 and cos >= 0.998 for every parameter gradient, 3e-2 of
max |ref| for the taps (test_model_tokens_against_the_reference), test_input_grad_gpu's per (image, channel) bounds for x.grad.  The loss is
CE + extra + s sum_k <W_k, feats_k> with fixed random W_k; s is chosen on the ORACLE's numbers so that the taps' term alone gives
blocks.0.attn.qkv.weight at least the gradient norm of the rest — asserted — so a missing tap term cannot hide under the bound."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle import dichavit_oracle as orc
from test_input_grad_cpu import grad_agreement
from test_kernels_gpu import _close, _f
from test_model_gpu import build, check_grads

pytestmark = pytest.mark.gpu

EPS = 1e-6
LAYERS = (3, 7, 11)  # two inner blocks and the last one (depth 12 in both fixtures)
QKV0 = "feature_extractor.blocks.0.attn.qkv.weight"


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _inputs(B, C, n_p, D):
    """x and gamma as test_layernorm draws them; dout unit normal times n_p; non-zero starts for everything accumulated into."""
    N = 1 + C * n_p
    x = (_f(B * N, D, scale=2.0, seed=1) + 0.5).view(B, N, D)
    gamma = 1 + 0.1 * _f(D, seed=2)
    dout = _f(B, 1 + C, D, scale=float(n_p), seed=4)
    dx_in = _f(B, N, D, seed=5)
    dg_in, db_in = _f(D, seed=6), _f(D, seed=7)
    return x, gamma, dout, dx_in, dg_in, db_in


def _ref64(B, C, n_p, D):
    """float64 torch autograd on the CPU through layer_norm followed by the segment mean -> (dx, dgamma, dbeta) for _inputs' tensors"""
    x, gamma, dout, *_ = _inputs(B, C, n_p, D)
    x64, g64 = x.cpu().double().requires_grad_(), gamma.cpu().double().requires_grad_()
    b64 = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    ln = F.layer_norm(x64, (D,), g64, b64, EPS)
    pooled = torch.cat([ln[:, :1], ln[:, 1:].view(B, C, n_p, D).mean(2)], dim=1)
    pooled.backward(dout.cpu().double())
    return x64.grad, g64.grad, b64.grad


def _run(hip, x, gamma, dout, dx_in, dg_in, db_in, B, C, n_p, D, null=False, ws=None):
    dx = dx_in.clone()
    dg, db = (None, None) if null else (dg_in.clone(), db_in.clone())
    hip.ln_pool_channels_bwd(x, gamma, dout, dx, dg, db, B, C, n_p, D, EPS, **({} if ws is None else dict(ws=ws)))
    return dx, dg, db


SPLIT, SPLIT_WIDE, WHOLE = (2, 3, 196, 384), (3, 5, 16, 768), (2, 4, 7, 192)
SHAPES = [SPLIT, SPLIT_WIDE, WHOLE,   # the shapes of test_pool_kernel_determinism_and_seams: split, split-wide and whole segments
          (2, 3, 1, 384),             # a segment of one row: three idle waves
          (5, 2, 3, 132),             # fewer rows than waves; D no multiple of 64 floats; five images: a partial CLS workgroup
          (2, 3, 7, 4),               # an odd remainder of rows; one float4 per row
          (1, 3, 197, 384),           # 21 splits of 9 rows and a last one of 8
          (2, 1, 36, 192),            # one channel
          (1, 2, 20, 1024),           # one image; the widest row (4 float4 per lane, every lane live)
          (1, 1, 1, 768),
          (64, 8, 196, 384),          # the headline shape: 4 splits of 49 rows, 16 full CLS workgroups, 2064 dgamma partials (measured: dx 6.2e-5,
                                      # dgamma 1.1e-3 at max |ref| 5.0e3, dbeta 3.9e-3 at max |ref| 1.4e4)
          (2, 18, 16, 384),           # So2Sat-like: 2 splits of 8 rows
          (2, 8, 15, 384)]            # one workgroup per segment, a partial last round of rows


@pytest.mark.parametrize("B,C,n_p,D", SHAPES)
def test_kernel_against_float64(hip, B, C, n_p, D):
    t = _inputs(B, C, n_p, D)
    x, gamma, dout, dx_in, dg_in, db_in = t
    dx, dg, db = _run(hip, *t, B, C, n_p, D)
    rx, rg, rb = _ref64(B, C, n_p, D)
    want_dx = dx_in.cpu().double() + rx
    print(f"B{B} C{C} n_p{n_p} D{D}: dx max err {(dx.cpu().double() - want_dx).abs().max().item():.3e}, "
          f"dgamma {(dg.cpu().double() - dg_in.cpu().double() - rg).abs().max().item():.3e} (max |ref| {rg.abs().max().item():.3e}), "
          f"dbeta {(db.cpu().double() - db_in.cpu().double() - rb).abs().max().item():.3e} (max |ref| {rb.abs().max().item():.3e})")
    # accumulation onto the non-zero starts, not overwrite
    _close(dx.cpu(), want_dx, 1e-4, 1e-4, "dx")
    _close(dg.cpu(), dg_in.cpu().double() + rg, 1e-4, 1e-3, "dgamma")
    _close(db.cpu(), db_in.cpu().double() + rb, 1e-4, 1e-3, "dbeta")
    assert not torch.equal(dx, dx_in) and (dx - dx_in).abs().max().item() > 1e-2  # the term itself is not below the bound
    # NULL dgamma / dbeta: accepted, the same dx bit for bit
    dx_null, _, _ = _run(hip, *t, B, C, n_p, D, null=True)
    assert torch.equal(dx_null, dx)


@pytest.mark.parametrize("B,C,n_p,D", [SPLIT, WHOLE], ids=["split", "whole"])
def test_kernel_is_deterministic_and_touches_its_rows_only(hip, B, C, n_p, D):
    t = _inputs(B, C, n_p, D)
    x, gamma, dout, dx_in, dg_in, db_in = t
    first = _run(hip, *t, B, C, n_p, D)
    again = _run(hip, *t, B, C, n_p, D)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    # dout = 0 for every image but one: the rows of the others keep their bits
    for b in (0, B - 1):
        d1 = torch.zeros_like(dout)
        d1[b] = dout[b]
        dx, dg, db = _run(hip, x, gamma, d1, dx_in, dg_in, db_in, B, C, n_p, D)
        others = [i for i in range(B) if i != b]
        assert torch.equal(dx[others], dx_in[others]) and torch.equal(dx[b], first[0][b])
    # ... and for every (image, row of dout) but one: exactly that segment's rows change
    N = 1 + C * n_p
    for b, j in ((0, 0), (B - 1, 1), (B - 1, C)):
        d1 = torch.zeros_like(dout)
        d1[b, j] = dout[b, j]
        dx, _, _ = _run(hip, x, gamma, d1, dx_in, dg_in, db_in, B, C, n_p, D)
        rows = torch.zeros(B, N, dtype=torch.bool, device="cuda")
        rows[b, 0 if j == 0 else slice(1 + (j - 1) * n_p, 1 + j * n_p)] = True
        assert torch.equal(dx[~rows], dx_in[~rows]) and torch.equal(dx[rows], first[0][rows])
    # exactly [B, N, D] of dx is written: guard regions before and after keep their NaNs
    G, n = 4096, B * N * D
    buf = torch.full((G + n + G,), float("nan"), device="cuda")
    inner = buf[G:G + n].view(B, N, D)
    inner.copy_(dx_in)
    hip.ln_pool_channels_bwd(x, gamma, dout, inner, dg_in.clone(), db_in.clone(), B, C, n_p, D, EPS)
    torch.cuda.synchronize()
    assert torch.equal(inner, first[0]) and torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n:]).all()


def test_kernel_refusals(hip):
    """Real tensors behind every pointer, large enough for any of the shapes named: a refused call must not have launched anything."""
    B, C, n_p = 2, 3, 16
    N = 1 + C * n_p
    x = torch.randn(B * N * 1028 + 4, device="cuda")
    gamma = torch.ones(1028, device="cuda")
    dout = torch.randn(B * (1 + C) * 1028, device="cuda")
    dx = torch.full((B * N * 1028 + 4,), float("nan"), device="cuda")
    dg, db = torch.full((1028,), float("nan"), device="cuda"), torch.full((1028,), float("nan"), device="cuda")
    for D in (6, 1028):
        with pytest.raises(RuntimeError, match="dcv_ln_pool_channels_bwd|workspace"):
            hip.ln_pool_channels_bwd(x, gamma, dout, dx, dg, db, B, C, n_p, D, EPS)
    need = hip.load().dcv_ln_pool_channels_bwd_ws_floats(B, C, n_p, 384)
    assert need == (B * C * 2 + 1) * 384
    with pytest.raises(RuntimeError, match="dcv_ln_pool_channels_bwd"):  # a short workspace
        hip.ln_pool_channels_bwd(x, gamma, dout, dx, dg, db, B, C, n_p, 384, EPS, ws=torch.empty(need - 4, device="cuda"))
    for bad in ("x", "dx"):  # a pointer that is not 16-byte aligned
        with pytest.raises(RuntimeError, match="dcv_ln_pool_channels_bwd"):
            hip.ln_pool_channels_bwd(x[1:] if bad == "x" else x, gamma, dout, dx[1:] if bad == "dx" else dx, dg, db, B, C, n_p, 384, EPS)
    torch.cuda.synchronize()
    assert torch.isnan(dx).all() and torch.isnan(dg).all() and torch.isnan(db).all()
    dx.zero_(); dg.zero_(); db.zero_()
    hip.ln_pool_channels_bwd(x, gamma, dout, dx, dg, db, B, C, n_p, 384, EPS, ws=torch.empty(need, device="cuda"))  # the exact size is enough
    assert torch.isfinite(dx[:B * N * 384]).all() and torch.isfinite(dg[:384]).all() and dg[:384].abs().max().item() > 0


def test_kernel_agrees_with_the_composite_it_replaces(hip):
    """dcv_ln_fwd for the statistics, then dcv_ln_bwd (f32 du) on the materialised broadcast of dout / n_p, accumulating into dx."""
    B, C, n_p, D = SPLIT
    N, M = 1 + C * n_p, B * (1 + C * n_p)
    t = _inputs(B, C, n_p, D)
    x, gamma, dout, dx_in, dg_in, db_in = t
    dx, dg, db = _run(hip, *t, B, C, n_p, D)
    du = torch.cat([dout[:, :1], (dout[:, 1:] / n_p).repeat_interleave(n_p, dim=1)], dim=1).contiguous()
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    scratch = torch.empty(M, D, device="cuda")
    hip.ln_fwd(x, gamma, torch.zeros(D, device="cuda"), scratch, mean, rstd, M, D, EPS)
    dx2, dg2, db2 = dx_in.clone(), dg_in.clone(), db_in.clone()
    hip.ln_bwd(du.view(M, D), x, mean, rstd, gamma, dx2.view(M, D), dx2.view(M, D), None, dg2, db2, M, D)
    _close(dx, dx2, 1e-4, 1e-4, "dx against the composite")
    _close(dg, dg2, 1e-4, 1e-3, "dgamma against the composite")
    _close(db, db2, 1e-4, 1e-3, "dbeta against the composite")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the model against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _pool64(f, pool, C):
    if pool is None:
        return f
    if pool == "cls":
        return f[:, 0]
    B, N, D = f.shape
    return torch.cat([f[:, :1], f[:, 1:].view(B, C, (N - 1) // C, D).mean(2)], dim=1)


def _tap_weights(shapes):
    g = torch.Generator(device="cpu").manual_seed(1234)
    return [torch.randn(*s, generator=g, dtype=torch.float64) for s in shapes]


@functools.lru_cache(maxsize=None)
def _oracle(name, pool, layers=LAYERS, masks_key=None):
    """The oracle's forward with the taps restated in float64 — orc.block_forward in a loop, layer_norm(eps=1e-6) with the final norm, the
    pooling — computed ONCE per case and shared.  Returns the values and, for the parameters and x, the gradient of the rest of the loss
    (CE + extra) and of the taps' term sum_k <W_k, feats_k> separately: the loss is linear in the second, so any weight s of it is their sum."""
    meta, a = load_golden(name)
    cfg = meta["cfg"]
    shapes = orc.state_shapes(cfg, meta["n_channels"], meta["img"], meta["num_classes"])
    sd = orc.make_state(shapes, meta["seed"], dtype=torch.float64)
    for v in sd.values():
        v.requires_grad_(True)
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    x64 = x.double().requires_grad_()
    ch = meta["mapper"][meta["chunk"]]
    C = len(ch)
    D, depth, heads = orc.MODEL_SIZES[cfg["pretrained_model_name"]]
    z, extra = orc.tokenise(sd, x64, cfg, ch, list(range(C)))
    dpr = orc.drop_path_rates(cfg)
    masks = None
    if masks_key is not None:
        order = [(bi, br) for bi, r in enumerate(dpr) if r > 0 for br in ("attn", "mlp")]
        masks = {k: torch.from_numpy(a["keep"][i]) for i, k in enumerate(order)}
    feats = []
    for i in range(depth):
        drop = (masks[(i, "attn")], masks[(i, "mlp")], 1.0 - dpr[i]) if masks is not None and dpr[i] > 0 else None
        z = orc.block_forward(sd, f"feature_extractor.blocks.{i}.", z, heads, drop)
        if i in layers:
            f = F.layer_norm(z, (D,), sd["feature_extractor.norm.weight"], sd["feature_extractor.norm.bias"], EPS)
            feats.append(_pool64(f, pool, C))
    f = F.layer_norm(z, (D,), sd["feature_extractor.norm.weight"], sd["feature_extractor.norm.bias"], EPS)[:, 0]
    logits = f @ sd["classifer_head.weight"].t() + sd["classifer_head.bias"]
    rest = F.cross_entropy(logits, y) + extra
    W = _tap_weights([tuple(t.shape) for t in feats])
    tap = sum((w * t).sum() for w, t in zip(W, feats))
    names = list(sd)
    leaves = [sd[k] for k in names] + [x64]
    g_tap = torch.autograd.grad(tap, leaves, retain_graph=True, allow_unused=True)
    g_rest = torch.autograd.grad(rest, leaves, allow_unused=True)
    s = 2.0 * g_rest[names.index(QKV0)].norm().item() / g_tap[names.index(QKV0)].norm().item()
    return dict(meta=meta, x=x, y=y, W=W, s=s, feats=[t.detach() for t in feats], logits=logits.detach(), masks=masks,
                g_tap=dict(zip(names + ["x"], g_tap)), g_rest=dict(zip(names + ["x"], g_rest)))


class _Ref:
    """what check_grads reads: sd_ref[name].grad"""

    def __init__(self, grad):
        self.grad = grad


def _sd_ref(o, s_tap, with_rest=True):
    out = {}
    for k, gt in o["g_tap"].items():
        gr = o["g_rest"][k] if with_rest else None
        parts = [p for p in ((None if gt is None else s_tap * gt), gr) if p is not None]
        out[k] = _Ref(sum(parts) if parts else None)
    return out


def _tap_loss(o, feats, dev):
    return o["s"] * sum((w.to(dev).float() * t).sum() for w, t in zip(o["W"], feats))


def _assert_taps_dominate(o):
    """On the oracle's numbers: the taps' term alone gives blocks.0.attn.qkv.weight at least the gradient norm of CE + extra alone."""
    gt, gr = o["s"] * o["g_tap"][QKV0].norm().item(), o["g_rest"][QKV0].norm().item()
    assert gt >= gr > 0, (gt, gr)


def _step(model, o, dev, pool, layers=LAYERS, with_rest=True, **fw):
    x, y = o["x"].to(dev), o["y"].to(dev)
    (out, extra), feats = model.forward_with_features(x, o["meta"]["chunk"], None, layers=list(layers), pool=pool, init_first_layer=None,
                                                      new_channel_init=None, cur_epoch=0, **fw)
    loss = _tap_loss(o, feats, dev)
    if with_rest:
        loss = loss + F.cross_entropy(out, y) + extra
    loss.backward()
    return out, extra, feats


def _check_feats(o, feats):
    for k, (t, ref) in enumerate(zip(feats, o["feats"])):
        assert t.dtype == torch.float32 and t.shape == ref.shape
        err, scale = (t.detach().cpu().double() - ref).abs().max().item(), ref.abs().max().item()
        print(f"tap {k}: {err / scale:.3e} of max |ref|")
        assert err <= 3e-2 * scale, (k, err, scale)


@pytest.mark.parametrize("pool", ["channel", "cls", None])
@pytest.mark.parametrize("name", ["tiny_e2e", "so2sat_s"])
def test_train_step_with_taps_against_the_oracle(gpu_device, name, pool):
    o = _oracle(name, pool)
    _assert_taps_dominate(o)
    model, _ = build(o["meta"], gpu_device)
    out, extra, feats = _step(model, o, gpu_device, pool)
    assert all(t.requires_grad for t in feats)
    _check_feats(o, feats)
    assert (out.detach().cpu().double() - o["logits"]).abs().max().item() <= 3e-2 * o["logits"].abs().max().item()
    worst = check_grads(model, _sd_ref(o, o["s"]))
    print(f"{name} pool={pool}: worst grad rel err {worst}, tap weight s = {o['s']:.3e}")


def test_cls_tap_at_the_last_block_without_the_cls_only_tail(gpu_device):
    """cls_only_tail off: the last block's stream is full-size, so the tap's dcv_ln_bwd walks the B CLS rows of x_final and of dx with the row
    stride N D (with the tail on, the default covered above, both are compact [B, D])."""
    o = _oracle("tiny_e2e", "cls")
    model, _ = build(o["meta"], gpu_device)
    model.cls_only_tail = False
    out, extra, feats = _step(model, o, gpu_device, "cls")
    _check_feats(o, feats)
    check_grads(model, _sd_ref(o, o["s"]))


def test_loss_on_the_taps_alone(gpu_device):
    o = _oracle("so2sat_s", "channel")
    model, _ = build(o["meta"], gpu_device)
    out, extra, feats = _step(model, o, gpu_device, "channel", with_rest=False)
    ref = _sd_ref(o, o["s"], with_rest=False)
    assert ref["classifer_head.weight"].grad is None and model.classifer_head.weight.grad is None  # `out` received no gradient
    assert model.feature_extractor.blocks[0].attn.qkv.weight.grad.norm().item() > 0
    assert model.feature_extractor.blocks[11].mlp.fc2.weight.grad.norm().item() > 0  # the last block is tapped: it has a gradient too
    check_grads(model, ref)


def test_eval_taps_are_get_intermediate_layers_bit_for_bit(gpu_device):
    meta, _ = load_golden("so2sat_s")
    model, _ = build(meta, gpu_device, train=False)
    fe = model.feature_extractor
    x, _ = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    x = x.to(gpu_device)
    with torch.no_grad():
        plain = model(x, "train", None)
        for layers in ([3, 7, 11], [2, 5], 4):
            for pool in ("channel", None):
                out, feats = model.forward_with_features(x, "train", None, layers=layers, pool=pool)
                want = fe.get_intermediate_layers(x, n=layers, chunk="train", pool=pool)
                assert len(feats) == len(want) and all(torch.equal(a, b) for a, b in zip(feats, want)), (layers, pool)
                assert not any(t.requires_grad for t in feats)
                if layers == [2, 5]:
                    assert torch.equal(out, plain)  # inner taps only: the forward is the plain one
        # pool="cls" is row 0 of the tokens; with the last block tapped the CLS-only tail stays and `out` keeps its bits
        toks = fe.get_intermediate_layers(x, n=[2, 5], chunk="train")
        out, feats = model.forward_with_features(x, "train", None, layers=[2, 5], pool="cls")
        assert torch.equal(out, plain) and all(torch.equal(a, b[:, 0]) for a, b in zip(feats, toks))
        out, feats = model.forward_with_features(x, "train", None, layers=[5, 11], pool="cls")
        assert torch.equal(out, plain) and feats[1].shape == (meta["B"], model.dim)


@pytest.mark.parametrize("layers,pool", [([3, 7], "channel"), ([3, 7], None), ([7, 11], "cls")])
def test_out_is_the_plain_forwards_bit_for_bit_in_training(gpu_device, layers, pool):
    """Inner taps only, or the last block tapped with pool="cls": the CLS-only tail is in the same state, so the logits, the extra loss and,
    with the taps left out of the loss, every gradient have the plain step's bits."""
    meta, _ = load_golden("so2sat_s")
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    x, y = x.to(gpu_device), y.to(gpu_device)
    runs = []
    for tapped in (False, True):
        model, _ = build(meta, gpu_device)
        if tapped:
            (out, extra), feats = model.forward_with_features(x, "train", None, layers=layers, pool=pool, cur_epoch=0)
        else:
            out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        (F.cross_entropy(out, y) + extra).backward()  # the taps receive no gradient: nothing of theirs runs in the backward
        runs.append((out.detach().clone(), extra.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][2].keys() == runs[1][2].keys() and not [n for n in runs[0][2] if not torch.equal(runs[0][2][n], runs[1][2][n])]


def test_data_only_input_gradient_from_the_taps(gpu_device):
    o = _oracle("so2sat_s", "channel")
    model, _ = build(o["meta"], gpu_device)
    for p in model.parameters():
        p.requires_grad_(False)
    x = o["x"].to(gpu_device).requires_grad_()
    (out, extra), feats = model.forward_with_features(x, "train", None, layers=list(LAYERS), pool="channel", cur_epoch=0)
    _tap_loss(o, feats, gpu_device).backward()
    assert all(p.grad is None for p in model.parameters())
    ref = (o["s"] * o["g_tap"]["x"]).numpy()
    rel, cos = grad_agreement(x.grad.detach().cpu().double().numpy(), ref)
    print(f"x.grad from a taps-only loss: per (image, channel) rel L2 max {rel.max():.3e}, cosine min {cos.min():.6f}")
    assert rel.max() <= 5e-2 and cos.min() >= 0.998


def test_frozen_prefix_with_taps_at_the_boundary_and_above(gpu_device):
    k, layers = 3, (2, 7, 11)  # the tap at block k - 1 = 2: its gradient reaches only `norm`
    o = _oracle("so2sat_s", "channel", layers)
    model, _ = build(o["meta"], gpu_device)
    model.freeze_prefix(k)
    _step(model, o, gpu_device, "channel", layers)
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert len(frozen) > 12 * k and all(p.grad is None for n, p in model.named_parameters() if not p.requires_grad)
    ref = _sd_ref(o, o["s"])
    for n in frozen:
        ref[n] = _Ref(None)
    check_grads(model, ref)
    # ... and the tap at k - 1 did reach norm: without it norm.weight's gradient is off by more than the bound
    gw = model.feature_extractor.norm.weight.grad.cpu().double()
    without = ref["feature_extractor.norm.weight"].grad - o["s"] * _tap_only_norm_grad(o, 0)
    assert (gw - without).norm().item() > 5e-2 * without.norm().item()
    with pytest.raises(ValueError, match="frozen prefix"):
        model.forward_with_features(o["x"].to(gpu_device), "train", None, layers=[k - 2], pool="channel")


def _tap_only_norm_grad(o, k):
    """d <W_k, feats_k> / d norm.weight in float64: feats_k = pool(x^) * gamma + beta, so the gradient is sum (W_k * pool(x^)) over all but D"""
    meta = o["meta"]
    shapes = orc.state_shapes(meta["cfg"], meta["n_channels"], meta["img"], meta["num_classes"])
    sd = orc.make_state(shapes, meta["seed"], dtype=torch.float64)
    g, b = sd["feature_extractor.norm.weight"], sd["feature_extractor.norm.bias"]
    xh = (o["feats"][k] - b) / g
    return (o["W"][k] * xh).flatten(0, -2).sum(0)


def test_drop_path_with_inner_taps(gpu_device):
    """DropPath on (the drop_path fixture, the reference's own masks): the bf16 copy written by the norm1 backward above a tap carries the
    block's DropPath factor AND the tap's term; the copy that feeds the tapped stream's own attention branch must not carry it."""
    layers = (2, 6, 9)
    o = _oracle("drop_path", "channel", layers, "golden")
    _assert_taps_dominate(o)
    model, _ = build(o["meta"], gpu_device)
    model.stochastic_weight_rounding = False
    model.drop_path_sampler = lambda bi, branch, B, dev: o["masks"][(bi, branch)]
    out, extra, feats = _step(model, o, gpu_device, "channel", layers)
    _check_feats(o, feats)
    check_grads(model, _sd_ref(o, o["s"]))


def test_two_tapped_steps_are_bit_identical(gpu_device):
    import diverse_channel_vit_amd as dcv
    assert dcv.is_deterministic()
    o = _oracle("so2sat_s", "channel")
    runs = []
    for rep in range(2):
        model, _ = build(o["meta"], gpu_device)
        out, extra, feats = _step(model, o, gpu_device, "channel")
        torch.cuda.synchronize()
        runs.append(([out.detach().clone()] + [t.detach().clone() for t in feats],
                     {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert runs[0][1].keys() == runs[1][1].keys() and not [n for n in runs[0][1] if not torch.equal(runs[0][1][n], runs[1][1][n])]


@contextlib.contextmanager
def _single_rank_group(gpu_device, port):
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("a process group already exists")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu_device)
    try:
        yield
    finally:
        dist.destroy_process_group()


def test_data_parallel_hands_norm_over_after_the_lowest_tap(gpu_device):
    import diverse_channel_vit_amd as dcv
    with _single_rank_group(gpu_device, "29617"):
        o = _oracle("so2sat_s", "channel")
        grads, handed = {}, []
        for mode in ("plain", "dp"):
            model, _ = build(o["meta"], gpu_device)
            if mode == "dp":
                model._ensure_arena(gpu_device)
                dp = dcv.DataParallel(model, min_bucket_bytes=1 << 20, force_collectives=True)
                dp.broadcast_parameters(0)
                dp.hook_misc_params()
                ready = dp.grad_ready
                dp.grad_ready = lambda arena, lo, hi: (handed.append((lo, hi)), ready(arena, lo, hi))[1]
            _step(model, o, gpu_device, "channel")
            if mode == "dp":
                assert dp.buckets_launched >= 8
                dp.finalize()
            torch.cuda.synchronize()
            grads[mode] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        # the final norm's slice is handed over after block LAYERS[0] + 1's backward — the lowest tap's term is in — and before that block's own
        fe = model.feature_extractor
        norm_range = model._range_of([fe.norm.weight, fe.norm.bias])
        block_range = lambda i: model._range_of([fe.blocks[i].norm1.weight, fe.blocks[i].mlp.fc2.bias])  # noqa: E731
        assert handed[:11 - LAYERS[0] + 1] == [block_range(i) for i in range(11, LAYERS[0] + 1, -1)] + [norm_range, block_range(LAYERS[0] + 1)]
        # norm's gradients depend on the forward and the taps' gradients alone: the same bits as without the reducer
        for k in ("feature_extractor.norm.weight", "feature_extractor.norm.bias"):
            assert torch.equal(grads["dp"][k], grads["plain"][k]), k
        for k, g in grads["plain"].items():  # the rest as test_dp_reducer_on_rccl_single_gpu holds it (the backward's GEMMs leave CUs to RCCL)
            assert (grads["dp"][k] - g).abs().max().item() <= 1e-3 * g.abs().max().item() + 1e-9, k


def test_data_parallel_issues_every_collective_of_the_block_loop_from_the_side_stream(gpu_device):
    """Two streams and a bucket larger than a block (tiny width: 1.8 MB per block): when the final norm's range is handed over inside the block
    loop, the slices of the blocks above are still pending and grad_ready launches them, so that hand-over has to come from the side stream
    like a block's own — their writers are side-stream GEMMs the main stream never waits for.  Only what follows the join of the streams (the
    tokeniser's hand-over and the flush, whose slice starts at the arena's offset 0) is issued from the main stream."""
    import diverse_channel_vit_amd as dcv
    with _single_rank_group(gpu_device, "29619"):
        o = _oracle("tiny_e2e", "channel")
        model, _ = build(o["meta"], gpu_device)
        model.wgrad_stream = True
        model._ensure_arena(gpu_device)
        dp = dcv.DataParallel(model, min_bucket_bytes=64 << 20, force_collectives=True)
        dp.broadcast_parameters(0)
        dp.hook_misc_params()
        issued, reduce = [], dp._reduce
        dp._reduce = lambda t: (issued.append((torch.cuda.current_stream().cuda_stream, t.data_ptr(), t.numel())), reduce(t))[1]
        main = torch.cuda.current_stream().cuda_stream
        _step(model, o, gpu_device, "channel")
        dp.finalize()
        torch.cuda.synchronize()
        side = model._side.cuda_stream
        assert side != main
        fe = model.feature_extractor
        block_range = lambda i: model._range_of([fe.blocks[i].norm1.weight, fe.blocks[i].mlp.fc2.bias])  # noqa: E731
        norm_range = model._range_of([fe.norm.weight, fe.norm.bias])
        base = model._grad_arena.data_ptr()  # slices of the encoder's gradient arena as (stream, lo, hi) in floats; the hooks' tensors lie elsewhere
        arena = [(st, (ptr - base) // 4, (ptr - base) // 4 + n) for st, ptr, n in issued if 0 <= ptr - base < 4 * model._enc_size]
        # the norm's hand-over after block LAYERS[0] + 1 launched the merged slices of blocks 11 .. LAYERS[0] + 2, then the norm went out alone
        assert (side, block_range(LAYERS[0] + 2)[0], block_range(11)[1]) in arena, arena
        assert (side, *norm_range) in arena, arena
        # what the main stream issues (after the join of the streams: the rest of the merge and the tokeniser's range) holds none of those
        from_main = [(lo, hi) for st, lo, hi in arena if st != side]
        assert from_main and all(hi <= block_range(LAYERS[0] + 1)[1] for lo, hi in from_main), arena
        check_grads(model, _sd_ref(o, o["s"]))


def test_tapped_forward_leaves_the_next_plain_step_alone(gpu_device):
    """A forward with taps (eval mode, no_grad: it draws nothing and rounds to nearest) before a plain training step: that step's outputs and
    gradients have the bits of the same step without the preceding call."""
    meta, _ = load_golden("so2sat_s")
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    x, y = x.to(gpu_device), y.to(gpu_device)
    runs = []
    for before in (False, True):
        model, _ = build(meta, gpu_device)
        if before:
            model.eval()
            with torch.no_grad():
                model.forward_with_features(x, "train", None, layers=4, pool="channel")
            model.train()
        out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        (F.cross_entropy(out, y) + extra).backward()
        runs.append((out.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert runs[0][1].keys() == runs[1][1].keys() and not [n for n in runs[0][1] if not torch.equal(runs[0][1][n], runs[1][1][n])]


def test_token_drop_refuses_the_channel_pool(gpu_device):
    import random
    meta, _ = load_golden("so2sat_s")
    model, _ = build(dict(meta, cfg=dict(meta["cfg"], dropout_tokens_hcs="random")), gpu_device)
    x, _ = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    random.seed(5)
    with pytest.raises(ValueError, match="ragged"):
        model.forward_with_features(x.to(gpu_device), "train", None, layers=2, pool="channel")
    random.seed(5)
    (out, extra), feats = model.forward_with_features(x.to(gpu_device), "train", None, layers=2, pool=None)
    assert feats[0].shape[0] == meta["B"] and feats[0].shape[2] == model.dim and feats[0].shape[1] <= 1 + 18 * 16
    (F.cross_entropy(out, torch.zeros(meta["B"], dtype=torch.long, device=gpu_device)) + extra + feats[0].sum() + feats[1].sum()).backward()
    assert torch.isfinite(model.feature_extractor.blocks[0].attn.qkv.weight.grad).all()
