"""get_intermediate_layers on the MI355X: the LayerNorm channel-pool kernel (dcv_ln_pool_channels) against float64 of the same formulas, its
determinism and segment seams, its refusals, and the model method against the real reference's tokens (tests/golden/intermediate_layers.npz,
written by make_golden_intermediate.py) and against the library's own forward.

Bounds.  Kernel, per output element: 1e-5 + 1e-5 a + n_p 2^-24 a, where a is, for that column, the segment's mean over its rows of
|gamma| |x^| + |beta| in float64 (x^ the normalised row; a dominates |LN output| whether the affine is applied per row or once to the mean):
the project's standing bound for the fp32 LayerNorm output (test_layernorm: rtol 1e-5, atol 1e-5; a mean of values each within it is within its
mean) plus the worst case of an n_p-term fp32 sum in any order.  Row 0 goes through the expressions of ln_fwd_kernel's fp32 output, so it is
compared with dcv_ln_fwd bit for bit.  Model: max |out - ref| <= 3e-2 max |ref| per returned layer, the bound every eval-feature check in
tests/test_model_gpu.py uses for final-normed features; a CPU emulation of the reference with bf16-rounded Linear operands and outputs stays at
<= 4.0e-3 of max |ref| on the tokens (2.8e-3 pooled) while the neighbouring layer's tokens differ by 0.17-0.31 of max |ref|.  Measured on the
MI355X: tokens 3.3e-3 .. 6.3e-3, pooled 4.3e-3 .. 9.2e-3 of max |ref| (DiChaViT-B the largest); the kernel at most 0.012 of its bound."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import dichavit_oracle as orc

pytestmark = pytest.mark.gpu

EPS = 1e-6


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


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _inputs(B, C, n_p, D, seed):
    """Random rows with a row mean far from zero, as test_ln_fwd_bwd_per_element uses."""
    N = 1 + C * n_p
    x = torch.randn(B, N, D, device="cuda", generator=_gen(seed)) * 3.0 + 5.0
    gamma = 1 + 0.1 * torch.randn(D, device="cuda", generator=_gen(seed + 1))
    beta = 0.1 * torch.randn(D, device="cuda", generator=_gen(seed + 2))
    return x, gamma, beta


def _pool(hip, x, gamma, beta, B, C, n_p, D, out=None):
    if out is None:
        out = torch.full((B, 1 + C, D), float("nan"), device="cuda")
    hip.ln_pool_channels(x, gamma, beta, out, B, C, n_p, D, EPS)
    return out


def _pooled_ref64(x, gamma, beta, B, C, n_p, D):
    """float64 of the same formulas -> (reference rows 1 .. C [B, C, D], the bound's a [B, C, D])."""
    g, b = gamma.double(), beta.double()
    ref = torch.empty(B, C, D, dtype=torch.float64, device=x.device)
    a = torch.empty_like(ref)
    for i in range(B):  # one image at a time: the float64 copy of the headline shape would be 1.2 GB
        x64 = x[i, 1:].double()
        mu = x64.mean(-1, keepdim=True)
        xh = ((x64 - mu) * (((x64 - mu) ** 2).mean(-1, keepdim=True) + EPS).rsqrt()).view(C, n_p, D)
        ref[i] = xh.mean(1) * g + b
        a[i] = (g.abs() * xh.abs() + b.abs()).mean(1)
    return ref, a


def _bound(a, n_p):
    return 1e-5 + 1e-5 * a + n_p * 2.0 ** -24 * a


SHAPES = [(64, 8, 196, 384),   # the headline shape: 4 splits per segment
          (64, 3, 196, 384),   # CHAMMI-sized: 11 splits
          (1, 3, 196, 384),    # fewer segments than CUs: 22 splits of 9 rows
          (2, 18, 16, 384),    # So2Sat-like: 2 splits of 8 rows
          (2, 1, 36, 192),     # one channel, DiChaViT-tiny
          (1, 8, 1, 768),      # a segment of one row
          (2, 3, 36, 768),     # DiChaViT-B width (4 float4 per lane)
          (64, 18, 16, 192),
          (2, 8, 15, 384)]     # one workgroup per segment, a partial last round of rows


@pytest.mark.parametrize("B,C,n_p,D", SHAPES)
def test_pool_kernel_against_float64(hip, B, C, n_p, D):
    x, gamma, beta = _inputs(B, C, n_p, D, seed=B + 7 * C + 13 * n_p + D)
    out = _pool(hip, x, gamma, beta, B, C, n_p, D)
    assert torch.isfinite(out).all()
    ref, a = _pooled_ref64(x, gamma, beta, B, C, n_p, D)
    err = (out[:, 1:].double() - ref).abs()
    bound = _bound(a, n_p)
    print(f"B{B} C{C} n_p{n_p} D{D}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
    bad = err > bound
    assert not bad.any(), f"{int(bad.sum())}/{bad.numel()} off, max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}"
    # row 0: the same row routine as dcv_ln_fwd's fp32 output
    N = 1 + C * n_p
    cls = torch.full((B, D), float("nan"), device="cuda")
    hip.ln_fwd(x, gamma, beta, cls, None, None, B, D, EPS, x_row_stride=N * D)
    assert torch.equal(out[:, 0], cls)


@pytest.mark.parametrize("B,C,n_p,D", [(2, 3, 196, 384), (3, 5, 16, 768), (2, 4, 7, 192)], ids=["split", "split-wide", "whole"])
def test_pool_kernel_determinism_and_seams(hip, B, C, n_p, D):
    x, gamma, beta = _inputs(B, C, n_p, D, seed=77 + n_p)
    N = 1 + C * n_p
    first = _pool(hip, x, gamma, beta, B, C, n_p, D)
    assert torch.equal(first, _pool(hip, x, gamma, beta, B, C, n_p, D))
    # exactly [B, 1 + C, D] is written: NaN-filled buffer with guard regions before and after
    G, n_out = 4096, B * (1 + C) * D
    buf = torch.full((G + n_out + G,), float("nan"), device="cuda")
    inner = buf[G:G + n_out].view(B, 1 + C, D)
    _pool(hip, x, gamma, beta, B, C, n_p, D, out=inner)
    torch.cuda.synchronize()
    assert torch.isfinite(inner).all() and torch.equal(inner, first)
    assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n_out:]).all()
    # no row crosses a segment boundary: NaN in the rows of one (image, channel) segment reaches exactly that output row
    for b, c in [(0, 0), (B - 1, C - 1), (B - 1, C // 2)]:
        xp = x.clone()
        xp[b, 1 + c * n_p:1 + (c + 1) * n_p] = float("nan")
        got = _pool(hip, xp, gamma, beta, B, C, n_p, D)
        assert torch.isnan(got[b, 1 + c]).all()
        mask = torch.ones(B, 1 + C, dtype=torch.bool, device="cuda")
        mask[b, 1 + c] = False
        assert torch.equal(got[mask], first[mask])
    # ... and a NaN CLS row reaches row 0 of its image alone
    xp = x.clone()
    xp[B - 1, 0] = float("nan")
    got = _pool(hip, xp, gamma, beta, B, C, n_p, D)
    assert torch.isnan(got[B - 1, 0]).all() and torch.equal(got[B - 1, 1:], first[B - 1, 1:]) and torch.equal(got[:B - 1], first[:B - 1])


def test_pool_kernel_refusals(hip):
    """Real tensors behind every pointer, large enough for any of the shapes named: a refused call must not have launched anything."""
    B, C, n_p = 2, 3, 16
    x = torch.randn(B * (1 + C * n_p) * 1028, device="cuda")
    gamma, beta = torch.ones(1028, device="cuda"), torch.zeros(1028, device="cuda")
    out = torch.full((B * (1 + C) * 1028,), float("nan"), device="cuda")
    for D in (386, 1028):
        with pytest.raises(RuntimeError, match="dcv_ln_pool_channels|workspace"):
            hip.ln_pool_channels(x, gamma, beta, out, B, C, n_p, D, EPS)
    need = hip.load().dcv_ln_pool_channels_ws_floats(B, C, n_p, 384)
    assert need == B * C * 2 * 384
    with pytest.raises(RuntimeError, match="dcv_ln_pool_channels"):
        hip.ln_pool_channels(x, gamma, beta, out, B, C, n_p, 384, EPS, ws=torch.empty(need - 4, device="cuda"))
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    hip.ln_pool_channels(x, gamma, beta, out, B, C, n_p, 384, EPS, ws=torch.empty(need, device="cuda"))  # the exact size is enough
    assert torch.isfinite(out[:B * (1 + C) * 384]).all()


# ------------------------------------------------------------------------------------------------------------------------------------
def _build(case, device, chammi=False):
    import diverse_channel_vit_amd as dcv
    cfg = Cfg(case["cfg"], in_channel_names=[f"c{i}" for i in range(case["n_channels"])], img_size=[case["img"]],
              num_classes=case["num_classes"])
    model = dcv.dichavit(cfg, mapper={k: list(v) for k, v in case["mapper"].items()})
    st = orc.make_state(orc.state_shapes(case["cfg"], case["n_channels"], case["img"], case["num_classes"], chammi=chammi), case["seed"])
    model.load_state_dict({**st, "adaptive_interface.0": st["proxies"]}, strict=True)
    return model.to(device).eval()


def _batch(case, device):
    x, _ = orc.make_batch(case["batch_seed"], case["B"], len(case["mapper"][case["chunk"]]), case["img_in"], case["num_classes"])
    return x.to(device)


def _pool64(t, C):
    """[B, 1 + C n_p, D] tokens -> [B, 1 + C, D] in float64: CLS, then the per-channel means."""
    t = t.double()
    B, N, D = t.shape
    return torch.cat([t[:, :1], t[:, 1:].view(B, C, (N - 1) // C, D).mean(2)], dim=1)


def test_model_tokens_against_the_reference(gpu_device):
    meta, a = load_golden("intermediate_layers")
    figures = {}
    for case in meta["cases"]:
        assert case["reference_method_raises"] == "TypeError"  # the reference's own body cannot run
        model = _build(case, gpu_device)
        fe = model.feature_extractor
        x = _batch(case, gpu_device)
        C = len(case["mapper"][case["chunk"]])
        refs = [torch.from_numpy(a[f"{case['name']}/block{i}"]).to(gpu_device).float() for i in case["blocks"]]  # stored in float16
        toks = fe.get_intermediate_layers(x, n=case["n"], chunk=case["chunk"])
        pooled = fe.get_intermediate_layers(x, n=case["n"], chunk=case["chunk"], pool="channel")
        assert isinstance(toks, list) and len(toks) == len(pooled) == case["n"]
        for k, (t, p, ref) in enumerate(zip(toks, pooled, refs)):
            assert t.dtype == p.dtype == torch.float32 and t.device == x.device and not t.requires_grad and not p.requires_grad
            assert t.shape == ref.shape and p.shape == (case["B"], 1 + C, ref.shape[-1])
            scale = ref.abs().max().item()
            err = (t - ref).abs().max().item()
            ref_p = _pool64(ref, C)
            err_p = (p.double() - ref_p).abs().max().item()
            scale_p = ref_p.abs().max().item()
            figures[(case["name"], case["blocks"][k])] = (err / scale, err_p / scale_p)
            print(f"{case['name']} block {case['blocks'][k]}: tokens {err / scale:.3e} of max |ref|, pooled {err_p / scale_p:.3e}")
            assert err <= 3e-2 * scale, f"{case['name']} block {case['blocks'][k]}: {err:.3e} > 3e-2 * {scale:.3f}"
            assert err_p <= 3e-2 * scale_p, f"{case['name']} block {case['blocks'][k]} pooled: {err_p:.3e} > 3e-2 * {scale_p:.3f}"
            # the bound separates: every other layer of the fixture is far outside it
            for j, other in enumerate(refs):
                if j != k:
                    assert (t - other).abs().max().item() > 3e-2 * other.abs().max().item(), (case["name"], k, j)
        del model
    print("max error / max |ref| per (case, block): (tokens, pooled)", {k: (f"{v[0]:.2e}", f"{v[1]:.2e}") for k, v in figures.items()})


def test_consistency_inside_the_library(gpu_device):
    meta, _ = load_golden("intermediate_layers")
    case = meta["cases"][0]
    model = _build(case, gpu_device)
    fe = model.feature_extractor
    x = _batch(case, gpu_device)
    C, D = 5, model.dim
    four = fe.get_intermediate_layers(x, n=4, chunk="train")
    pooled = fe.get_intermediate_layers(x, n=4, chunk="train", pool="channel")
    g, b = fe.norm.weight.detach().double(), fe.norm.bias.detach().double()
    for t, p in zip(four, pooled):
        # pool="channel" against pool=None pooled in float64, within the kernel's bound with a taken from the returned tokens themselves:
        # |LN output| <= |gamma| |x^| + |beta| per element, so this a is no larger than the bound's and the check no weaker
        n_p = (t.shape[1] - 1) // C
        a = _pool64(t.abs(), C)[:, 1:]
        assert ((p[:, 1:].double() - _pool64(t, C)[:, 1:]).abs() <= _bound(a, n_p)).all()
        assert torch.equal(p[:, 0], t[:, 0])
    # a list of indices, negative indices, the default
    assert torch.equal(fe.get_intermediate_layers(x, n=[11], chunk="train")[0], fe.get_intermediate_layers(x, chunk="train")[0])
    assert torch.equal(fe.get_intermediate_layers(x, {}, 1, chunk="train")[0], four[3])
    for k, bi in enumerate((8, 9, 10, 11)):
        assert torch.equal(fe.get_intermediate_layers(x, n=[bi], chunk="train")[0], four[k]), bi
    mixed = fe.get_intermediate_layers(x, n=(-1, 8), chunk="train", pool="channel")
    assert len(mixed) == 2 and torch.equal(mixed[0], pooled[0]) and torch.equal(mixed[1], pooled[3])
    early = fe.get_intermediate_layers(x, n=[0], chunk="train")[0]
    assert early.shape == four[0].shape and torch.isfinite(early).all()
    with pytest.raises(KeyError):
        fe.get_intermediate_layers(x)  # chunk="" is no mapper key, as in get_last_selfattention


def test_last_entry_row0_is_the_forward_feature(gpu_device):
    """A CHAMMI-style model (an "Allen" chunk in the mapper: nn.Identity head, model(x, chunk) returns the final-normed CLS feature).  With
    cls_only_tail off the forward runs the last block on all rows — the same launches on the same nearest-rounded operands as the capture — so
    row 0 of the last entry equals it bit for bit; with the default CLS-only tail the feature comes from other launches (one-row GEMMs, the
    one-query attention) and agrees within the eval-feature bound."""
    meta, _ = load_golden("chammi")
    case = dict(cfg=meta["cfg"], n_channels=meta["n_channels"], img=meta["img"], num_classes=meta["num_classes"], seed=meta["seed"],
                mapper=meta["mapper"])
    model = _build(case, gpu_device, chammi=True)
    ch = meta["mapper"]["Allen"]
    x, _ = orc.make_batch(meta["seed"] + len(ch), 2, len(ch), meta["img"], meta["num_classes"])
    x = x.to(gpu_device)
    fe = model.feature_extractor
    for pool in (None, "channel"):
        last = fe.get_intermediate_layers(x, n=1, chunk="Allen", pool=pool)[0]
        assert model.cls_only_tail
        with torch.no_grad():
            feat_tail = model(x, "Allen")
        assert feat_tail.shape == last[:, 0].shape
        assert (last[:, 0] - feat_tail).abs().max().item() <= 3e-2 * feat_tail.abs().max().item()
        model.cls_only_tail = False
        try:
            with torch.no_grad():
                feat = model(x, "Allen")
        finally:
            model.cls_only_tail = True
        assert torch.equal(last[:, 0], feat), (pool, (last[:, 0] - feat).abs().max().item())


def test_call_leaves_the_training_step_alone(gpu_device):
    """A call between loss = ... and loss.backward() must not touch what the backward reads (the stochastically rounded operand copies, the
    pre-scaled q bias, the rounding seed, the arenas): gradients and the next step's loss are bit-identical to the same sequence without it."""
    from diverse_channel_vit_amd import hip
    from diverse_channel_vit_amd.optim import HipAdamW
    assert hip.is_deterministic()
    meta, _ = load_golden("intermediate_layers")
    case = meta["cases"][0]
    x = _batch(case, gpu_device)
    y = torch.arange(case["B"], device=gpu_device) % case["num_classes"]
    runs = []
    for probe in (False, True):
        model = _build(case, gpu_device).train()
        assert model.stochastic_weight_rounding
        opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=0.04, model=model)
        out, extra = model(x, case["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss = torch.nn.functional.cross_entropy(out, y) + extra
        if probe:
            model.eval()
            got = model.feature_extractor.get_intermediate_layers(x, n=4, chunk=case["chunk"], pool="channel")
            assert len(got) == 4 and all(torch.isfinite(t).all() for t in got)
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


def test_train_mode_token_drop_and_hcs(gpu_device):
    import random
    meta, _ = load_golden("intermediate_layers")
    case = meta["cases"][0]
    x = _batch(case, gpu_device)
    # token drop: the channel segments are ragged
    dropped = dict(case, cfg=dict(case["cfg"], dropout_tokens_hcs="random"))
    model = _build(dropped, gpu_device).train()
    fe = model.feature_extractor
    random.seed(5)
    with pytest.raises(ValueError, match="ragged"):
        fe.get_intermediate_layers(x, chunk="train", pool="channel")
    random.seed(5)
    kept = fe.get_intermediate_layers(x, chunk="train")[0]
    assert kept.shape[0] == 1 and kept.shape[2] == 384 and 16 <= kept.shape[1] <= 1 + 5 * 16 and torch.isfinite(kept).all()
    model.eval()  # eval ignores the option
    assert fe.get_intermediate_layers(x, chunk="train", pool="channel")[0].shape == (1, 6, 384)
    del model
    # HCS in train mode with a pinned sampler: 1 + C_sampled rows, in the subset's order
    hcs = dict(case, cfg=dict(case["cfg"], enable_sample=True))
    model = _build(hcs, gpu_device).train()
    picked = [3, 0, 4]
    model.hcs_sampler = lambda m, chunk, cur, picked=picked: (picked, [cur.index(c) for c in picked])
    fe = model.feature_extractor
    p = fe.get_intermediate_layers(x, n=2, chunk="train", pool="channel")
    t = fe.get_intermediate_layers(x, n=2, chunk="train")
    assert [tuple(v.shape) for v in p] == [(1, 4, 384)] * 2 and [tuple(v.shape) for v in t] == [(1, 1 + 3 * 16, 384)] * 2
    assert torch.equal(p[1][:, 0], t[1][:, 0])
    model.eval()
    full = fe.get_intermediate_layers(x, chunk="train", pool="channel")[0]
    assert full.shape == (1, 6, 384)


def test_dump_features_layers(gpu_device, tmp_path):
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("chammi")
    case = dict(cfg=meta["cfg"], n_channels=meta["n_channels"], img=meta["img"], num_classes=meta["num_classes"], seed=meta["seed"],
                mapper=meta["mapper"])
    model = _build(case, gpu_device, chammi=True)
    D = model.dim
    loaders = {c: [orc.make_batch(400 + len(meta["mapper"][c]) + i, 2, len(meta["mapper"][c]), meta["img"], 14)[0] for i in range(2)]
               for c in ("Allen", "HPA")}
    kw = dict(training_chunks="Allen_CP", new_channel_init="avg_2", device=gpu_device)
    paths = dcv.dump_features(model, loaders, str(tmp_path / "probe"), "features.npy", layers=4, pool="channel", **kw)
    plain = dcv.dump_features(model, loaders, str(tmp_path / "cls"), "features.npy", layers=4, **kw)
    default = dcv.dump_features(model, loaders, str(tmp_path / "default"), "features.npy", **kw)
    fe = model.feature_extractor
    for c, pth, pth_plain, pth_default in zip(("Allen", "HPA"), paths, plain, default):
        f = np.load(pth)
        assert f.shape == (4, 5 * D) and f.dtype == np.float32
        rows = []
        for xb in loaders[c]:
            got = fe.get_intermediate_layers(xb.to(gpu_device), n=4, chunk=c, training_chunks="Allen_CP", new_channel_init="avg_2", pool="channel")
            rows.append(torch.cat([t[:, 0] for t in got] + [got[-1][:, 1:].mean(1)], dim=-1).cpu())
        want = torch.cat(rows).numpy()
        assert np.array_equal(f, want)
        assert np.array_equal(np.load(pth_plain), want[:, :4 * D])
        # the default call: the model's own output, as before
        with torch.no_grad():
            out = torch.cat([model(xb.to(gpu_device), c, "Allen_CP", init_first_layer=None, new_channel_init="avg_2").float().cpu()
                             for xb in loaders[c]]).numpy()
        assert np.array_equal(np.load(pth_default), out) and out.shape == (4, D)
