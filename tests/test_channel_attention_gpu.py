"""get_channel_attention on the MI355X: the channel-mass kernel (dcv_attn_channel_mass / _ps) against float64 torch, its internal consistency,
and the model method against the real reference's maps (tests/golden/attn_maps.npz) lumped in float64 (channel_lumping.py).

Bounds.  Kernel: |got - ref| <= 3e-4 ref + 1e-6 for the token masses T and the channel matrix A (ref: float64 softmax of the same bf16 q, k, then
the one-hot lumping) — the relative part is the per-element bound test_probs_kernel_against_torch holds for p, and a sum of positive terms that
are each within a relative bound is within it; the floor covers masses near underflow — and every row sum of T and A within 1e-4 of 1.
Model: mean total variation against the lumped fixture map <= 1e-2, the TV_BOUND of test_attn_maps_gpu.py: lumping cannot increase total
variation, and the token-level test holds that bound.
Measured on the MI355X (the tests print these): kernel, worst case over the seven shapes and both forms, max |got - ref| / (3e-4 ref + 1e-6) =
0.038 for T and 0.024 for A, row sums within 1.13e-5 of 1; with n_p = 1 T equals dcv_attn_probs_rows' map bit for bit; model mean total
variation per (case, layer) 2.4e-4 .. 1.6e-3, and 6.8e-4 of the kernel bound against get_last_selfattention lumped in float64."""
import copy
import ctypes as C
import math

import pytest
import torch

from channel_lumping import lump, mean_tv
from conftest import load_golden
from oracle import dichavit_oracle as orc

pytestmark = pytest.mark.gpu

TV_BOUND = 1e-2
SCALE = 64 ** -0.5
ERR_SHAPE, ERR_NULL = -1, -5


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
        qkv[..., :D] *= SCALE * math.log2(math.e)  # q' = q scale log2(e), as the model's pre-scaled operand copies deliver it
    qkv = qkv.to(torch.bfloat16).cuda()
    if N > 1:  # one spiked key against one query (as test_attention_fwd_bwd): a late tile raises the row maximum
        qkv[0, N // 2, :64] *= 4
        qkv[0, N - 1, D:D + 64] = qkv[0, N // 2, :64]
    return qkv


def _probs64(qkv, B, N, H, prescaled):
    t = qkv.double().view(B, N, 3, H, 64)
    q, k = t[:, :, 0].transpose(1, 2), t[:, :, 1].transpose(1, 2)
    return torch.softmax(q @ k.transpose(-1, -2) * (math.log(2.0) if prescaled else SCALE), dim=-1)


def _lse(hip, qkv, B, N, H, prescaled):
    o = torch.empty(B, N, H * 64, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, N, device="cuda")
    hip.attn_fwd(qkv, o, lse, B, N, H, 64, SCALE, prescaled=prescaled)
    return lse


def _mass(hip, qkv, lse, B, N, H, C_, n_p, prescaled, tok=True, ch=True, ws=None):
    T = torch.empty(B, H, N, 1 + C_, device="cuda") if tok is True else tok if tok is not False else None
    A = torch.empty(B, H, 1 + C_, 1 + C_, device="cuda") if ch is True else ch if ch is not False else None
    hip.attn_channel_mass(qkv, lse, B, N, H, 64, SCALE, C_, n_p, tok=T, ch=A, prescaled=prescaled, ws=ws)
    return T, A


def _within(got, ref):
    """max of |got - ref| / (3e-4 ref + 1e-6): the kernel bound holds when <= 1"""
    return ((got.double() - ref).abs() / (3e-4 * ref + 1e-6)).max().item()


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
@pytest.mark.parametrize("B,H,C_,n_p", [(2, 6, 1, 1), (2, 6, 12, 4), (1, 3, 64, 1), (2, 6, 5, 16), (1, 3, 3, 36), (2, 6, 2, 64), (1, 2, 8, 196)])
def test_kernel_against_float64(hip, B, H, C_, n_p, prescaled):
    N = 1 + C_ * n_p
    qkv = _qkv(B, N, H, seed=N + 7 * H, prescaled=prescaled)
    lse = _lse(hip, qkv, B, N, H, prescaled)
    T, A = _mass(hip, qkv, lse, B, N, H, C_, n_p, prescaled)
    assert T.shape == (B, H, N, 1 + C_) and A.shape == (B, H, 1 + C_, 1 + C_)
    Tr, Ar = lump(_probs64(qkv, B, N, H, prescaled), C_, n_p)
    wt, wa = _within(T, Tr), _within(A, Ar)
    rt, ra = (T.double().sum(-1) - 1).abs().max().item(), (A.double().sum(-1) - 1).abs().max().item()
    print(f"B{B} H{H} C{C_} n_p{n_p} {'ps' if prescaled else 'plain'}: max err / bound T {wt:.3f} A {wa:.3f}; max |row sum - 1| T {rt:.2e} A {ra:.2e}")
    assert wt <= 1, f"T: max |got - ref| / (3e-4 ref + 1e-6) = {wt:.3g}"
    assert wa <= 1, f"A: max |got - ref| / (3e-4 ref + 1e-6) = {wa:.3g}"
    assert rt <= 1e-4 and ra <= 1e-4
    if n_p == 1:  # every key its own segment: T is the probability matrix itself
        P = torch.empty(B, H, N, N, device="cuda")
        hip.attn_probs(qkv, lse, P, B, N, H, 64, SCALE, prescaled=prescaled)
        wp = _within(T, P.double())
        print(f"    against attn_probs: max err / bound {wp:.3g}, bit-identical: {torch.equal(T, P)}")
        assert wp <= 1


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
def test_kernel_consistency(hip, prescaled):
    B, H, C_, n_p = 2, 6, 5, 16
    N, W = 1 + C_ * n_p, 1 + C_
    qkv = _qkv(B, N, H, seed=99, prescaled=prescaled)
    lse = _lse(hip, qkv, B, N, H, prescaled)
    T, A = _mass(hip, qkv, lse, B, N, H, C_, n_p, prescaled)
    # A is the segment mean of the kernel's own T; its CLS row is T's, bit for bit
    seg = torch.cat([T[:, :, :1].double(), T[:, :, 1:].double().view(B, H, C_, n_p, W).mean(3)], dim=2)
    assert (A.double() - seg).abs().max().item() <= 1e-6
    assert torch.equal(A[:, :, 0], T[:, :, 0])
    # two calls agree bit for bit; each output requested alone equals the pair's
    T2, A2 = _mass(hip, qkv, lse, B, N, H, C_, n_p, prescaled)
    assert torch.equal(T, T2) and torch.equal(A, A2)
    T3, none = _mass(hip, qkv, lse, B, N, H, C_, n_p, prescaled, ch=False)
    assert none is None and torch.equal(T3, T)
    none, A3 = _mass(hip, qkv, lse, B, N, H, C_, n_p, prescaled, tok=False)
    assert none is None and torch.equal(A3, A)
    # the kernel writes exactly its outputs and its workspace: NaN-filled buffers with guard regions before and after
    G = 4096
    nT, nA = B * H * N * W, B * H * W * W
    nW = hip.load().dcv_attn_channel_mass_ws_floats(B, N, H, C_)
    assert nW == nT

    def guarded(n):
        buf = torch.full((G + n + G,), float("nan"), device="cuda")
        return buf, buf[G:G + n]

    def guards_intact(buf, n):
        return bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n:]).all())

    bT, iT = guarded(nT)
    bA, iA = guarded(nA)
    bW, iW = guarded(nW)
    _mass(hip, qkv, lse, B, N, H, C_, n_p, prescaled, tok=iT.view(B, H, N, W), ch=iA.view(B, H, W, W), ws=iW)
    torch.cuda.synchronize()
    assert torch.isfinite(iT).all() and torch.isfinite(iA).all()
    assert guards_intact(bT, nT) and guards_intact(bA, nA) and guards_intact(bW, nW)
    assert torch.equal(iT.view_as(T), T) and torch.equal(iA.view_as(A), A)
    # the channel matrix alone goes through the workspace: NaN on entry does not reach the output, nothing outside it is touched
    bA, iA = guarded(nA)
    _mass(hip, qkv, lse, B, N, H, C_, n_p, prescaled, tok=False, ch=iA.view(B, H, W, W), ws=iW)
    torch.cuda.synchronize()
    assert torch.isfinite(iA).all() and torch.equal(iA.view_as(A), A)
    assert guards_intact(bA, nA) and guards_intact(bW, nW)
    # ... and so through the stream's shared workspace, whatever it held
    hip._workspace(nW, A).fill_(float("nan"))
    assert torch.equal(_mass(hip, qkv, lse, B, N, H, C_, n_p, prescaled, tok=False)[1], A)


def test_kernel_refusals(hip):
    """Real tensors behind every pointer: a refused call returns its error code and must not have launched anything."""
    B, H, C_, n_p = 2, 6, 5, 16
    N, W = 1 + C_ * n_p, 1 + C_
    qkv = _qkv(B, N + 4, H, seed=3, prescaled=False)  # large enough for any of the shapes named
    lse = torch.zeros(B, H, N + 4, device="cuda")
    T = torch.full((B * H * (N + 4) * (W + 2),), float("nan"), device="cuda")
    A = torch.full((B * H * (W + 2) * (W + 2),), float("nan"), device="cuda")
    ws = torch.full((B * H * (N + 4) * (W + 2),), float("nan"), device="cuda")
    lib = hip.load()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ps, tok=T, ch=A, N_=N, C__=C_, n_p_=n_p, w=ws, wf=None):
        wf = (w.numel() if w is not None else 0) if wf is None else wf
        if ps:
            return lib.dcv_attn_channel_mass_ps(p(qkv), p(lse), p(tok), p(ch), B, N_, H, 64, C__, n_p_, p(w), wf, st)
        return lib.dcv_attn_channel_mass(p(qkv), p(lse), p(tok), p(ch), B, N_, H, 64, SCALE, C__, n_p_, p(w), wf, st)

    for ps in (False, True):
        for kw in (dict(N_=N + 1), dict(N_=N - 1), dict(C__=C_ + 1), dict(n_p_=n_p - 1), dict(C__=0), dict(n_p_=0), dict(tok=None, wf=B * H * N * W - 1)):
            assert call(ps, **kw) == ERR_SHAPE, kw
        assert call(ps, tok=None, ch=None) == ERR_NULL
        assert call(ps, tok=None, w=None) == ERR_NULL
    with pytest.raises(RuntimeError, match="dcv_attn_channel_mass"):
        hip.attn_channel_mass(qkv, lse, B, N, H, 64, SCALE, C_, n_p - 1, tok=T, ch=A)
    with pytest.raises(ValueError, match="both None"):
        hip.attn_channel_mass(qkv, lse, B, N, H, 64, SCALE, C_, n_p)
    torch.cuda.synchronize()
    assert torch.isnan(T).all() and torch.isnan(A).all() and torch.isnan(ws).all()


# ------------------------------------------------------------------------------------------------------------------------------------
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


def test_model_against_the_reference(gpu_device):
    meta, a = load_golden("attn_maps")
    tvs, worst = {}, 0.0
    for case in meta["cases"]:
        model = _build(case, case["qk_mult"], gpu_device)
        fe = model.feature_extractor
        x = _batch(case, gpu_device)
        C_ = len(case["mapper"][case["chunk"]])
        for li in case["layers"]:
            ref = torch.from_numpy(a[f"{case['name']}/layer{li}"]).to(gpu_device)  # stored in float16
            N = ref.shape[-1]
            n_p = (N - 1) // C_
            Tr, Ar = lump(ref, C_, n_p)
            got = fe.get_channel_attention(x, chunk=case["chunk"], n=[li])
            assert isinstance(got, list) and len(got) == 1
            A = got[0]
            assert A.dtype == torch.float32 and A.shape == Ar.shape and A.device == x.device and not A.requires_grad
            tv = mean_tv(A, Ar)
            tvs[(case["name"], li)] = tv
            assert tv <= TV_BOUND, f"{case['name']} layer {li}: mean total variation {tv:.3e}"
            # the token form, and both against the library's own N x N map of the same block lumped in float64
            T = fe.get_channel_attention(x, chunk=case["chunk"], n=[li], queries="token")[0]
            assert T.dtype == torch.float32 and T.shape == Tr.shape and not T.requires_grad
            assert mean_tv(T, Tr) <= TV_BOUND
            seg = torch.cat([T[:, :, :1].double(), T[:, :, 1:].double().view(T.shape[0], T.shape[1], C_, n_p, 1 + C_).mean(3)], dim=2)
            assert (A.double() - seg).abs().max().item() <= 1e-6
            Tp, Ap = lump(fe.get_last_selfattention(x, chunk=case["chunk"], layer_idx=li), C_, n_p)
            wt, wa = _within(T, Tp), _within(A, Ap)
            worst = max(worst, wt, wa)
            assert wt <= 1 and wa <= 1, f"{case['name']} layer {li}: against get_last_selfattention, err / bound T {wt:.3g} A {wa:.3g}"
        if case["name"] == "sub":
            assert C_ == 3 and A.shape == (case["B"], 6, 4, 4) and T.shape == (case["B"], 6, 49, 4)  # 3 of the 5 channels
        if case["name"] == "small":
            # the bound separates: the lumped map of another layer is far outside it
            wrong = mean_tv(fe.get_channel_attention(x, chunk=case["chunk"], n=1)[0], lump(torch.from_numpy(a["small/layer5"]).to(gpu_device), 5, 16)[1])
            assert wrong >= 10 * TV_BOUND, wrong
            with pytest.raises(KeyError):
                fe.get_channel_attention(x)  # as get_last_selfattention: the default chunk "" is no mapper key
        del model
    print("mean total variation of A per (case, layer):", {k: f"{v:.2e}" for k, v in tvs.items()})
    print(f"against get_last_selfattention lumped in float64: worst err / bound {worst:.3g}")


def test_all_blocks_in_one_forward(gpu_device):
    meta, _ = load_golden("attn_maps")
    case = meta["cases"][0]
    model = _build(case, case["qk_mult"], gpu_device)
    fe = model.feature_extractor
    x = _batch(case, gpu_device)
    depth = len(fe.blocks)
    assert depth == 12
    every = {}
    for q, shape in (("channel", (1, 6, 6, 6)), ("token", (1, 6, 81, 6))):
        every[q] = fe.get_channel_attention(x, chunk="train", n=depth, queries=q)
        assert len(every[q]) == depth and all(tuple(t.shape) == shape for t in every[q])
        for li in range(depth):
            assert torch.equal(every[q][li], fe.get_channel_attention(x, chunk="train", n=[li], queries=q)[0]), (q, li)
        assert all((t.double().sum(-1) - 1).abs().max().item() <= 1e-4 for t in every[q])
    # a list of indices comes back in block order; the default is the last block
    some = fe.get_channel_attention(x, chunk="train", n=[-1, 2, 7])
    assert len(some) == 3 and all(torch.equal(s, every["channel"][i]) for s, i in zip(some, (2, 7, 11)))
    assert torch.equal(fe.get_channel_attention(x, chunk="train")[0], every["channel"][11])


def test_train_mode_token_drop_and_hcs(gpu_device):
    import random
    meta, _ = load_golden("attn_maps")
    case = meta["cases"][0]
    x = _batch(case, gpu_device)
    # token drop: the channel segments are ragged
    model = _build(dict(case, cfg=dict(case["cfg"], dropout_tokens_hcs="channel")), case["qk_mult"], gpu_device).train()
    fe = model.feature_extractor
    random.seed(5)
    for q in ("channel", "token"):
        with pytest.raises(ValueError, match="ragged"):
            fe.get_channel_attention(x, chunk="train", queries=q)
    model.eval()  # eval ignores the option
    assert fe.get_channel_attention(x, chunk="train")[0].shape == (1, 6, 6, 6)
    del model
    # HCS in train mode with a pinned sampler: the segments are the sampled subset's, in its order
    model = _build(dict(case, cfg=dict(case["cfg"], enable_sample=True)), case["qk_mult"], gpu_device).train()
    picked = [3, 0, 4]
    model.hcs_sampler = lambda m, chunk, cur, picked=picked: (picked, [cur.index(c) for c in picked])
    fe = model.feature_extractor
    A, = fe.get_channel_attention(x, chunk="train")
    T, = fe.get_channel_attention(x, chunk="train", queries="token")
    assert A.shape == (1, 6, 4, 4) and T.shape == (1, 6, 49, 4)
    assert (A.double().sum(-1) - 1).abs().max().item() <= 1e-4 and torch.equal(A[:, :, 0], T[:, :, 0])


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
            got = model.feature_extractor.get_channel_attention(x, chunk=case["chunk"], n=12)
            got += model.feature_extractor.get_channel_attention(x, chunk=case["chunk"], n=[5], queries="token")
            assert len(got) == 13 and all(torch.isfinite(t).all() for t in got)
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
    A0 = model.feature_extractor.get_channel_attention(x, chunk=case["chunk"], n=[0])[0]
    cp = copy.deepcopy(model)
    assert torch.equal(cp.feature_extractor.get_channel_attention(x, chunk=case["chunk"], n=[0])[0], A0)
    with torch.no_grad():
        cp.feature_extractor.blocks[0].attn.qkv.weight.mul_(1.5)
    Ac = cp.feature_extractor.get_channel_attention(x, chunk=case["chunk"], n=[0])[0]
    assert mean_tv(Ac, A0) > 1e-5  # two orders above fp32 rounding of a row of masses (1e-7): other weights, not noise
    assert torch.equal(model.feature_extractor.get_channel_attention(x, chunk=case["chunk"], n=[0])[0], A0)
