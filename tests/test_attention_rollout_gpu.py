"""get_attention_rollout on the MI355X: the rollout-step kernel (dcv_attn_rollout_step / _ps) against float64 torch, its internal consistency,
the model method against the float64 rollout of its own get_last_selfattention maps, and against the rollout of the real reference's maps
(tests/golden/attn_rollout.npz, every start layer).

Bounds.  Kernel: |got - ref| <= 3e-4 ref + 1e-6 sum(w) (ref: float64 softmax of the same bf16 q, k, pushed through alpha I + (1 - alpha) mean_h P) —
the relative part is the per-element bound test_probs_kernel_against_torch holds for p, and out is a non-negative combination of p's plus one
exactly representable term; |sum_k out - sum_k w| <= 1e-4 sum(w).  Model against its own maps, start layer s of L = 12 blocks:
(L - s) (6e-4 ref + 2e-6) element by element — the kernel's 3e-4 and the map's 3e-4 per block rolled; non-negative linear steps preserve relative
bounds.  Model against the reference fixture: tv <= (1 - residual) (L - s) 1e-2, the TV_BOUND of test_attn_maps_gpu.py per block actually
rolled.  That ceiling discriminates only at high s (the full rollout lies within 0.02 .. 0.06 of the uniform vector); s = 0 is carried by the
comparison with the model's own maps, which test_attn_maps_gpu.py holds to the reference.
Measured on the MI355X (the tests print these): kernel, worst case over the ten shapes, four kinds of w, three alpha and both forms, max
|got - ref| / (3e-4 ref + 1e-6 sum w) = 0.004 (0.009 at B = 600) and |sum out - sum w| <= 6.3e-7 sum w; w = e_0 against attn_probs(nq=1): 0.034 of
the bound; twelve chained steps: 9.5e-5 of theirs.  Model against its own maps: at most 3.7e-4 of the bound over the four cases and twelve start
layers (residual 0.25: 1.8e-4; random start: 4.4e-5).  Model against the reference's rollout: total variation 1.1e-4 .. 4.2e-4 at s = 0 rising to
7.4e-4 .. 3.7e-3 at s = 11 (ceiling there 5e-3).  The bounds are the ones reasoned above, not tightened to these."""
import copy
import ctypes as C
import math
import random

import pytest
import torch

from attention_rollout_ref import rollout, tv
from conftest import load_golden
from oracle import dichavit_oracle as orc

pytestmark = pytest.mark.gpu

TV_BOUND = 1e-2  # test_attn_maps_gpu.py
SCALE = 64 ** -0.5
ERR_UNSUPPORTED = -3
G = 4096  # guard floats before and after a buffer


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
    """As test_channel_attention_gpu._qkv, including the spiked key."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = H * 64
    qkv = torch.randn(B, N, 3 * D, generator=g) * 1.5
    if prescaled:
        qkv[..., :D] *= SCALE * math.log2(math.e)  # q' = q scale log2(e), as the model's pre-scaled operand copies deliver it
    qkv = qkv.to(torch.bfloat16).cuda()
    if N > 1:  # one spiked key against one query: a late tile raises the row maximum
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


def _step(hip, qkv, lse, w, B, N, H, alpha, prescaled, out=None):
    out = torch.empty(B, N, device="cuda") if out is None else out
    hip.attn_rollout_step(qkv, lse, w, out, B, N, H, 64, SCALE, alpha, prescaled=prescaled)
    return out


def _step64(P, w, alpha):
    w = w.double()
    return alpha * w + (1 - alpha) * torch.einsum("bq,bqk->bk", w, P.mean(1))


def _weights(B, N, seed):
    """The query weights the kernel is tried on: random positive normalised; one-hot at 0 (the default start); one-hot at N - 1 (a clamped
    query row that leaked would double it); zero on the whole first 128 queries (N > 128: whole query tiles of zeros)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = torch.rand(B, N, generator=g) + 1e-3
    ws = {"random": rnd / rnd.sum(-1, keepdim=True)}
    for name, at in (("onehot0", 0), ("onehotlast", N - 1)):
        ws[name] = torch.zeros(B, N)
        ws[name][:, at] = 1.0
    if N > 128:
        z = rnd.clone()
        z[:, :128] = 0.0
        ws["zero128"] = z / z.sum(-1, keepdim=True)
    return {k: v.cuda() for k, v in ws.items()}


def _within(got, ref, sw):
    """max of |got - ref| / (3e-4 ref + 1e-6 sum(w)): the kernel bound holds when <= 1"""
    return ((got.double() - ref).abs() / (3e-4 * ref + 1e-6 * sw)).max().item()


SHAPES = [(2, 6, 1), (2, 6, 2), (1, 3, 33), (2, 6, 64), (2, 6, 65), (1, 3, 129), (2, 2, 197), (1, 12, 81), (1, 6, 257), (3, 1, 385)]


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
@pytest.mark.parametrize("B,H,N", SHAPES)
def test_kernel_against_float64(hip, B, H, N, prescaled):
    qkv = _qkv(B, N, H, seed=N + 7 * H, prescaled=prescaled)
    lse = _lse(hip, qkv, B, N, H, prescaled)
    P = _probs64(qkv, B, N, H, prescaled)
    worst, worst_sum = 0.0, 0.0
    for name, w in _weights(B, N, seed=N).items():
        sw = w.double().sum(-1, keepdim=True)
        for alpha in (0.5, 0.0, 0.9):
            out = _step(hip, qkv, lse, w, B, N, H, alpha, prescaled)
            assert out.shape == (B, N) and out.dtype == torch.float32
            wi = _within(out, _step64(P, w, alpha), sw)
            ds = ((out.double().sum(-1, keepdim=True) - sw).abs() / sw).max().item()
            worst, worst_sum = max(worst, wi), max(worst_sum, ds)
            assert wi <= 1, f"w {name} alpha {alpha}: max |got - ref| / (3e-4 ref + 1e-6 sum w) = {wi:.3g}"
            assert ds <= 1e-4, f"w {name} alpha {alpha}: |sum out - sum w| / sum w = {ds:.3g}"
    print(f"B{B} H{H} N{N} {'ps' if prescaled else 'plain'}: max err / bound {worst:.3f}; max |sum out - sum w| / sum w {worst_sum:.2e}")


def test_kernel_many_workgroups(hip):
    """Many more workgroups than CUs (600 against 256)."""
    B, H, N = 600, 2, 33
    qkv = _qkv(B, N, H, seed=600, prescaled=True)
    lse = _lse(hip, qkv, B, N, H, True)
    w = _weights(B, N, seed=5)["random"]
    out = _step(hip, qkv, lse, w, B, N, H, 0.5, True)
    wi = _within(out, _step64(_probs64(qkv, B, N, H, True), w, 0.5), w.double().sum(-1, keepdim=True))
    print(f"B{B} H{H} N{N}: max err / bound {wi:.3f}")
    assert wi <= 1


def _guarded(n):
    buf = torch.full((G + n + G,), float("nan"), device="cuda")
    return buf, buf[G:G + n]


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
def test_kernel_consistency(hip, prescaled):
    B, H, N = 2, 6, 197
    qkv = _qkv(B, N, H, seed=99, prescaled=prescaled)
    lse = _lse(hip, qkv, B, N, H, prescaled)
    w = _weights(B, N, seed=3)["random"]
    w0 = w.clone()
    out = _step(hip, qkv, lse, w, B, N, H, 0.5, prescaled)
    # two calls agree bit for bit; w is left alone
    assert torch.equal(_step(hip, qkv, lse, w, B, N, H, 0.5, prescaled), out)
    assert torch.equal(w, w0)
    # the kernel writes exactly out[b, k], k < N: a NaN-filled buffer with guard regions before and after.  There is no workspace — and nothing a
    # NaN-filled one could reach: the stream's shared workspace, whatever it holds, is not read
    hip._workspace(1, out).fill_(float("nan"))
    buf, inner = _guarded(B * N)
    _step(hip, qkv, lse, w, B, N, H, 0.5, prescaled, out=inner.view(B, N))
    torch.cuda.synchronize()
    assert torch.isfinite(inner).all() and torch.equal(inner.view(B, N), out)
    assert bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[G + B * N:]).all())
    # w = e_0: what is left after the identity's share is (1 - alpha) times the head mean of the CLS query's probabilities
    e0 = _weights(B, N, seed=3)["onehot0"]
    P0 = torch.empty(B, H, 1, N, device="cuda")
    hip.attn_probs(qkv, lse, P0, B, N, H, 64, SCALE, nq=1, prescaled=prescaled)
    for alpha in (0.5, 0.0, 0.9):
        got = _step(hip, qkv, lse, e0, B, N, H, alpha, prescaled).double() - alpha * e0.double()
        ref = (1 - alpha) * P0.double().mean(1)[:, 0]
        # against the float64 of the kernel's own probabilities: the head sum and the scaling are all that differ
        wi = ((got - ref).abs() / (3e-4 * ref + 1e-6)).max().item()
        print(f"alpha {alpha}: against attn_probs(nq=1), max err / bound {wi:.3g}")
        assert wi <= 1
    # refused, and nothing launched: out overlapping w
    lib = hip.load()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    big = torch.full((2 * B * N,), 0.25, device="cuda")
    for off in (0, 1, B * N - 1):
        rc = (lib.dcv_attn_rollout_step_ps(p(qkv), p(lse), p(big), p(big[off:]), B, N, H, 64, 0.5, st) if prescaled else
              lib.dcv_attn_rollout_step(p(qkv), p(lse), p(big), p(big[off:]), B, N, H, 64, SCALE, 0.5, st))
        assert rc == ERR_UNSUPPORTED, off
    with pytest.raises(RuntimeError, match="dcv_attn_rollout_step"):
        hip.attn_rollout_step(qkv, lse, w, w, B, N, H, 64, SCALE, 0.5, prescaled=prescaled)
    with pytest.raises(ValueError, match="attn_rollout_step"):
        hip.attn_rollout_step(qkv, lse, w[:1], out, B, N, H, 64, SCALE, 0.5, prescaled=prescaled)
    torch.cuda.synchronize()
    assert bool((big == 0.25).all()) and torch.equal(w, w0)


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
def test_twelve_chained_steps(hip, prescaled):
    B, H, N, L = 2, 6, 81, 12
    r = _weights(B, N, seed=1)["onehot0"]
    ref = r.double()
    nxt = torch.empty_like(r)
    for l in range(L):
        qkv = _qkv(B, N, H, seed=1000 + l, prescaled=prescaled)
        lse = _lse(hip, qkv, B, N, H, prescaled)
        _step(hip, qkv, lse, r, B, N, H, 0.5, prescaled, out=nxt)
        r, nxt = nxt, r
        ref = _step64(_probs64(qkv, B, N, H, prescaled), ref, 0.5)
    wi = ((r.double() - ref).abs() / (L * 3e-4 * ref + L * 1e-6)).max().item()
    print(f"{L} chained steps, {'ps' if prescaled else 'plain'}: max err / bound {wi:.1e}; sum {r.double().sum(-1).tolist()}")
    assert wi <= 1


# ------------------------------------------------------------------------------------------------------------------------------------
def _build(case, device, **cfg_over):
    import diverse_channel_vit_amd as dcv
    cfg = Cfg(dict(case["cfg"], **cfg_over), in_channel_names=[f"c{i}" for i in range(case["n_channels"])], img_size=[case["img"]],
              num_classes=case["num_classes"])
    model = dcv.dichavit(cfg, mapper={k: list(v) for k, v in case["mapper"].items()})
    st = orc.make_state(orc.state_shapes(case["cfg"], case["n_channels"], case["img"], case["num_classes"]), case["seed"])
    D = model.dim
    for k in st:
        if k.endswith("attn.qkv.weight"):
            st[k] = st[k].clone()
            st[k][:2 * D] *= case["qk_mult"]  # the fixture's sharpened maps (make_golden_attn.py)
    model.load_state_dict({**st, "adaptive_interface.0": st["proxies"]}, strict=True)
    return model.to(device).eval()


def _batch(case, device):
    x, _ = orc.make_batch(case["batch_seed"], case["B"], len(case["mapper"][case["chunk"]]), case["img_in"], case["num_classes"])
    return x.to(device)


@pytest.fixture(scope="module")
def rolled(gpu_device):
    """Per fixture case: the model's rollout for every start layer, and its own twelve get_last_selfattention maps.  Computed once."""
    meta, a = load_golden("attn_rollout")
    res = {}
    for case in meta["cases"]:
        model = _build(case, gpu_device)
        fe = model.feature_extractor
        x = _batch(case, gpu_device)
        L = len(fe.blocks)
        maps = [fe.get_last_selfattention(x, chunk=case["chunk"], layer_idx=i) for i in range(L)]
        got = [fe.get_attention_rollout(x, chunk=case["chunk"], start_layer=s) for s in range(L)]
        g = torch.Generator(device="cpu").manual_seed(case["seed"])
        start = torch.rand(case["B"], case["N"], generator=g).to(gpu_device)
        start[:, 3] = 0.0
        extra = dict(quarter=fe.get_attention_rollout(x, chunk=case["chunk"], residual=0.25),
                     start=fe.get_attention_rollout(x, chunk=case["chunk"], start_layer=4, start=start),
                     neg=fe.get_attention_rollout(x, chunk=case["chunk"], start_layer=-1))
        res[case["name"]] = dict(case=case, L=L, maps=maps, got=got, ref=torch.from_numpy(a[f"{case['name']}/rollout"]), start=start, extra=extra,
                                 device=x.device)
        del model
    return res


def _within_model(got, ref, steps):
    return ((got.double() - ref).abs() / (steps * 6e-4 * ref + steps * 2e-6)).max().item()


def test_model_against_its_own_maps(rolled):
    for name, d in rolled.items():
        L, case = d["L"], d["case"]
        ratios = []
        for s in range(L):
            got = d["got"][s]
            assert got.dtype == torch.float32 and tuple(got.shape) == (case["B"], case["N"]) and got.device == d["device"] and not got.requires_grad
            wi = _within_model(got, rollout(d["maps"], s, 0.5), L - s)
            ratios.append(wi)
            assert (got.double().sum(-1) - 1).abs().max().item() <= (L - s) * 1e-4
        print(f"{name}: against the float64 rollout of the model's own maps, max err / bound per start layer: {[f'{r:.1e}' for r in ratios]}")
        assert max(ratios) <= 1, (name, ratios)
        wq = _within_model(d["extra"]["quarter"], rollout(d["maps"], 0, 0.25), L)
        ws = _within_model(d["extra"]["start"], rollout(d["maps"], 4, 0.5, d["start"]), L - 4)
        print(f"{name}: residual 0.25: {wq:.1e}; random start from layer 4: {ws:.1e}")
        assert wq <= 1 and ws <= 1
        assert (d["extra"]["start"].double().sum(-1) - d["start"].double().sum(-1)).abs().max().item() <= (L - 4) * 1e-4 * d["start"].sum(-1).max().item()
        assert torch.equal(d["extra"]["neg"], d["got"][L - 1])  # start_layer=-1 is start_layer=11


def test_model_against_the_reference(rolled):
    for name, d in rolled.items():
        L = d["L"]
        tvs = [tv(d["got"][s], d["ref"][s]) for s in range(L)]
        print(f"{name}: total variation against the reference's rollout per start layer: {[f'{t:.2e}' for t in tvs]}")
        for s in range(L):
            # the ceiling grows with the blocks rolled while the rollout itself flattens: it discriminates only at high s (s = 11: 5e-3 against a
            # distance of 0.5 to the full rollout); s = 0 is carried by test_model_against_its_own_maps
            assert tvs[s] <= (1 - 0.5) * (L - s) * TV_BOUND, (name, s, tvs[s])
        # it does discriminate there: another start layer's answer is far outside the ceiling
        assert tv(d["got"][L - 1], d["ref"][L - 2]) > 10 * 0.5 * TV_BOUND


def test_train_mode_hcs_and_token_drop(gpu_device):
    meta, _ = load_golden("attn_rollout")
    case = meta["cases"][0]
    x = _batch(case, gpu_device)
    # HCS in train mode with a pinned sampler: 3 of the 5 channels
    model = _build(case, gpu_device, enable_sample=True).train()
    picked = [3, 0, 4]
    model.hcs_sampler = lambda m, chunk, cur, picked=picked: (picked, [cur.index(c) for c in picked])
    r = model.feature_extractor.get_attention_rollout(x, chunk="train")
    assert tuple(r.shape) == (case["B"], 1 + 3 * 16) and (r.double().sum(-1) - 1).abs().max().item() <= 12e-4 and (r >= 0).all()
    del model
    # token drop: N is the tokens this forward saw
    model = _build(case, gpu_device, dropout_tokens_hcs="channel_random50").train()  # keeps ceil(5 / 2) = 3 whole channels
    fe = model.feature_extractor
    random.seed(5)
    r = fe.get_attention_rollout(x, chunk="train")
    assert tuple(r.shape) == (case["B"], 1 + 3 * 16)
    assert (r.double().sum(-1) - 1).abs().max().item() <= 12e-4 and (r >= 0).all()
    model.eval()  # eval ignores the option
    assert tuple(fe.get_attention_rollout(x, chunk="train").shape) == (case["B"], case["N"])
    del model
    # both: ceil(3 / 2) = 2 of the 3 sampled channels stay
    model = _build(case, gpu_device, enable_sample=True, dropout_tokens_hcs="channel_random50").train()
    model.hcs_sampler = lambda m, chunk, cur, picked=picked: (picked, [cur.index(c) for c in picked])
    r = model.feature_extractor.get_attention_rollout(x, chunk="train")
    assert tuple(r.shape) == (case["B"], 1 + 2 * 16) and (r.double().sum(-1) - 1).abs().max().item() <= 12e-4 and (r >= 0).all()


def test_input_affine_with_uint8_input(gpu_device):
    meta, _ = load_golden("attn_rollout")
    case = meta["cases"][0]
    model = _build(case, gpu_device)
    fe = model.feature_extractor
    g = torch.Generator(device="cpu").manual_seed(11)
    xu = torch.randint(0, 256, (case["B"], 5, 32, 32), generator=g, dtype=torch.uint8).to(gpu_device)
    mean, std = [0.4, 0.5, 0.45, 0.55, 0.5], [0.2, 0.25, 0.3, 0.22, 0.27]
    with pytest.raises(ValueError, match="set_input_normalisation"):
        fe.get_attention_rollout(xu, chunk="train")  # as forward(): raw pixels need the affine
    model.set_input_normalisation(mean, std)
    got = fe.get_attention_rollout(xu, chunk="train", start_layer=8)
    maps = [fe.get_last_selfattention(xu, chunk="train", layer_idx=i) for i in range(12)]
    wi = _within_model(got, rollout(maps, 8, 0.5), 4)
    print(f"uint8 input through the input affine: max err / bound {wi:.1e}")
    assert wi <= 1
    # the affine is applied: a model without it, fed the normalised float images, sees the same tokens up to the rounding of the affine
    m, s = (torch.tensor(v, device=gpu_device).view(1, 5, 1, 1) for v in (mean, std))
    plain = _build(case, gpu_device)  # (held: the encoder runs through its owner)
    same = plain.feature_extractor.get_attention_rollout((xu.float() / 255.0 - m) / s, chunk="train", start_layer=8)
    print(f"    total variation against the normalised float input: {tv(got, same):.2e}")
    assert tv(got, same) <= (1 - 0.5) * 4 * TV_BOUND  # the ceiling the reference comparison holds for four blocks rolled


def test_bad_arguments_raise(gpu_device):
    meta, _ = load_golden("attn_rollout")
    case = meta["cases"][0]
    model = _build(case, gpu_device)
    fe = model.feature_extractor
    x = _batch(case, gpu_device)
    B, N = case["B"], case["N"]
    with pytest.raises(ValueError, match="residual"):
        fe.get_attention_rollout(x, chunk="train", residual=1.0)
    with pytest.raises(ValueError, match="start_layer"):
        fe.get_attention_rollout(x, chunk="train", start_layer=12)
    ok = torch.rand(B, N, device=gpu_device)
    for bad in (ok[:, :-1].contiguous(), ok[:1], ok.view(-1), ok.double(), ok.half(), ok.cpu(), -ok, torch.full_like(ok, float("nan"))):
        with pytest.raises(ValueError, match="start"):
            fe.get_attention_rollout(x, chunk="train", start=bad)
    neg = ok.clone()
    neg[1, N - 1] = -1e-6
    with pytest.raises(ValueError, match="start"):
        fe.get_attention_rollout(x, chunk="train", start=neg)
    with pytest.raises(KeyError):
        fe.get_attention_rollout(x)  # as get_last_selfattention: the default chunk "" is no mapper key
    before = ok.clone()
    assert tuple(fe.get_attention_rollout(x, chunk="train", start=ok).shape) == (B, N) and torch.equal(ok, before)  # start is not written


def test_probe_leaves_the_training_step_alone(gpu_device):
    """A rollout between loss = ... and loss.backward() must not touch what the backward reads (the stochastically rounded operand copies,
    the pre-scaled q bias, the rounding seed): gradients and the next step's loss are bit-identical to the same sequence without it."""
    from diverse_channel_vit_amd import hip
    from diverse_channel_vit_amd.optim import HipAdamW
    assert hip.is_deterministic()
    meta, _ = load_golden("attn_rollout")
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
            got = model.feature_extractor.get_attention_rollout(x, chunk=case["chunk"])
            assert torch.isfinite(got).all()
            model.train()
        loss.backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        opt.step()
        opt.zero_grad(set_to_none=True)
        params = {n: p.detach().clone() for n, p in model.named_parameters()}
        out2, extra2 = model(x, case["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss2 = torch.nn.functional.cross_entropy(out2, y) + extra2
        loss2.backward()
        grads2 = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        runs.append((loss.detach().clone(), grads, params, loss2.detach().clone(), grads2))
        del model, opt
    (l0, g0, p0, m0, h0), (l1, g1, p1, m1, h1) = runs
    assert torch.equal(l0, l1) and g0.keys() == g1.keys() and len(g0) > 100
    assert not [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not [n for n in p0 if not torch.equal(p0[n], p1[n])]
    assert torch.equal(m0, m1)
    assert not [n for n in h0 if not torch.equal(h0[n], h1[n])]


def test_deepcopy_runs_on_the_copys_weights(gpu_device):
    meta, _ = load_golden("attn_rollout")
    case = meta["cases"][0]
    model = _build(case, gpu_device)
    x = _batch(case, gpu_device)
    r0 = model.feature_extractor.get_attention_rollout(x, chunk=case["chunk"], start_layer=-1)
    cp = copy.deepcopy(model)
    assert torch.equal(cp.feature_extractor.get_attention_rollout(x, chunk=case["chunk"], start_layer=-1), r0)
    with torch.no_grad():
        cp.feature_extractor.blocks[11].attn.qkv.weight.mul_(1.5)
    assert tv(cp.feature_extractor.get_attention_rollout(x, chunk=case["chunk"], start_layer=-1), r0) > 1e-4
    assert torch.equal(model.feature_extractor.get_attention_rollout(x, chunk=case["chunk"], start_layer=-1), r0)
