"""get_attention_relevance on the MI355X: the relevance-step kernel (dcv_attn_relevance_step / _ps) against its float64 restatement on random
bf16 operands, bit for bit on exact operands, with poisoned gradient rows, its structure; the model method against the relevance of the real
reference's maps and gradients (tests/golden/attn_relevance.npz: both recorded targets, every start layer) and its own invariants.

Bounds.  Kernel: |got - ref| <= 3e-4 mag + 1e-6 sum(w) max|dO| max|V| 64, ref and mag from tests/attention_relevance_ref.relevance_step_ref on the
same bf16 q, k, v, dO: mag[k] = w[k] + 1/H sum sum w_q p_qk sum_d |dO_qd V_kd| is the absolute-value companion of out, which bounds every partial
sum on either side of relu's kink (max(x, 0) is 1-Lipschitz, so an error of G passes through it undiminished at most); 3e-4 is the rollout
kernel's own relative bound for the same p, and G itself is an fp32 sum of 64 exact products, in error by at most 64 2^-24 of its companion.
Model against the fixture: total variation of the normalised patch relevance r[:, 1:] / sum <= 3 x the distance `emu_tv` the fixture records
for a float64 run of the reference whose Linear operands and outputs are rounded to bf16; |r[:, 0] - ref| and |sum r[:, 1:] - ref| within the
same 3 x emu_tv, relative.  The margin of 3 is over an emulation that rounds the forward only: the GPU also rounds dO and the backward GEMMs'
operands to bf16 and sums in another order.  The model tests print every figure before asserting.
Measured on the MI355X (the tests print these): kernel, worst case over the ten seams, three Nq, four (B, H), three kinds of w and both forms,
max |got - ref| / bound = 0.001 (0.002 at 66 000 workgroups, below 0.0005 at N = 1569); exact operands, poisoned rows and the rerun: bit for bit.
Model against the fixture, tv over the twelve start layers and both targets / bound: small 4.4e-3 .. 1.0e-2 / 4.1e-2, sub 4.7e-3 .. 1.0e-2 /
2.3e-2, tiny48 2.0e-3 .. 3.2e-3 / 9.9e-3, base 1.1e-3 .. 2.9e-3 / 9.3e-3; r[:, 0] within 1.6e-4 relative, sum r[:, 1:] within 9.6e-3 (sub),
3.7e-3, 2.0e-3 and 1.2e-3.  cls_only_tail off against on: bit-identical at start layers 0 and 11.  uint8 input against the normalised float
input: tv 4.8e-3.  The bounds are the ones reasoned above, not tightened to these."""
import copy
import ctypes as C
import math
import random

import pytest
import torch

from attention_relevance_ref import normalised_patches, relevance_step_ref, tv
from conftest import load_golden
from oracle import dichavit_oracle as orc

pytestmark = pytest.mark.gpu

SCALE = 64 ** -0.5
ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -3  # include/dcv.h
G = 4096  # guard floats before and after a buffer
FACTOR = 3.0  # over the fixture's emulation distance


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


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------------------------------------------
def _operands(B, N, H, seed, prescaled):
    """qkv [B, N, 3 H 64] bf16 with one spiked key (a late tile raises the row maximum) and dO [B, N, H 64] bf16, on the device."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = H * 64
    qkv = torch.randn(B, N, 3 * D, generator=g) * 1.5
    if prescaled:
        qkv[..., :D] *= SCALE * math.log2(math.e)
    qkv = qkv.to(torch.bfloat16).cuda()
    if N > 1:
        qkv[0, N // 2, :64] *= 4
        qkv[0, N - 1, D:D + 64] = qkv[0, N // 2, :64]
    dO = (torch.randn(B, N, D, generator=g) * 0.5).to(torch.bfloat16).cuda()
    return qkv, dO


def _heads(qkv, dO, B, N, H):
    t = qkv.view(B, N, 3, H, 64)
    return tuple(t[:, :, i].transpose(1, 2) for i in range(3)) + (dO.view(B, N, H, 64).transpose(1, 2),)


def _lse(hip, qkv, B, N, H, prescaled):
    o = torch.empty(B, N, H * 64, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, N, device="cuda")
    hip.attn_fwd(qkv, o, lse, B, N, H, 64, SCALE, prescaled=prescaled)
    return lse


def _step(hip, qkv, lse, dO, w, B, N, H, nq, prescaled, out=None):
    out = torch.empty(B, N, device="cuda") if out is None else out
    hip.attn_relevance_step(qkv, lse, dO, w, out, B, N, H, 64, SCALE, nq=nq, prescaled=prescaled)
    return out


def _weights(B, N, seed):
    """one-hot at CLS (the default start); dense random; random with exact zeros (a third of the rows, and the whole first 64-query tile when
    there is a second one)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    dense = torch.rand(B, N, generator=g) + 1e-3
    onehot = torch.zeros(B, N)
    onehot[:, 0] = 1.0
    zeros = dense.clone()
    zeros[torch.rand(B, N, generator=g) < 1 / 3] = 0.0
    if N > 64:
        zeros[:, :64] = 0.0
    if N > 1:
        zeros[:, N - 1] = dense[:, N - 1]  # never all zero
    return {"onehot": onehot.cuda(), "dense": dense.cuda(), "zeros": zeros.cuda()}


def _ratio(got, qkv, dO, w, B, N, H, nq, prescaled):
    """max of |got - ref| / (3e-4 mag + 1e-6 sum(w) max|dO| max|V| 64): the kernel bound holds when <= 1"""
    q, k, v, g = _heads(qkv, dO, B, N, H)
    ref, mag = relevance_step_ref(q, k, v, g, w, nq, math.log(2.0) if prescaled else SCALE, magnitude=True)
    floor = 1e-6 * w.double().sum(-1, keepdim=True) * float(dO.abs().max()) * float(v.abs().max()) * 64
    err = (got.double() - ref).abs()
    return torch.where(err == 0, err, err / (3e-4 * mag + floor)).max().item()  # an all-zero w has a bound of 0, met by equality alone


SEAMS = [1, 33, 63, 64, 65, 127, 128, 129, 193, 257]


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
@pytest.mark.parametrize("N", SEAMS)
def test_kernel_against_float64(hip, N, prescaled):
    """Every N on the seams of the 64-query tile, its 32-row halves, the 32-key wave and the 128-key workgroup; per N, (B, H) runs through
    (1, 1), (3, 3), (1, 6), (3, 6) and Nq through 1, 33 and N; three kinds of w."""
    worst = 0.0
    for B, H in ((1, 1), (3, 3), (1, 6), (3, 6)):
        qkv, dO = _operands(B, N, H, seed=N + 7 * H + B, prescaled=prescaled)
        lse = _lse(hip, qkv, B, N, H, prescaled)
        for nq in sorted({1, min(33, N), N}):
            for name, w in _weights(B, N, seed=N + nq).items():
                out = _step(hip, qkv, lse, dO, w, B, N, H, nq, prescaled)
                assert out.shape == (B, N) and out.dtype == torch.float32
                r = _ratio(out, qkv, dO, w, B, N, H, nq, prescaled)
                worst = max(worst, r)
                assert r <= 1, f"B{B} H{H} N{N} Nq{nq} w {name}: max |got - ref| / bound = {r:.3g}"
                assert (out >= w).all()
    print(f"N{N} {'ps' if prescaled else 'plain'}: max err / bound {worst:.3f}")


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
def test_kernel_at_the_headline_token_count(hip, prescaled):
    B, H, N = 2, 6, 1569
    qkv, dO = _operands(B, N, H, seed=1569, prescaled=prescaled)
    lse = _lse(hip, qkv, B, N, H, prescaled)
    for nq, kind in ((N, "dense"), (N, "zeros"), (1, "onehot")):
        w = _weights(B, N, seed=9)[kind]
        r = _ratio(_step(hip, qkv, lse, dO, w, B, N, H, nq, prescaled), qkv, dO, w, B, N, H, nq, prescaled)
        print(f"B{B} H{H} N{N} Nq{nq} w {kind} {'ps' if prescaled else 'plain'}: max err / bound {r:.3f}")
        assert r <= 1


def test_kernel_many_workgroups(hip):
    """B ceil(N / 128) above 65 535 workgroups in one launch."""
    B, H, N = 66000, 1, 2
    qkv, dO = _operands(B, N, H, seed=600, prescaled=True)
    lse = _lse(hip, qkv, B, N, H, True)
    w = _weights(B, N, seed=5)["dense"]
    out = _step(hip, qkv, lse, dO, w, B, N, H, N, True)
    r = _ratio(out, qkv, dO, w, B, N, H, N, True)
    print(f"B{B} H{H} N{N}: max err / bound {r:.3f}")
    assert r <= 1


def _exact(B, N, H, nq, seed):
    """q = 0 and lse = 0: every p is exp2(0) = 1 and w_q p_qk = w_q for dyadic w; dO and V small integers: G is an integer of at most 256 in
    magnitude, every product w_q max(G, 0) a multiple of 1/4 and every partial sum below 2^22: exact in fp32 in any order.  Returns the
    operands and the float32 the kernel must produce: fma(fl(1 / H), sum, w) rounded once."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = H * 64
    qkv = torch.zeros(B, N, 3, H, 64)
    qkv[:, :, 1] = torch.randn(B, N, H, 64, generator=g)  # k: multiplied by q = 0
    qkv[:, :, 2] = torch.randint(-2, 3, (B, N, H, 64), generator=g).float()
    dO = torch.randint(-2, 3, (B, N, H, 64), generator=g).float()
    w = torch.tensor([0.0, 0.25, 0.5, 1.0, 2.0])[torch.randint(0, 5, (B, N), generator=g)]
    lse = torch.zeros(B, H, N)
    Gm = torch.einsum("bqhd,bkhd->bhqk", dO.double(), qkv[:, :, 2].double()).clamp(min=0)[:, :, :nq]
    tot = torch.einsum("bq,bhqk->bk", w.double()[:, :nq], Gm)
    beta = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H), dtype=torch.float32)
    want = (beta.double() * tot + w.double()).float()  # both the product and the sum are exact in float64: one rounding, as the fma's
    return qkv.view(B, N, 3 * D).to(torch.bfloat16).cuda(), lse.cuda(), dO.view(B, N, D).to(torch.bfloat16).cuda(), w.cuda(), want.cuda()


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
@pytest.mark.parametrize("N", SEAMS)
def test_kernel_bit_for_bit_on_exact_operands(hip, N, prescaled):
    for B, H in ((1, 1), (2, 3), (2, 6)):
        for nq in sorted({1, min(33, N), N}):
            qkv, lse, dO, w, want = _exact(B, N, H, nq, seed=3 * N + H + nq)
            buf = torch.full((G + B * N + G,), float("nan"), device="cuda")
            out = _step(hip, qkv, lse, dO, w, B, N, H, nq, prescaled, out=buf[G:G + B * N].view(B, N))
            bad = (out != want).nonzero()
            assert bad.numel() == 0, f"B{B} H{H} N{N} Nq{nq}: {bad.shape[0]} elements differ, first {bad[0].tolist()}: {out[tuple(bad[0])].item()} " \
                                     f"against {want[tuple(bad[0])].item()}"
            assert bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[G + B * N:]).all())  # nothing but out[b, k], k < N, is written


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
@pytest.mark.parametrize("N,nq", [(65, 1), (65, 33), (129, 64), (193, 65), (257, 129)])
def test_rows_past_nq_never_reach_a_result(hip, N, nq, prescaled):
    """dO rows at or past Nq hold NaN — the state of the CLS-only last block's buffer — and so do lse and w there; q rows there hold Inf.  The
    output is bit-identical to the run with those rows zeroed.  Data, not a fault: every row read lies inside the buffers."""
    B, H = 2, 3
    qkv, dO = _operands(B, N, H, seed=N + nq, prescaled=prescaled)
    lse = _lse(hip, qkv, B, N, H, prescaled)
    w = _weights(B, N, seed=N)["dense"]
    clean_dO, clean_lse, clean_w, clean_qkv = dO.clone(), lse.clone(), w.clone(), qkv.clone()  # w[k] is also out[k]'s identity term: kept
    clean_dO[:, nq:] = 0
    clean_lse[:, :, nq:] = 0
    clean_qkv[:, nq:, :H * 64] = 0
    want = _step(hip, clean_qkv, clean_lse, clean_dO, clean_w, B, N, H, nq, prescaled)
    dO[:, nq:] = float("nan")
    lse[:, :, nq:] = float("nan")
    qkv[:, nq:, :H * 64] = float("inf")
    got = _step(hip, qkv, lse, dO, w, B, N, H, nq, prescaled)  # w past nq: whatever it holds, finite here
    assert torch.isfinite(got).all() and torch.equal(got, want)
    w[:, nq:] = float("nan")
    got = _step(hip, qkv, lse, dO, w, B, N, H, nq, prescaled)
    # out[k] = w[k] + ...: the identity term reads w at the KEY, so keys past nq carry their own NaN and nothing else does
    assert torch.equal(got[:, :nq], want[:, :nq]) and bool(torch.isnan(got[:, nq:]).all())
    r = _ratio(want, clean_qkv, clean_dO, clean_w, B, N, H, nq, prescaled)
    assert r <= 1, r


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
@pytest.mark.parametrize("N", [33, 129, 257])
def test_a_weight_of_zero_contributes_exactly_nothing(hip, N, prescaled):
    """dO rows whose weight is 0 hold NaN, +Inf and -Inf: bit-identical to the run with those rows zeroed."""
    B, H = 2, 6
    qkv, dO = _operands(B, N, H, seed=N, prescaled=prescaled)
    lse = _lse(hip, qkv, B, N, H, prescaled)
    w = _weights(B, N, seed=N + 1)["zeros"]
    dead = (w == 0)
    assert dead.any() and not dead.all()
    clean = dO.clone()
    clean[dead] = 0
    want = _step(hip, qkv, lse, clean, w, B, N, H, N, prescaled)
    fill = torch.tensor([float("nan"), float("inf"), float("-inf")], device="cuda")[torch.arange(H * 64, device="cuda") % 3].to(torch.bfloat16)
    dO[dead] = fill
    got = _step(hip, qkv, lse, dO, w, B, N, H, N, prescaled)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert _ratio(want, qkv, clean, w, B, N, H, N, prescaled) <= 1


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
def test_kernel_structure(hip, prescaled):
    B, H, N = 2, 6, 197
    qkv, dO = _operands(B, N, H, seed=99, prescaled=prescaled)
    lse = _lse(hip, qkv, B, N, H, prescaled)
    w = _weights(B, N, seed=3)["dense"]
    w0, dO0 = w.clone(), dO.clone()
    out = _step(hip, qkv, lse, dO, w, B, N, H, N, prescaled)
    # two calls agree bit for bit; the inputs are left alone
    assert torch.equal(_step(hip, qkv, lse, dO, w, B, N, H, N, prescaled), out)
    assert torch.equal(w, w0) and torch.equal(dO, dO0)
    # out[b, k] does not depend on which other keys are computed, nor on the images beside it: the second image alone
    alone = _step(hip, qkv[1:].contiguous(), lse[1:].contiguous(), dO[1:].contiguous(), w[1:].contiguous(), 1, N, H, N, prescaled)
    assert torch.equal(alone[0], out[1])
    # refused, and nothing launched
    lib = hip.load()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(qkv_, lse_, dO_, w_, out_, nq=N, hd=64):
        if prescaled:
            return lib.dcv_attn_relevance_step_ps(p(qkv_), p(lse_), p(dO_), p(w_), p(out_), B, N, nq, H, hd, st)
        return lib.dcv_attn_relevance_step(p(qkv_), p(lse_), p(dO_), p(w_), p(out_), B, N, nq, H, hd, SCALE, st)

    big = torch.full((2 * B * N,), 0.25, device="cuda")
    for off in (0, 1, B * N - 1):
        assert raw(qkv, lse, dO, big, big[off:]) == ERR_UNSUPPORTED, off
    sink = torch.full((B * N + 8,), 0.25, device="cuda")
    assert raw(qkv, lse, dO, w, sink, hd=32) == ERR_UNSUPPORTED
    assert raw(qkv, lse, dO, w, sink, nq=0) == ERR_SHAPE and raw(qkv, lse, dO, w, sink, nq=N + 1) == ERR_SHAPE
    pad = torch.zeros(dO.numel() + 8, dtype=torch.bfloat16, device="cuda")
    assert raw(qkv, lse, pad[1:], w, sink) == ERR_ALIGN  # dO two bytes off a 16-byte boundary
    qpad = torch.zeros(qkv.numel() + 8, dtype=torch.bfloat16, device="cuda")
    assert raw(qpad[4:], lse, dO, w, sink) == ERR_ALIGN
    bytes_ = torch.zeros(4 * B * N + 8, dtype=torch.uint8, device="cuda")
    assert raw(qkv, lse, dO, w, bytes_[1:]) == ERR_ALIGN
    with pytest.raises(RuntimeError, match="dcv_attn_relevance_step"):
        hip.attn_relevance_step(qkv, lse, dO, w, w, B, N, H, 64, SCALE, prescaled=prescaled)
    with pytest.raises(ValueError, match="attn_relevance_step"):
        hip.attn_relevance_step(qkv, lse, dO[:1], w, out, B, N, H, 64, SCALE, prescaled=prescaled)
    torch.cuda.synchronize()
    assert bool((big == 0.25).all()) and bool((sink == 0.25).all()) and torch.equal(w, w0)


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "ps"])
@pytest.mark.parametrize("B,H,N", [(2, 3, 197), (1, 2, 65), (1, 6, 129)])
def test_unit_gradients_give_the_rollout_step_bit_for_bit(hip, B, H, N, prescaled):
    """dO[b, q, h, 0] = 1 and V[b, k, h, 0] = 1, every other dO element 0: G = dO V^T is exactly 1 for every (q, k), so each relevance term
    p max(G, 0) is p itself, and a row of weight 0 adds the +0 that the rollout's exp2(-inf) adds.  Both steps then form the same tot in the
    same order, and with the rollout's alpha = 0 both store fl(fl(1 / H) tot) at a key whose own weight is 0.  Two weight vectors, zero on the
    odd and on the even tokens, cover every key.  (2, 3, 197): four query tiles, two key workgroups, a ragged tail; (1, 2, 65): a second tile of
    one row, an idle wave, the skipped second query block; (1, 6, 129): the second key workgroup owns a single key."""
    qkv, _ = _operands(B, N, H, seed=N + H, prescaled=prescaled)
    lse = _lse(hip, qkv, B, N, H, prescaled)  # of q and k alone
    qkv.view(B, N, 3, H, 64)[:, :, 2, :, 0] = 1
    dO = torch.zeros(B, N, H, 64, dtype=torch.bfloat16, device="cuda")
    dO[..., 0] = 1
    dO = dO.view(B, N, H * 64)
    dense = (torch.rand(B, N, generator=torch.Generator(device="cpu").manual_seed(N)) + 1e-3).cuda()
    odd = (torch.arange(N, device="cuda") % 2 == 1)
    for dead in (odd, ~odd):
        w = torch.where(dead, torch.zeros_like(dense), dense)
        rel = _step(hip, qkv, lse, dO, w, B, N, H, N, prescaled)
        roll = torch.empty(B, N, device="cuda")
        hip.attn_rollout_step(qkv, lse, w, roll, B, N, H, 64, SCALE, 0.0, prescaled=prescaled)
        assert bool((roll[:, dead] > 0).all())  # the live rows reach every key: the comparison is of sums, not of zeros
        assert torch.equal(rel[:, dead], roll[:, dead])


# ------------------------------------------------------------------------------------------------------------------------------------
# the model
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
def explained(gpu_device):
    """Per fixture case: the model's relevance for both recorded targets and every start layer.  Computed once."""
    meta, a = load_golden("attn_relevance")
    res = {}
    for case in meta["cases"]:
        model = _build(case, gpu_device)
        x = _batch(case, gpu_device)
        L = case["depth"]
        targets = torch.tensor(case["targets"], device=gpu_device)
        got = [[model.get_attention_relevance(x, targets[ti], chunk=case["chunk"], start_layer=s) for s in range(L)] for ti in range(2)]
        res[case["name"]] = dict(case=case, L=L, got=got, ref=torch.from_numpy(a[f"{case['name']}/relevance"]), device=x.device,
                                 targets=targets)
        del model
    return res


def _distances(got, ref):
    """(tv of the normalised patch relevance, relative error of r[:, 0], relative error of sum r[:, 1:]) of a [B, N] pair"""
    ref = ref.double().to(got.device)
    got = got.double()
    s_got, s_ref = got[:, 1:].sum(-1), ref[:, 1:].sum(-1)
    return (tv(normalised_patches(got), normalised_patches(ref)), ((got[:, 0] - ref[:, 0]).abs() / ref[:, 0]).max().item(),
            ((s_got - s_ref).abs() / s_ref).max().item())


def test_model_against_the_reference(explained):
    failures = []
    for name, d in explained.items():
        case, L = d["case"], d["L"]
        bound = FACTOR * case["emu_tv"]
        for ti in range(2):
            dist = [_distances(d["got"][ti][s], d["ref"][ti, s]) for s in range(L)]
            print(f"{name} target {ti} (bound {bound:.2e}): tv per start layer {[f'{t[0]:.1e}' for t in dist]}; r[:,0] rel "
                  f"{max(t[1] for t in dist):.1e}; sum r[:,1:] rel {[f'{t[2]:.1e}' for t in dist]}")
            for s in range(L):
                got = d["got"][ti][s]
                assert got.dtype == torch.float32 and tuple(got.shape) == (case["B"], case["N"]) and got.device == d["device"]
                assert not got.requires_grad and bool((got >= 0).all()) and bool((got[:, 0] >= 1).all())
                if max(dist[s]) > bound:
                    failures.append((name, ti, s, dist[s], bound))
        for s in range(L):
            # a call that ignored `target` would be this far off: target 0's answer against the fixture's target 1
            other = tv(normalised_patches(d["got"][0][s]), normalised_patches(d["ref"][1, s]))
            assert other > bound, (name, s, other, bound)
    assert not failures, failures


def test_model_invariants(gpu_device, explained):
    d = explained["small"]
    case = d["case"]
    x = _batch(case, gpu_device)
    model = _build(case, gpu_device)
    fe = model.feature_extractor
    t0 = d["targets"][0]
    base = d["got"][0]
    # deterministic: a second model, a second call
    assert torch.equal(model.get_attention_relevance(x, t0, chunk=case["chunk"]), base[0])
    assert torch.equal(model.get_attention_relevance(x, t0, chunk=case["chunk"], start_layer=-3), base[9])
    # a float target equal to the head's weight rows is the integer target, bit for bit; so is the encoder's twin
    rows = model.classifer_head.weight.detach()[t0].contiguous()
    assert torch.equal(model.get_attention_relevance(x, rows, chunk=case["chunk"]), base[0])
    assert torch.equal(fe.get_attention_relevance(x, rows, chunk=case["chunk"], start_layer=5), base[5])
    assert torch.equal(model.get_attention_relevance(x, t0.int(), chunk=case["chunk"]), base[0])
    # the default target is the argmax of this call's own logits
    top = model(x, case["chunk"]).argmax(1)
    print(f"the GPU's top classes {top.tolist()}, the reference's {t0.tolist()}")
    assert torch.equal(model.get_attention_relevance(x, chunk=case["chunk"], start_layer=7),
                       model.get_attention_relevance(x, top, chunk=case["chunk"], start_layer=7))
    # start= one-hot CLS is the default
    e0 = torch.zeros(case["B"], case["N"], device=gpu_device)
    e0[:, 0] = 1
    assert torch.equal(model.get_attention_relevance(x, t0, chunk=case["chunk"], start=e0), base[0])
    assert e0.sum().item() == case["B"] and bool((e0[:, 0] == 1).all())  # start is not written
    # linear in start
    two = model.get_attention_relevance(x, t0, chunk=case["chunk"], start=2 * e0, start_layer=6)
    assert torch.allclose(two, 2 * base[6], rtol=1e-5, atol=0)
    # the CLS-only tail off: every row of the last block computed, Nq = N in its step.  The rows the tail skips have an exactly zero gradient
    # in exact arithmetic; here they carry the backward's own rounding, so the two agree within the kernel bound per block rolled
    # (3e-4 relative of a non-negative sum, 1e-6 absolute)
    model.cls_only_tail = False
    full = [model.get_attention_relevance(x, t0, chunk=case["chunk"], start_layer=s) for s in (0, 11)]
    model.cls_only_tail = True
    for s, f in zip((0, 11), full):
        dist = _distances(f, base[s])
        print(f"cls_only_tail off against on, start_layer {s}: tv {dist[0]:.2e}, r[:,0] rel {dist[1]:.2e}, sum rel {dist[2]:.2e}")
        err = ((f.double() - base[s].double()).abs() / ((12 - s) * (3e-4 * base[s].double() + 1e-6))).max().item()
        print(f"    element by element against (12 - s) (3e-4 relative + 1e-6): {err:.3g}")
        assert err <= 1


def test_input_affine_with_uint8_input(gpu_device):
    meta, _ = load_golden("attn_relevance")
    case = meta["cases"][0]
    model = _build(case, gpu_device)
    g = torch.Generator(device="cpu").manual_seed(11)
    xu = torch.randint(0, 256, (case["B"], 5, 32, 32), generator=g, dtype=torch.uint8).to(gpu_device)
    mean, std = [0.4, 0.5, 0.45, 0.55, 0.5], [0.2, 0.25, 0.3, 0.22, 0.27]
    t = torch.tensor([1, 4], device=gpu_device)
    with pytest.raises(ValueError, match="set_input_normalisation"):
        model.get_attention_relevance(xu, t, chunk="train")  # as forward(): raw pixels need the affine
    model.set_input_normalisation(mean, std)
    got = model.get_attention_relevance(xu, t, chunk="train", start_layer=8)
    m, s = (torch.tensor(v, device=gpu_device).view(1, 5, 1, 1) for v in (mean, std))
    plain = _build(case, gpu_device)
    same = plain.get_attention_relevance((xu.float() / 255.0 - m) / s, t, chunk="train", start_layer=8)
    dist = _distances(got, same)
    print(f"uint8 through the input affine against the normalised float input: tv {dist[0]:.2e}, r[:,0] rel {dist[1]:.2e}, sum rel {dist[2]:.2e}")
    assert max(dist) <= FACTOR * case["emu_tv"]  # the two differ by the rounding of the affine: inside what bf16 operands move


def test_train_mode_hcs_and_token_drop(gpu_device):
    meta, _ = load_golden("attn_relevance")
    case = meta["cases"][0]
    x = _batch(case, gpu_device)
    t = torch.tensor(case["targets"][0], device=gpu_device)
    picked = [3, 0, 4]

    def check(r, n_tokens):
        assert tuple(r.shape) == (case["B"], n_tokens) and r.dtype == torch.float32 and torch.isfinite(r).all()
        assert bool((r >= 0).all()) and bool((r[:, 0] >= 1).all()) and bool((r[:, 1:].sum(-1) > 0).all())

    # HCS in train mode with a pinned sampler: 3 of the 5 channels
    model = _build(case, gpu_device, enable_sample=True).train()
    model.hcs_sampler = lambda m, chunk, cur, picked=picked: (picked, [cur.index(c) for c in picked])
    check(model.get_attention_relevance(x, t, chunk="train"), 1 + 3 * 16)
    assert model._sr_seed is None  # no stochastic rounding was drawn
    del model
    # token drop: N is the tokens this forward saw
    model = _build(case, gpu_device, dropout_tokens_hcs="channel_random50").train()  # keeps ceil(5 / 2) = 3 whole channels
    random.seed(5)
    check(model.get_attention_relevance(x, t, chunk="train"), 1 + 3 * 16)
    model.eval()  # eval ignores the option
    check(model.get_attention_relevance(x, t, chunk="train"), case["N"])
    del model
    # both: ceil(3 / 2) = 2 of the 3 sampled channels stay
    model = _build(case, gpu_device, enable_sample=True, dropout_tokens_hcs="channel_random50").train()
    model.hcs_sampler = lambda m, chunk, cur, picked=picked: (picked, [cur.index(c) for c in picked])
    check(model.get_attention_relevance(x, t, chunk="train"), 1 + 2 * 16)


def test_bad_arguments_raise(gpu_device):
    meta, _ = load_golden("attn_relevance")
    case = meta["cases"][0]
    model = _build(case, gpu_device)
    fe = model.feature_extractor
    x = _batch(case, gpu_device)
    B, N, D, K = case["B"], case["N"], model.dim, case["num_classes"]
    ok = torch.zeros(B, dtype=torch.long, device=gpu_device)
    okf = torch.randn(B, D, device=gpu_device)
    for bad in (ok[:1], ok.view(B, 1), ok.bool(), ok.cpu(), ok + K, ok - 1, okf[:, :-1].contiguous(), okf[:1], okf.double(), okf.half(), okf.cpu(),
                [0, 1], 3):
        with pytest.raises(ValueError, match="target"):
            model.get_attention_relevance(x, bad, chunk="train")
    for bad in (ok, okf.double(), None):
        with pytest.raises(ValueError, match="dfeat"):
            fe.get_attention_relevance(x, bad, chunk="train")
    with pytest.raises(ValueError, match="start_layer"):
        model.get_attention_relevance(x, ok, chunk="train", start_layer=12)
    with pytest.raises(ValueError, match="start_layer"):
        fe.get_attention_relevance(x, okf, chunk="train", start_layer=-13)
    st = torch.rand(B, N, device=gpu_device)
    neg = st.clone()
    neg[1, N - 1] = -1e-6
    for bad in (st[:, :-1].contiguous(), st.double(), st.cpu(), -st, neg, torch.full_like(st, float("nan")), [1.0]):
        with pytest.raises(ValueError, match="start"):
            model.get_attention_relevance(x, ok, chunk="train", start=bad)
    with pytest.raises(KeyError):
        model.get_attention_relevance(x, ok)  # as the other probes: the default chunk "" is no mapper key
    # no head and no float target
    headless = _build(case, gpu_device)
    headless.classifer_head = torch.nn.Identity()
    for t in (None, ok):
        with pytest.raises(ValueError, match="no classifier head"):
            headless.get_attention_relevance(x, t, chunk="train")
    r = headless.get_attention_relevance(x, okf, chunk="train")
    assert tuple(r.shape) == (B, N) and torch.equal(r, model.get_attention_relevance(x, okf, chunk="train"))
    # an orphaned encoder has no owner to run through
    orphan = copy.copy(fe)
    orphan._owner = None
    with pytest.raises(RuntimeError, match="not linked"):
        orphan.get_attention_relevance(x, okf, chunk="train")


def test_probe_leaves_the_training_step_alone(gpu_device):
    """A relevance call between loss = ... and loss.backward() must not touch what the backward reads (the stochastically rounded operand
    copies, the pre-scaled q bias, the rounding seed), any .grad or the gradient arena: gradients, the updated parameters and the next step's
    loss and gradients are bit-identical to the same sequence without it."""
    from diverse_channel_vit_amd import hip
    from diverse_channel_vit_amd.optim import HipAdamW
    assert hip.is_deterministic()
    meta, _ = load_golden("attn_relevance")
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
            seed = model._sr_seed.clone()
            for mode in ("eval", "train"):
                getattr(model, mode)()
                got = model.get_attention_relevance(x, y, chunk=case["chunk"])
                assert torch.isfinite(got).all() and not got.requires_grad
            assert torch.equal(model._sr_seed, seed) and all(p.grad is None for p in model.parameters())
        loss.backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        if probe:  # with gradients in place: none is touched
            got = model.get_attention_relevance(x, y, chunk=case["chunk"])
            assert not [n for n, p in model.named_parameters() if p.grad is not None and not torch.equal(p.grad, grads[n])]
        opt.step()
        opt.zero_grad(set_to_none=True)
        params = {n: p.detach().clone() for n, p in model.named_parameters()}
        out2, extra2 = model(x, case["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss2 = torch.nn.functional.cross_entropy(out2, y) + extra2
        loss2.backward()
        grads2 = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        runs.append((loss.detach().clone(), grads, params, loss2.detach().clone(), grads2, model._sr_seed.clone()))
        del model, opt
    (l0, g0, p0, m0, h0, s0), (l1, g1, p1, m1, h1, s1) = runs
    assert torch.equal(l0, l1) and g0.keys() == g1.keys() and len(g0) > 100
    assert not [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not [n for n in p0 if not torch.equal(p0[n], p1[n])]
    assert torch.equal(m0, m1) and torch.equal(s0, s1)
    assert not [n for n in h0 if not torch.equal(h0[n], h1[n])]
