"""The selective backward on an MI355X: dcv_bias_grad (the bias gradient without its weight gradient) bit for bit on exact operands and within
the fp32 summation bound on random ones, and the model's backward under set_trainable() presets and hand-set requires_grad patterns against
the full backward — same bits wherever a launch survived, no launch for a frozen weight, one dcv_bias_grad per "frozen weight, trained bias"
layer, None from the node for whoever did not ask.

The launch plan of dcv_bias_grad is restated here (bias_plan, from csrc/bias_grad.hip) with the case table of the kernel tests;
tests/test_selective_backward_cpu.py holds both against the library without a GPU.  Model-level tests build the tiny model of
tests/golden/tiny_e2e.npz (depth 12, 3 channels, 32 x 32, B 2: M = 98 token rows), nearest rounding, deterministic reductions.
Needs an MI355X (-m gpu)."""
import importlib
import json
import os
from collections import namedtuple

import pytest
import torch

from conftest import GOLDEN, load_golden
from oracle import dichavit_oracle as orc

# ---- csrc/bias_grad.hip restated ---------------------------------------------------------------------------------------------------
BG_U, BG_WAVES, BG_GRID_CAP = 8, 4, 512  # 16-byte loads in flight per lane, waves per workgroup, the grid cap
BiasPlan = namedtuple("BiasPlan", "col_chunks lpc s rows_per_wave rows_per_wg row_chunks row_wgs passes")


def bias_plan(M, P):
    units = P // 8
    col_chunks = -(-units // 64)
    lpc = -(-units // col_chunks)
    s = 64 // lpc
    rows_per_wave = BG_U * s
    rows_per_wg = BG_WAVES * rows_per_wave
    row_chunks = -(-M // rows_per_wg)
    row_wgs = min(row_chunks, max(BG_GRID_CAP // col_chunks, 1))
    return BiasPlan(col_chunks, lpc, s, rows_per_wave, rows_per_wg, row_chunks, row_wgs, -(-row_chunks // row_wgs))


WIDTHS = (8, 192, 384, 1152, 1536)  # one lane per row; two rows per wave load; 48 of 64 lanes; three column chunks of 48 and of 64 lanes
BCase = namedtuple("BCase", "name M P ldy")


def bias_cases():
    """Every seam of the plan at every width: one row; one below / at / one above a wave step, a workgroup's row chunk and the rows one grid
    pass covers (above it some workgroup walks two chunks and the others one); a padded layout at the workgroup seam."""
    out = []
    for P in WIDTHS:
        p1 = bias_plan(1, P)
        cap_rows = max(BG_GRID_CAP // p1.col_chunks, 1) * p1.rows_per_wg
        out.append(BCase(f"P{P} one row", 1, P, P))
        for what, at in (("wave", p1.rows_per_wave), ("workgroup", p1.rows_per_wg), ("grid pass", cap_rows)):
            for d in (-1, 0, 1):
                out.append(BCase(f"P{P} {what} {d:+d}", at + d, P, P))
        out.append(BCase(f"P{P} padded rows", 3 * p1.rows_per_wg + 1, P, P + 24))
    return out


BIAS_CASES = bias_cases()


def visited_rows(M, P):
    """The rows every workgroup of the plan adds, in the kernel's index arithmetic: workgroup b walks row chunks b, b + row_wgs, ...; wave w,
    load j, sub-row q of a chunk take row chunk * rows_per_wg + w * rows_per_wave + j * s + q when it lies below M.  Returns one list per
    workgroup (the same for every column chunk)."""
    p = bias_plan(M, P)
    out = []
    for b in range(p.row_wgs):
        rows = []
        for rc in range(b, p.row_chunks, p.row_wgs):
            for w in range(BG_WAVES):
                for j in range(BG_U):
                    for q in range(p.s):
                        r = rc * p.rows_per_wg + w * p.rows_per_wave + j * p.s + q
                        if r < M:
                            rows.append(r)
        out.append(rows)
    return out


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def _bits(t):
    return t.view(torch.int32)


SENT, GUARD = 1e30, -77.0


def _operands(M, P, ldy, dev, gen, exact):
    """Y [M, P] inside a [M + 2, ldy] buffer whose guard rows and padding columns hold a sentinel; dbias [P] inside a guarded buffer."""
    buf = torch.full((M + 2, ldy), SENT, dtype=torch.bfloat16, device=dev)
    Y = buf[1:M + 1, :P]
    if exact:
        Y.copy_(torch.randint(-4, 5, (M, P), device=dev, generator=gen).to(torch.bfloat16))
    else:
        Y.copy_((torch.randn(M, P, device=dev, generator=gen) * 3).to(torch.bfloat16))
    dfull = torch.full((P + 16,), GUARD, dtype=torch.float32, device=dev)
    dbias = dfull[8:8 + P]
    return Y, dfull, dbias


@pytest.mark.parametrize("case", BIAS_CASES, ids=lambda c: c.name)
def test_bias_grad_exact_operands(hip, case):
    """Integers in [-4, 4] and an integer preload: every partial sum is an integer below 2^24, so the result is the int64 column sum plus the
    preload bit for bit, whatever the order.  The sentinel around Y does not leak and the floats around dbias stay untouched."""
    import ctypes as C
    M, P, ldy = case.M, case.P, case.ldy
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(M % 9973 + P)
    Y, dfull, dbias = _operands(M, P, ldy, dev, gen, exact=True)
    pre = torch.randint(-3, 4, (P,), device=dev, generator=gen).float()
    dbias.copy_(pre)
    lib = hip.load()
    got = [C.c_int() for _ in range(5)]
    assert lib.dcv_bias_grad_plan(M, P, *[C.byref(g) for g in got]) == 0
    p = bias_plan(M, P)
    assert [g.value for g in got] == [p.col_chunks, p.rows_per_wave, p.rows_per_wg, p.row_wgs, p.passes]
    hip.bias_grad(Y, dbias)
    ref = torch.sum(Y, dim=0, dtype=torch.float64) + pre.double()
    assert float(ref.abs().max()) < 2 ** 24
    same = dbias.double() == ref
    assert bool(same.all()), f"{case.name}: {int((~same).sum())} columns differ, first at {int((~same).nonzero()[0])}"
    assert bool((dfull[:8] == GUARD).all()) and bool((dfull[8 + P:] == GUARD).all()), "dcv_bias_grad wrote outside dbias"


RANDOM_SHAPES = [(1000, 384), (777, 1536)] + [(bias_plan(1, P).rows_per_wg * (BG_GRID_CAP // bias_plan(1, P).col_chunks + 3) + 5, P) for P in (384, 1152)]


@pytest.mark.parametrize("M,P", RANDOM_SHAPES, ids=lambda v: str(v))
def test_bias_grad_random_operands(hip, M, P):
    """Random bf16 operands against float64 column sums: |got - ref| <= M 2^-24 sum_m |Y[m, p]| per element, the bound of an fp32 summation of
    M terms in any order (every one of the at most M - 1 additions a term goes through rounds by at most 2^-24 relative).  The large shapes
    cross the grid cap once: most workgroups walk one row chunk, a few walk two.  Two calls on the same input give the same bits."""
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(P + 1)
    Y, _, dbias = _operands(M, P, P, dev, gen, exact=False)
    p = bias_plan(M, P)
    assert p.passes == (2 if M > 5000 else 1)
    dbias.zero_()
    hip.bias_grad(Y, dbias)
    first = dbias.clone()
    dbias.zero_()
    hip.bias_grad(Y, dbias)
    assert torch.equal(_bits(first), _bits(dbias))
    ref = torch.sum(Y, dim=0, dtype=torch.float64)
    bound = M * 2.0 ** -24 * torch.sum(Y.abs(), dim=0, dtype=torch.float64)
    err = (dbias.double() - ref).abs()
    print(f"M {M} P {P}: max |err| {err.max().item():.3e}, smallest bound {bound.min().item():.3e}, max err / bound {(err / bound).max().item():.3e}")
    assert bool((err <= bound).all())


# ---- model level -------------------------------------------------------------------------------------------------------------------
dichavit = importlib.import_module("diverse_channel_vit_amd.dichavit")  # the package attribute of that name is the factory function
LINEARS = ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")


class Cfg(dict):
    __getattr__ = dict.get


def build(device, **cfg_over):
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("tiny_e2e")
    cfgd = dict(meta["cfg"], **cfg_over)
    cfg = Cfg(cfgd, in_channel_names=[f"c{i}" for i in range(meta["n_channels"])], img_size=[meta["img"]], num_classes=meta["num_classes"])
    model = dcv.dichavit(cfg, mapper={k: list(v) for k, v in meta["mapper"].items()})
    st = orc.make_state(orc.state_shapes(cfgd, meta["n_channels"], meta["img"], meta["num_classes"]), meta["seed"])
    model.load_state_dict({**st, "adaptive_interface.0": st["proxies"]}, strict=True)
    model = model.to(device).train()
    model.stochastic_weight_rounding = False
    assert len(model.feature_extractor.blocks) == 12
    return model


def batch(device, seed=3):
    x, y = orc.make_batch(seed, 2, 3, 32, 5)
    return x.to(device), y.to(device)


def fwd_bwd(model, x, y, zero=True):
    if zero:
        model.zero_grad(set_to_none=True)
        x.grad = None
    out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    loss = torch.nn.functional.cross_entropy(out, y) + extra
    loss.backward()
    return out.detach().clone(), loss.detach().clone()


def linear_layers(model):
    """{weight name: (weight, bias, bias name)} of the layers the gradient plan's table covers: four per block and the patch projection."""
    named = dict(model.named_parameters())
    names = [f"feature_extractor.blocks.{bi}.{lin}" for bi in range(len(model.feature_extractor.blocks)) for lin in LINEARS]
    names.append("feature_extractor.patch_embed.proj")
    return {n + ".weight": (named[n + ".weight"], named[n + ".bias"], n + ".bias") for n in names}


class Recorded:
    """One forward + backward under the pass-through launch recorder of tests/switch_pairs.py, with post hooks that note, per weight-gradient
    launch, the arena slot it wrote (by name) and, per bias sum, the Y buffer it read."""

    def __init__(self, model, x, y, passes=1):
        import switch_pairs as sp
        self.products, self.bias_sums, self.tn_Y, self.node_out = [], [], {}, []
        mp = pytest.MonkeyPatch()
        try:
            self.log = sp.install_recorder(mp.setattr, post={"gemm_tn_acc": self._tn, "gemm_tn_acc_group": self._group, "bias_grad": self._bias})
            real = dichavit._EncoderFn._backward

            def backward(ctx, *a):
                res = real(ctx, *a)
                self.node_out.append(res)
                return res

            mp.setattr(dichavit._EncoderFn, "_backward", staticmethod(backward))
            self.model = model
            self.out, self.loss = fwd_bwd(model, x, y)
            for _ in range(passes - 1):
                fwd_bwd(model, x, y, zero=False)
            torch.cuda.synchronize()
        finally:
            mp.undo()
        self.names = [n for n, _ in self.log]
        self.grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        self.xgrad = None if x.grad is None else x.grad.detach().clone()

    def _slot(self, t):
        """the name of the encoder parameter whose gradient-arena slot (or scratch-arena slot) starts at t"""
        m = self.model
        for ga in (m._grad_arena, m._grad_scratch):
            if ga is not None:
                off = (t.data_ptr() - ga.data_ptr()) // 4
                if 0 <= off < ga.numel():
                    i = m._enc_off.index(off)
                    return self._pname[id(m._enc_params[i])]
        raise AssertionError("a gradient was written outside the gradient arena")

    @property
    def _pname(self):
        return {id(p): n for n, p in self.model.named_parameters()}

    def _tn(self, a):
        w = self._slot(a["dW"])
        b = None if a["dbias"] is None else self._slot(a["dbias"])
        self.products.append((w, b, "single"))
        if b is not None:
            self.tn_Y[b] = a["Y"].detach().clone()

    def _group(self, a):
        for Y, X, dW, db in a["items"]:
            self.products.append((self._slot(dW), None if db is None else self._slot(db), "group"))

    def _bias(self, a):
        self.bias_sums.append((self._slot(a["dbias"]), a["Y"].detach().clone()))


@pytest.fixture(scope="module")
def full_runs(gpu_device):
    """The reference runs, computed once: the full backward as shipped and with wgrad_group = False, both again with x.requires_grad."""
    runs = {}
    for grouped in (True, False):
        for xg in (False, True):
            model = build(gpu_device)
            model.wgrad_group = grouped
            x, y = batch(gpu_device)
            runs[(grouped, xg)] = Recorded(model, x.requires_grad_(xg), y)
    return runs


CONFIGS = [
    (("channel_embed",), False),
    (("bias",), False),
    (("norm",), False),
    (("head", "norm"), False),
    (("feature_extractor.blocks.*.attn.qkv.weight",), False),
    (("channel_embed", "feature_extractor.blocks.7.mlp.fc1.*"), False),
    (("bias",), True),
]
ALWAYS_EXACT = ("feature_extractor.patch_embed.channel_embed.weight", "feature_extractor.pos_embed", "feature_extractor.cls_token")


@pytest.mark.parametrize("specs,xgrad", CONFIGS, ids=lambda v: "+".join(v) if isinstance(v, tuple) else f"x{int(v)}")
def test_selective_backward_against_the_full_one(gpu_device, full_runs, specs, xgrad):
    """What the issue's configurations must keep and must drop: see the module docstring.  The reference of a launched product is the
    wgrad_group = False full run when its block kept fewer than four products and the shipped full run otherwise (on this width — D = 192, no
    grouped plan — the two coincide, which the test states as well)."""
    model = build(gpu_device)
    trainable = model.set_trainable(*specs)
    x, y = batch(gpu_device)
    run = Recorded(model, x.requires_grad_(xgrad), y)
    ref_g, ref_s = full_runs[(True, xgrad)], full_runs[(False, xgrad)]
    for n in ref_g.grads:
        assert torch.equal(_bits(ref_g.grads[n]), _bits(ref_s.grads[n])), f"{n}: D = 192 has no grouped launch"
    assert torch.equal(_bits(run.out), _bits(ref_g.out)) and torch.equal(_bits(run.loss), _bits(ref_g.loss))
    named = dict(model.named_parameters())
    for n, p in named.items():
        assert (p.grad is None) == (n not in trainable or n == "proxies"), n  # `proxies` has no gradient in this loss
    if xgrad:
        assert torch.equal(_bits(run.xgrad), _bits(ref_g.xgrad))
    layers = linear_layers(model)
    products_of_block = {}
    for wn, (w, b, bn) in layers.items():
        blk = wn.rsplit(".", 3)[0] if ".blocks." in wn else "patch"
        products_of_block[blk] = products_of_block.get(blk, 0) + int(w.requires_grad)
    bias_only = {bn for wn, (w, b, bn) in layers.items() if b.requires_grad and not w.requires_grad}
    in_table = {n for wn, (w, b, bn) in layers.items() for n in (wn, bn)}
    checked = 0
    for n in trainable:
        if n == "proxies" or n in bias_only:
            continue
        ref = ref_g
        if n in in_table:  # a launched product (the weight and, when trained, its bias)
            wn = n if n.endswith(".weight") else n[:-5] + ".weight"
            blk = wn.rsplit(".", 3)[0] if ".blocks." in wn else "patch"
            ref = ref_s if blk != "patch" and products_of_block[blk] < 4 else ref_g
        assert torch.equal(_bits(run.grads[n]), _bits(ref.grads[n])), n
        checked += 1
    assert checked == len([n for n in trainable if n != "proxies"]) - len(bias_only)
    for n in ALWAYS_EXACT:
        assert (n in trainable) == (n in run.grads)
    # the bias sums: one dcv_bias_grad per "frozen weight, trained bias" layer, on the buffer the full run's product read, within the bound
    assert sorted(n for n, _ in run.bias_sums) == sorted(bias_only)
    for bn, Y in run.bias_sums:
        assert torch.equal(Y.view(torch.int16), ref_g.tn_Y[bn].view(torch.int16)), f"{bn}: another buffer than the full run's product read"
        M = Y.shape[0]
        ref = torch.sum(Y, dim=0, dtype=torch.float64)
        bound = M * 2.0 ** -24 * torch.sum(Y.abs(), dim=0, dtype=torch.float64)
        err = (run.grads[bn].double() - ref).abs()
        assert bool((err <= bound).all()), (bn, float((err - bound).max()))
    # no product for a frozen weight, every product of a trained one, its bias sum inside exactly when the bias is trained
    launched = {w: b for w, b, _ in run.products}
    assert len(launched) == len(run.products)
    assert sorted(launched) == sorted(wn for wn, (w, b, bn) in layers.items() if w.requires_grad)
    for wn, b in launched.items():
        assert b == (layers[wn][2] if layers[wn][1].requires_grad else None), wn
    # the node returned None for every parameter that did not ask
    assert len(run.node_out) == 1
    res = run.node_out[0]
    assert len(res) == 9 + len(model._enc_params)
    for p, g in zip(model._enc_params, res[9:]):
        assert (g is None) == (not p.requires_grad)
    assert (res[6] is None) == (not xgrad)


def _step_names(model, x, y, opt=None):
    """The recorder's names over one training step: forward, backward and, with opt, clip_grad_norm_ and the optimiser step."""
    import diverse_channel_vit_amd as dcv
    import switch_pairs as sp
    mp = pytest.MonkeyPatch()
    try:
        log = sp.install_recorder(mp.setattr)
        fwd_bwd(model, x, y)
        if opt is not None:
            dcv.clip_grad_norm_(model, 1.0)
            opt.step()
        torch.cuda.synchronize()
    finally:
        mp.undo()
    return [n for n, _ in log]


def recorded_sequences(device):
    """The three launch sequences tests/golden/selective_backward_launches.json holds, as recorded on the commit before the selective backward:
    a training step with every flag true, one under freeze_prefix(6), and the data-only call (every parameter frozen, x asks)."""
    import diverse_channel_vit_amd as dcv
    out = {}
    x, y = batch(device)
    model = build(device)
    fwd_bwd(model, x, y)  # arenas and workspaces exist from here on
    opt = dcv.HipAdamW(dcv.param_groups(model, lr=1e-3, weight_decay=0.05), model=model)
    out["train_step"] = _step_names(model, x, y, opt)
    model = build(device)
    model.freeze_prefix(6)
    out["freeze_prefix_6"] = _step_names(model, x, y)
    model = build(device)
    for p in model.parameters():
        p.requires_grad_(False)
    out["data_only"] = _step_names(model, x.clone().requires_grad_(True), y)
    return out


def test_unchanged_launch_sequences_and_bits(gpu_device, full_runs):
    """With every flag true, under freeze_prefix(6) and in the data-only call the recorder's log is the previous commit's, name for name
    (tests/golden/selective_backward_launches.json, recorded there on an MI355X), and the gradients are the full run's bits."""
    with open(os.path.join(GOLDEN, "selective_backward_launches.json")) as f:
        want = json.load(f)
    got = recorded_sequences(gpu_device)
    for key in ("train_step", "freeze_prefix_6", "data_only"):
        assert got[key] == want[key], f"{key}: the launch sequence changed"
    assert "bias_grad" not in sum(got.values(), [])
    x, y = batch(gpu_device)
    ref, refx = full_runs[(True, False)], full_runs[(True, True)]
    model = build(gpu_device)
    model.freeze_prefix(6)
    out, loss = fwd_bwd(model, x, y)
    assert torch.equal(_bits(out), _bits(ref.out))
    live = {n for n, p in model.named_parameters() if p.grad is not None}
    assert len(live) == 12 * 6 + 4
    for n in live:
        assert torch.equal(_bits(dict(model.named_parameters())[n].grad), _bits(ref.grads[n])), n
    model = build(gpu_device)
    for p in model.parameters():
        p.requires_grad_(False)
    arena = model._grad_arena
    xg = x.clone().requires_grad_(True)
    fwd_bwd(model, xg, y)
    assert model._grad_arena is arena and all(p.grad is None for p in model.parameters())
    assert torch.equal(_bits(xg.grad), _bits(refx.xgrad))


def test_width_384_partial_block_goes_out_product_by_product(gpu_device):
    """D = 384 (the small model on the same batch, M = 98), where _group_ok has a plan: with one weight of block 5 frozen that block's three
    remaining products are the wgrad_group = False full run's bits and every other block's gradients the grouped full run's."""
    x, y = batch(gpu_device)
    runs = {}
    for key in ("grouped", "single", "partial"):
        model = build(gpu_device, pretrained_model_name="small")
        assert model.dim == 384 and model._group_ok(x.shape[0] * 49, 384), "no grouped plan on this fixture"
        model.wgrad_group = key != "single"
        if key == "partial":
            model.feature_extractor.blocks[5].mlp.fc1.weight.requires_grad_(False)
        runs[key] = Recorded(model, x, y)
    g, s, p = runs["grouped"], runs["single"], runs["partial"]
    assert "gemm_tn_acc_group" in g.names and "gemm_tn_acc_group" not in s.names
    frozen = "feature_extractor.blocks.5.mlp.fc1.weight"
    assert frozen not in p.grads and [n for n, _ in p.bias_sums] == [frozen[:-6] + "bias"]
    kinds = {w: kind for w, b, kind in p.products}
    assert frozen not in kinds
    n_blk5 = 0
    for n, grad in p.grads.items():
        if n == frozen[:-6] + "bias":
            continue
        blk5 = n.startswith("feature_extractor.blocks.5.") and (".attn." in n or ".mlp." in n)
        ref = s if blk5 else g
        assert torch.equal(_bits(grad), _bits(ref.grads[n])), n
        if n in kinds:
            assert kinds[n] == ("single" if blk5 else ("group" if ".blocks." in n and ".blocks.11." not in n else "single")), n
        n_blk5 += int(blk5)
    assert n_blk5 == 6  # three weights with their biases
    differ = [n for n in g.grads if not torch.equal(_bits(g.grads[n]), _bits(s.grads[n]))]
    print(f"D = 384, M = 98: {len(differ)} gradients differ in bits between the grouped and the one-by-one full run")


def _memory_of(model, x, y):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fwd_bwd(model, x, y)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def _encoder_node(out):
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


def test_channel_embed_only_keeps_no_product_operand(gpu_device):
    """("channel_embed",): the saved state of a block holds none of h, u1, u2 (o stays: the attention backward reads it), the tokeniser's
    im2col rows are not kept, and the peak of forward + backward is strictly below the full step's."""
    model = build(gpu_device)
    x, y = batch(gpu_device)
    fwd_bwd(model, x, y)  # arenas and workspaces exist from here on
    m_full = _memory_of(model, x, y)
    out, _ = model(x, "train", None)
    st = _encoder_node(out).st
    assert all(k in st["layers"][3] for k in ("h", "u1", "u2", "o")) and "Xp" in st
    model.set_trainable("channel_embed")
    m_sel = _memory_of(model, x, y)
    print(f"peak memory of forward + backward: full {m_full} B, channel_embed only {m_sel} B")
    assert m_sel < m_full
    out, _ = model(x, "train", None)
    st = _encoder_node(out).st
    assert "Xp" not in st and st["frozen_k"] is None and not st.get("data_only")
    for L in st["layers"]:
        assert not any(k in L for k in ("h", "u1", "u2")) and all(k in L for k in ("o", "qkv", "z", "x_in", "x_mid"))


def test_two_backward_passes_accumulate(gpu_device):
    """The CHAMMI step under ("bias",): .grad after two passes is, bit for bit, the sum autograd forms from the two single-pass results."""
    x1, y1 = batch(gpu_device, seed=3)
    x2, y2 = batch(gpu_device, seed=4)
    singles = []
    for x, y in ((x1, y1), (x2, y2)):
        model = build(gpu_device)
        model.set_trainable("bias")
        fwd_bwd(model, x, y)
        singles.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    model = build(gpu_device)
    model.set_trainable("bias")
    fwd_bwd(model, x1, y1)
    fwd_bwd(model, x2, y2, zero=False)
    both = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert sorted(both) == sorted(singles[0]) and len(both) == 12 * 6 + 1 + 1 + 1  # six biases per block, patch projection, final norm, head
    for n, g in both.items():
        assert torch.equal(_bits(g), _bits(singles[0][n] + singles[1][n])), n


def test_hipadamw_step_on_scattered_trainable_runs(gpu_device):
    """("bias", "channel_embed"): the trainable tensors are scattered runs of the arena, not a prefix.  One HipAdamW step over param_groups:
    frozen parameters keep their bits, updated ones are within 1e-6 |p| + 1e-7 of a float64 AdamW step (the bound of
    test_llrd_groups_follow_torch_float64), and clip_grad_norm_ returns the norm of the gradients that exist."""
    import diverse_channel_vit_amd as dcv
    model = build(gpu_device)
    trainable = set(model.set_trainable("bias", "channel_embed"))
    x, y = batch(gpu_device)
    groups = dcv.param_groups(model, lr=1e-3, weight_decay=0.05)
    assert {id(p) for g in groups for p in g["params"]} == {id(p) for n, p in model.named_parameters() if n in trainable}
    opt = dcv.HipAdamW(groups, model=model)
    fwd_bwd(model, x, y)
    named = dict(model.named_parameters())
    live = [n for n, p in named.items() if p.grad is not None]
    assert sorted(live) == sorted(trainable)
    want = torch.sqrt(sum((named[n].grad.double() ** 2).sum() for n in live)).item()
    got = dcv.clip_grad_norm_(model, 10.0 * want).item()  # the clip does not bite: the gradients stay as they are
    print(f"gradient norm under (bias, channel_embed): float64 {want:.8g}, HIP {got:.8g}")
    assert abs(got - want) <= 1e-5 * want
    before = {n: p.detach().clone() for n, p in named.items()}
    ref = {}
    for g in opt.param_groups:
        twins = [p.detach().double().clone().requires_grad_(True) for p in g["params"]]
        for q, p in zip(twins, g["params"]):
            q.grad = p.grad.detach().double().clone()
        torch.optim.AdamW(twins, lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"], foreach=False).step()
        ref.update({id(p): q.detach() for p, q in zip(g["params"], twins)})
    opt.step()
    torch.cuda.synchronize()
    for n, p in named.items():
        if n in trainable:
            err = (p.detach().double() - ref[id(p)]).abs()
            bound = 1e-6 * ref[id(p)].abs() + 1e-7
            assert bool((err <= bound).all()), n
            assert not torch.equal(_bits(p.detach()), _bits(before[n])) or not bool(p.grad.any()), n
        else:
            assert torch.equal(_bits(p.detach()), _bits(before[n])), n


def test_feature_taps_with_drop_path_under_norm_only(gpu_device):
    """forward_with_features(layers=[3], pool="channel") with drop_path_rate > 0 and pinned masks under ("norm",): the gradients of the
    parameters that remain are the bits of the same call on the all-trainable model."""
    x, y = batch(gpu_device)

    def masks(bi, branch, B, dev):
        return torch.tensor([(bi + (branch == "mlp")) % 2, 1.0])[:B]

    grads = []
    for specs in (None, ("norm",)):
        model = build(gpu_device, drop_path_rate=0.3)
        model.drop_path_sampler = masks
        if specs:
            model.set_trainable(*specs)
        model.zero_grad(set_to_none=True)
        (out, extra), feats = model.forward_with_features(x, "train", None, layers=[3], pool="channel")
        loss = torch.nn.functional.cross_entropy(out, y) + extra + feats[0].square().mean()
        loss.backward()
        grads.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    full, sel = grads
    assert len(sel) == 12 * 4 + 2
    for n, g in sel.items():
        assert torch.equal(_bits(g), _bits(full[n])), n
