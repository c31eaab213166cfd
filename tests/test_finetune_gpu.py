"""Fine-tuning on the HIP path: dcv_adamw_groups (AdamW over the arena with a table of runs) held bit for bit to dcv_adamw_dyn called
once per run; HipAdamW with parameter groups and frozen parameters against torch.optim.AdamW in float64; the frozen-prefix forward and
backward against the full one, bit for bit; clip_grad_norm_ over runs of gradients; the captured multi-group step.

The launch plan of dcv_adamw_groups is restated here (groups_plan, from csrc/optim_groups.hip) with the case table of the kernel test;
tests/test_finetune_cpu.py checks both without a GPU.  Model-level tests build the tiny model of tests/golden/tiny_e2e.npz (depth 12,
3 channels, 32 x 32, B 2).  Needs an MI355X (-m gpu)."""
import random
from collections import namedtuple

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import dichavit_oracle as orc

# ---- csrc/optim_groups.hip restated ------------------------------------------------------------------------------------------------
CHUNK4, GRID_CAP, LANES = 1024, 2048, 256  # ADAMW_G_CHUNK4, ADAMW_G_GRID_CAP, workgroup size
MAX_GROUPS, MAX_SEGS = 32, 1024            # include/dcv.h

GroupsPlan = namedtuple("GroupsPlan", "grid nchunks chunks_min chunks_max ragged4")


def groups_plan(n4):
    nchunks = -(-n4 // CHUNK4)
    grid = min(nchunks, GRID_CAP)
    return GroupsPlan(grid, nchunks, nchunks // grid, -(-nchunks // grid), n4 % CHUNK4)


def groups_regime(n4):
    p = groups_plan(n4)
    if p.nchunks < GRID_CAP:
        return "below cap"
    if p.nchunks == GRID_CAP:
        return "at cap"
    if p.nchunks == GRID_CAP + 1 and not p.ragged4:
        return "cap + 1"
    return "rounds + ragged" if p.chunks_min >= 2 and p.ragged4 else "past cap"


def groups_visits(n4):
    """How often the kernel's loops reach every float4 of [0, n4): workgroup b walks chunks b, b + grid, ...; lane t of a chunk takes
    base + t, base + 256 + t, ... below the chunk's end."""
    p = groups_plan(n4)
    seen = np.zeros(n4, dtype=np.int32)
    lanes = np.arange(LANES)
    for b in range(p.grid):
        for c in range(b, p.nchunks, p.grid):
            base, cend = c * CHUNK4, min(c * CHUNK4 + CHUNK4, n4)
            for j in range(CHUNK4 // LANES):
                i = base + j * LANES + lanes
                np.add.at(seen, i[i < cend], 1)
    return seen


def _runs(n4, cuts, groups):
    """cuts: interior run ends (float4 units); groups: one row per run."""
    ends = sorted(cuts) + [n4]
    assert len(ends) == len(groups) and len(set(ends)) == len(ends) and ends[0] > 0
    return ends, list(groups)


def _many_runs(n4, n_runs, first, seed, n_groups):
    """n_runs - 1 cuts from `first` on, 1 to 3 float4 apart: run 0 is [0, first + ...), the last run takes the rest, and the n_runs - 2
    runs between two cuts are 1 to 3 float4 long; rows cycling so that neighbours differ."""
    rs = np.random.RandomState(seed)
    cuts = list(first + np.cumsum(rs.randint(1, 4, n_runs - 1)))
    groups = [(k * 7 + 3) % n_groups if k % 5 else -1 for k in range(n_runs)]
    for k in range(1, n_runs):
        if groups[k] == groups[k - 1]:
            groups[k] = (groups[k] + 1) % n_groups
    return _runs(n4, [int(c) for c in cuts], groups)


GCase = namedtuple("GCase", "name n4 ends groups n_groups")
ROUNDS_N4 = 2 * GRID_CAP * CHUNK4 + 5 * CHUNK4 + 777  # two full rounds, five chunks of a third, a ragged last chunk


def _g(name, n4, table, n_groups):
    return GCase(name, n4, table[0], table[1], n_groups)


GROUPS_CASES = [
    # boundaries exactly on a chunk seam (1024), one float4 after the next (2049) and one before the third (3071); a run of ONE float4
    _g("seams", 4 * CHUNK4 + 100, _runs(4 * CHUNK4 + 100, [1, CHUNK4, 2 * CHUNK4 + 1, 3 * CHUNK4 - 1], [2, 0, 1, 0, 2]), 3),
    _g("one run", 1500, _runs(1500, [], [0]), 1),
    _g("40 runs in a chunk", 3 * CHUNK4, _many_runs(3 * CHUNK4, 42, CHUNK4 + 17, 5, 4), 4),
    _g("max runs", 5 * CHUNK4 + 77, _many_runs(5 * CHUNK4 + 77, MAX_SEGS, 300, 6, MAX_GROUPS), MAX_GROUPS),
    _g("skipped first run", 2 * CHUNK4 + 8, _runs(2 * CHUNK4 + 8, [CHUNK4 + 300, CHUNK4 + 301], [-1, 1, 0]), 2),
    _g("skipped last run", 2 * CHUNK4 + 8, _runs(2 * CHUNK4 + 8, [700, 2 * CHUNK4], [0, 1, -1]), 2),
    _g("at cap", GRID_CAP * CHUNK4, _runs(GRID_CAP * CHUNK4, [CHUNK4 * 1000, CHUNK4 * 1000 + 1], [0, -1, 1]), 2),
    _g("cap + 1", (GRID_CAP + 1) * CHUNK4, _runs((GRID_CAP + 1) * CHUNK4, [GRID_CAP * CHUNK4 - 1, GRID_CAP * CHUNK4 + 1], [1, 0, 1]), 2),
    # workgroups walk two or three chunks; seams of the second and third round cut one before / on / one after
    _g("rounds + ragged", ROUNDS_N4,
       _runs(ROUNDS_N4, [GRID_CAP * CHUNK4 - 1, GRID_CAP * CHUNK4 + 3 * CHUNK4, 2 * GRID_CAP * CHUNK4 + 1, 2 * GRID_CAP * CHUNK4 + 4 * CHUNK4 + 5,
                         ROUNDS_N4 - 300], [0, 1, -1, 2, 0, 1]), 3),
]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def _rows(n_groups, step0):
    """Distinct scalars per group; the step counts differ per group too."""
    rows = [(1e-2 * 0.8 ** k, 0.9 - 0.01 * (k % 5), 0.999 - 0.002 * (k % 7), 1e-8 * (1 + k % 3), 0.05 * (k % 4)) for k in range(n_groups)]
    return rows, [step0 + 3 * k for k in range(n_groups)]


def _bits(t):
    return t.view(torch.int32)


SENT = 12345.678


@pytest.mark.parametrize("case", GROUPS_CASES, ids=lambda c: c.name)
def test_adamw_groups_is_adamw_dyn_per_run(hip, case):
    """p, m, v after three consecutive steps, bit for bit, against dcv_adamw_dyn called once per non-skipped run with that run's row.
    Skipped runs hold a sentinel in p, m, v and NaN in g: the sentinel survives (nothing written) and no NaN appears anywhere (g not
    read); the floats around [0, n) keep their sentinel."""
    n4, n = case.n4, 4 * case.n4
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(case.n4 % 1000 + len(case.ends))
    full = [torch.full((n + 8,), SENT, device=dev) for _ in range(4)]
    p, g, m, v = (t[4:4 + n] for t in full)
    p.copy_(torch.randn(n, device=dev, generator=gen) * 0.3)
    m.copy_(torch.randn(n, device=dev, generator=gen) * 0.01)
    v.copy_(torch.rand(n, device=dev, generator=gen) * 1e-3)
    ends = torch.tensor(case.ends, dtype=torch.int32, device=dev)
    grps = torch.tensor(case.groups, dtype=torch.int32, device=dev)
    skipped = torch.zeros(n, dtype=torch.bool, device=dev)
    lo = 0
    for e, r in zip(case.ends, case.groups):
        if r < 0:
            skipped[4 * lo:4 * e] = True
        lo = e
    for t in (p, m, v):
        t[skipped] = SENT
    rp, rm, rv = p.clone(), m.clone(), v.clone()
    hyper = torch.zeros(8 * case.n_groups, device=dev)
    for step in range(3):
        g.copy_(torch.randn(n, device=dev, generator=gen) * 0.7)
        g[skipped] = float("nan")
        rows, steps = _rows(case.n_groups, 1 + step)
        hip.adamw_set_hyper_groups(hyper, rows, steps, 0.5)
        lo = 0
        for e, r in zip(case.ends, case.groups):
            if r >= 0:
                hip.adamw_dyn(rp[4 * lo:4 * e], g[4 * lo:4 * e], rm[4 * lo:4 * e], rv[4 * lo:4 * e], 4 * (e - lo), hyper[8 * r:8 * r + 8])
            lo = e
        hip.adamw_groups(p, g, m, v, n, ends, grps, len(case.ends), hyper, case.n_groups)
        for name, a, b in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
            same = _bits(a) == _bits(b)
            assert bool(same.all()), f"{case.name} step {step + 1}: {int((~same).sum())} elements of {name} differ, first at {int((~same).nonzero()[0])}"
    for t in (p, m, v):
        assert bool((t[skipped] == SENT).all()) and not bool(torch.isnan(t).any()), case.name
    assert bool((p[~skipped] != SENT).all())  # every other element was updated
    for t in full:
        assert bool((t[:4] == SENT).all()) and bool((t[4 + n:] == SENT).all()), "dcv_adamw_groups wrote outside its range"


def test_set_hyper_groups_rows_and_error_codes(hip):
    """Every row of dcv_adamw_set_hyper_groups holds exactly the eight fp32 values dcv_adamw_set_hyper writes for the same scalars and
    step; every documented bad argument is refused with its code and leaves the buffers alone."""
    import ctypes as C
    dev = "cuda"
    rows, _ = _rows(5, 1)
    for step in (1, 7, 100000):
        steps = [step, 1, step + 1, 7, 100000]
        table = torch.zeros(40, device=dev)
        hip.adamw_set_hyper_groups(table, rows, steps, 0.25)
        for k, (r, s) in enumerate(zip(rows, steps)):
            one = torch.zeros(8, device=dev)
            hip.adamw_set_hyper(one, *r, s, 0.25)
            assert torch.equal(_bits(table[8 * k:8 * k + 8]), _bits(one)), (step, k)
    lib = hip.load()
    n = 64
    p, g, m, v = (torch.full((n + 4,), 1.0, device=dev) for _ in range(4))
    ends, grps = torch.tensor([16], dtype=torch.int32, device=dev), torch.tensor([0], dtype=torch.int32, device=dev)
    hyper = torch.zeros(8 * MAX_GROUPS, device=dev)
    hip.adamw_set_hyper_groups(hyper, rows[:1], [1], 1.0)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ok = [P(p), P(g), P(m), P(v), n, P(ends), P(grps), 1, P(hyper), 1, None]

    def call(**kw):
        a = list(ok)
        for i, val in kw.items():
            a[int(i[1:])] = val
        return lib.dcv_adamw_groups(*a)

    NULL, SHAPE, ALIGN = -5, -1, -2
    for i in (0, 1, 2, 3, 5, 6, 8):
        assert call(**{f"a{i}": None}) == NULL, i
    for bad in (0, -4, 62):
        assert call(a4=bad) == SHAPE, bad
    for bad in (0, MAX_SEGS + 1):
        assert call(a7=bad) == SHAPE, bad
    for bad in (0, MAX_GROUPS + 1):
        assert call(a9=bad) == SHAPE, bad
    for i, t in ((0, p), (1, g), (2, m), (3, v)):
        assert call(**{f"a{i}": C.c_void_p(t.data_ptr() + 4)}) == ALIGN, i
    for i, t in ((5, ends), (6, grps), (8, hyper)):  # the int32 / fp32 tables: 4-byte alignment
        assert call(**{f"a{i}": C.c_void_p(t.data_ptr() + 2)}) == ALIGN, i
    # run ends are int32 float4 indices, and a chunk's end (base + CHUNK4) must not wrap: the first n past that is refused, the last one
    # below it is not a shape error (here it stops at the next check, a misaligned p, so nothing is launched over 34 GB that do not exist)
    assert call(a4=4 * (0x7FFFFFFF - CHUNK4 + 1)) == SHAPE
    assert call(a4=4 * (0x7FFFFFFF - CHUNK4), a0=C.c_void_p(p.data_ptr() + 4)) == ALIGN
    rows_c = (C.c_float * 5)(1e-3, 0.9, 0.999, 1e-8, 0.0)
    one, zero = (C.c_int * 1)(1), (C.c_int * 1)(0)
    sh = lib.dcv_adamw_set_hyper_groups
    assert sh(None, C.cast(rows_c, C.c_void_p), C.cast(one, C.c_void_p), 1, 1.0, None) == NULL
    assert sh(P(hyper), None, C.cast(one, C.c_void_p), 1, 1.0, None) == NULL
    assert sh(P(hyper), C.cast(rows_c, C.c_void_p), None, 1, 1.0, None) == NULL
    assert sh(P(hyper), C.cast(rows_c, C.c_void_p), C.cast(one, C.c_void_p), 0, 1.0, None) == SHAPE
    assert sh(P(hyper), C.cast(rows_c, C.c_void_p), C.cast(one, C.c_void_p), MAX_GROUPS + 1, 1.0, None) == SHAPE
    assert sh(P(hyper), C.cast(rows_c, C.c_void_p), C.cast(zero, C.c_void_p), 1, 1.0, None) == SHAPE
    torch.cuda.synchronize()
    for t in (p, g, m, v):
        assert bool((t == 1.0).all())  # no refused call launched anything


# ---- model level ---------------------------------------------------------------------------------------------------------------------
class Cfg(dict):
    __getattr__ = dict.get


def build(device, **cfg_over):
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("tiny_e2e")
    cfgd = dict(meta["cfg"], **cfg_over)
    cfg = Cfg(cfgd, in_channel_names=[f"c{i}" for i in range(meta["n_channels"])], img_size=[meta["img"]], num_classes=meta["num_classes"])
    model = dcv.dichavit(cfg, mapper={k: list(v) for k, v in meta["mapper"].items()})
    st = orc.make_state(orc.state_shapes(meta["cfg"], meta["n_channels"], meta["img"], meta["num_classes"]), meta["seed"])
    model.load_state_dict({**st, "adaptive_interface.0": st["proxies"]}, strict=True)
    model = model.to(device).train()
    assert len(model.feature_extractor.blocks) == 12
    return model


def batch(device, seed=3):
    x, y = orc.make_batch(seed, 2, 3, 32, 5)
    return x.to(device), y.to(device)


def fwd_bwd(model, x, y, zero=True):
    if zero:
        model.zero_grad(set_to_none=True)
    out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    loss = torch.nn.functional.cross_entropy(out, y) + extra
    loss.backward()
    return out.detach().clone(), loss.detach().clone()


def _torch64_step(opt, expected_step):
    """One float64 torch.optim.AdamW step over opt's groups, from the state HipAdamW holds (the recipe of test_adamw_against_float64: each step
    from the state the kernel itself left).  expected_step: {id(p): step count p is about to take}.  Returns {id(p): p64 after the step}."""
    twins, groups64 = {}, []
    for g in opt.param_groups:
        ps = []
        for p in g["params"]:
            q = p.detach().double().clone().requires_grad_(True)
            twins[id(p)] = q
            ps.append(q)
        groups64.append(dict(params=ps, lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"]))
    ref = torch.optim.AdamW(groups64, foreach=False)
    for g in opt.param_groups:
        for p in g["params"]:
            q = twins[id(p)]
            if p.grad is None:
                continue
            q.grad = p.grad.detach().double().clone()
            st = opt.state.get(p, {})
            t = expected_step[id(p)] - 1
            ref.state[q] = dict(step=torch.tensor(float(t), dtype=torch.float32),
                                exp_avg=st["exp_avg"].detach().double().clone() if "exp_avg" in st else torch.zeros_like(q),
                                exp_avg_sq=st["exp_avg_sq"].detach().double().clone() if "exp_avg_sq" in st else torch.zeros_like(q))
    ref.step()
    return {k: q.detach() for k, q in twins.items()}


def _count_launches(monkeypatch, hip):
    calls = {"groups": 0, "dyn": 0, "plain": 0}
    for name, key in (("adamw_groups", "groups"), ("adamw_dyn", "dyn"), ("adamw", "plain")):
        real = getattr(hip, name)

        def wrapped(*a, _real=real, _key=key, **k):
            calls[_key] += 1
            return _real(*a, **k)

        monkeypatch.setattr(hip, name, wrapped)
    return calls


def _check_against_torch64(opt, ref, who):
    for g in opt.param_groups:
        for p in g["params"]:
            if p.grad is None:
                continue
            r = ref[id(p)]
            err = (p.detach().double() - r).abs()
            bound = 1e-6 * r.abs() + 1e-7
            assert bool((err <= bound).all()), f"{who}: max excess {(err - bound).max().item():.3e}"


def test_llrd_groups_follow_torch_float64(hip, gpu_device, monkeypatch):
    """param_groups(layer_decay=0.75) on the tiny model: three steps on real gradients, each within 1e-6 |p| + 1e-7 of a float64
    torch.optim.AdamW over the same groups, with ONE dcv_adamw_groups launch per step."""
    import diverse_channel_vit_amd as dcv
    model = build(gpu_device)
    x, y = batch(gpu_device)
    fwd_bwd(model, x, y)
    groups = dcv.param_groups(model, lr=1e-3, weight_decay=0.05, layer_decay=0.75)
    assert 20 <= len(groups) <= MAX_GROUPS
    opt = dcv.HipAdamW(groups, model=model)
    calls = _count_launches(monkeypatch, hip)
    outside = [p for p in model._all_params[len(model._enc_params):]]
    for step in range(1, 4):
        fwd_bwd(model, x, y)
        with_grad = {id(p) for g in opt.param_groups for p in g["params"] if p.grad is not None}
        ref = _torch64_step(opt, {i: step for i in with_grad})
        before = dict(calls)
        opt.step()
        assert calls["groups"] - before["groups"] == 1 and calls["plain"] == 0
        assert calls["dyn"] - before["dyn"] == sum(1 for p in outside if id(p) in with_grad)
        _check_against_torch64(opt, ref, f"step {step}")
        assert all(opt.state[p]["step"] == step for g in opt.param_groups for p in g["params"] if p.grad is not None)
    torch.cuda.synchronize()


def test_frozen_prefix_in_the_optimizer_and_gradual_unfreezing(hip, gpu_device, monkeypatch):
    """freeze_prefix(8): one grouped launch plus one per trainable parameter outside the encoder range; frozen parameters keep their bits
    and get no state.  Gradual unfreezing, one group per freeze unit: block 7 is frozen for steps 1-2 and trainable from step 3; its
    state[p]["step"] counts from its first update, as torch's per-parameter count does, and every step follows torch float64."""
    import diverse_channel_vit_amd as dcv
    model = build(gpu_device)
    x, y = batch(gpu_device)
    fwd_bwd(model, x, y)
    model.freeze_prefix(8)
    blk7 = list(model.feature_extractor.blocks[7].parameters())
    rest = [p for p in model.parameters() if p.requires_grad]
    assert rest and all(p.requires_grad is False for p in blk7)
    frozen = [p for p in model.parameters() if not p.requires_grad]
    snap = [p.detach().clone() for p in frozen]
    opt = dcv.HipAdamW([dict(params=rest), dict(params=blk7, lr=3e-4, weight_decay=0.0)], lr=1e-3, weight_decay=0.05, model=model)
    calls = _count_launches(monkeypatch, hip)
    outside = model._all_params[len(model._enc_params):]
    taken = {}
    for step in range(1, 5):
        if step == 3:
            for p in blk7:
                p.requires_grad_(True)
        fwd_bwd(model, x, y)
        live = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
        assert all((p.grad is not None) == (step >= 3) for p in blk7)
        for p in live:
            taken[id(p)] = taken.get(id(p), 0) + 1
        ref = _torch64_step(opt, taken)
        before = dict(calls)
        opt.step()
        assert calls["groups"] - before["groups"] == 1 and calls["plain"] == 0
        assert calls["dyn"] - before["dyn"] == sum(1 for p in outside if p.grad is not None)
        _check_against_torch64(opt, ref, f"step {step}")
        for p in live:
            assert opt.state[p]["step"] == taken[id(p)]
        if step == 2:
            assert all(p not in opt.state or not opt.state[p] for p in blk7)
            for p, s in zip(frozen, snap):
                assert torch.equal(_bits(p.detach()), _bits(s))
    assert all(opt.state[p]["step"] == 2 for p in blk7) and opt.state[model.feature_extractor.norm.weight]["step"] == 4
    assert all(opt.state[p]["step"] == 4 for p in rest if p.grad is not None)  # `proxies` has no gradient in this loss, hence no state
    still = [(p, s) for p, s in zip(frozen, snap) if not any(p is q for q in blk7)]
    for p, s in still:
        assert torch.equal(_bits(p.detach()), _bits(s)) and (p not in opt.state or not opt.state[p])


@pytest.fixture(scope="module")
def full_run(gpu_device):
    """The unfrozen model's logits, loss and gradients on the shared batch (nearest rounding), computed once."""
    model = build(gpu_device)
    model.stochastic_weight_rounding = False
    x, y = batch(gpu_device)
    out, loss = fwd_bwd(model, x, y)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return out, loss, grads


def _same_as_full(model, out, loss, ref):
    o_ref, l_ref, g_ref = ref
    assert torch.equal(_bits(out), _bits(o_ref)) and torch.equal(_bits(loss), _bits(l_ref))
    n = 0
    for name, p in model.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, name
            continue
        if name not in g_ref:
            assert p.grad is None, name
            continue
        assert p.grad is not None and torch.equal(_bits(p.grad), _bits(g_ref[name])), name
        n += 1
    return n


@pytest.mark.parametrize("k", [1, 6, 11, 12])
def test_truncated_backward_matches_the_full_one(gpu_device, full_run, k):
    """freeze_prefix(k): logits and loss are the unfrozen model's bits, every trainable parameter's gradient is the full backward's bits,
    frozen parameters have none, and nothing of blocks < k is kept (st["layers"][i] holds the DropPath factors only)."""
    model = build(gpu_device)
    model.stochastic_weight_rounding = False
    model.freeze_prefix(k)
    x, y = batch(gpu_device)
    out, loss = fwd_bwd(model, x, y)
    n = _same_as_full(model, out, loss, full_run)
    assert n == 12 * (12 - k) + 2 + 2  # the blocks above, the final norm, the head


def _memory_of(model, x, y):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fwd_bwd(model, x, y)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_truncated_backward_saves_memory_and_yields_to_upstream_gradients(gpu_device, full_run):
    """Peak memory over forward + backward is strictly lower at k = 6 than at k = 0.  When x requires a gradient, or the positional table is
    trainable, block 6 is no frozen prefix: the full backward runs and every gradient is the unfrozen run's."""
    model = build(gpu_device)
    model.stochastic_weight_rounding = False
    x, y = batch(gpu_device)
    fwd_bwd(model, x, y)  # arenas and workspaces exist from here on
    m0 = _memory_of(model, x, y)
    model.freeze_prefix(6)
    m6 = _memory_of(model, x, y)
    print(f"peak memory of forward + backward: k = 0 {m0} B, k = 6 {m6} B")
    assert m6 < m0
    # x requires a gradient
    ref_model = build(gpu_device)
    ref_model.stochastic_weight_rounding = False
    xr = x.clone().requires_grad_(True)
    fwd_bwd(ref_model, xr, y)
    xg = x.clone().requires_grad_(True)
    out, loss = fwd_bwd(model, xg, y)
    _same_as_full(model, out, loss, full_run)
    assert xg.grad is not None and torch.equal(_bits(xg.grad), _bits(xr.grad))
    # the positional table is trainable
    pos = model.feature_extractor.pos_embed
    pos.requires_grad_(True)
    out, loss = fwd_bwd(model, x, y)
    _same_as_full(model, out, loss, full_run)
    assert torch.equal(_bits(pos.grad), _bits(full_run[2]["feature_extractor.pos_embed"]))


def test_truncated_backward_with_drop_path_and_token_dropout(gpu_device):
    """k = 6 again with drop_path_rate > 0 (pinned masks: the factors of the frozen block 5 are still what block 6's norm1 backward
    multiplies into the copy for the block below) and with dropout_tokens_hcs = "random" (python RNG seeded alike)."""
    x, y = batch(gpu_device)

    def masks(bi, branch, B, dev):
        return torch.tensor([(bi + (branch == "mlp")) % 2, 1.0])[:B]

    for over, sampler in ((dict(drop_path_rate=0.3), masks), (dict(dropout_tokens_hcs="random"), None)):
        runs = []
        for k in (0, 6):
            model = build(gpu_device, **over)
            model.stochastic_weight_rounding = False
            model.drop_path_sampler = sampler
            if k:
                model.freeze_prefix(k)
            random.seed(1234)
            out, loss = fwd_bwd(model, x, y)
            runs.append((model, out, loss))
        (m0, o0, l0), (m6, o6, l6) = runs
        ref = (o0, l0, {n: p.grad for n, p in m0.named_parameters() if p.grad is not None})
        assert _same_as_full(m6, o6, l6, ref) == 12 * 6 + 4, over


def test_clip_grad_norm_over_runs_of_gradients(gpu_device):
    """freeze_prefix(6), then additionally ONE frozen tensor in the middle of the trainable range (its gradient is still computed into the
    arena and must stay out of the norm), against torch.nn.utils.clip_grad_norm_ over the parameters that have gradients; the bounds of
    test_clip_grad_norm_matches_torch, with and without the clip biting."""
    import diverse_channel_vit_amd as dcv
    model = build(gpu_device)
    x, y = batch(gpu_device)
    for middle in (False, True):
        model.freeze_prefix(6)
        if middle:
            model.feature_extractor.blocks[8].mlp.fc1.weight.requires_grad_(False)
        fwd_bwd(model, x, y)
        norm = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None)).item()
        for max_norm in (0.5 * norm, 2.0 * norm):  # the clip bites, and it does not
            fwd_bwd(model, x, y)
            live = [p for p in model.parameters() if p.grad is not None]
            assert len(live) == 12 * 6 + 4 - int(middle)
            twins = [torch.nn.Parameter(p.detach().clone()) for p in live]
            for t, p in zip(twins, live):
                t.grad = p.grad.detach().clone()
            raw = [t.grad.clone() for t in twins]
            tot = torch.nn.utils.clip_grad_norm_(twins, max_norm)
            got = dcv.clip_grad_norm_(model, max_norm)
            print(f"frozen tensor in the middle {middle}, max_norm {max_norm:.4g}: torch {tot.item():.8g}, HIP {got.item():.8g}")
            assert abs(got.item() - tot.item()) <= 1e-5 * tot.item(), (middle, max_norm)
            for t, p, r in zip(twins, live, raw):
                assert torch.allclose(p.grad, t.grad, rtol=1e-5, atol=1e-9), (middle, max_norm)
                assert torch.equal(t.grad, r) == (max_norm > norm)


def test_captured_multi_group_step(gpu_device):
    """GraphedTrainStep with a capturable multi-group HipAdamW: two warm-up steps and three replays equal five eager steps (bit for bit in
    the deterministic mode the suite runs in, as test_graphed_step_matches_eager); a group whose lr is set to 0 between replays stops —
    exactly its parameters keep their bits — while the others move."""
    import diverse_channel_vit_amd as dcv
    x, y = batch(gpu_device, seed=77)
    ce = torch.nn.CrossEntropyLoss()
    runs = {}
    for mode in ("eager", "graph"):
        model = build(gpu_device)
        model.stochastic_weight_rounding = False
        opt = dcv.HipAdamW(dcv.param_groups(model, lr=1e-3, weight_decay=0.05, layer_decay=0.75), model=model, capturable=(mode == "graph"))
        losses = []
        if mode == "eager":
            for _ in range(5):
                opt.zero_grad()
                out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
                loss = ce(out, y) + extra
                loss.backward()
                opt.step()
                losses.append(loss.item())
        else:
            gs = dcv.GraphedTrainStep(model, opt, "train", None, ce, 1.0, warmup=2)
            for _ in range(3):
                losses.append(gs(x, y).item())
        runs[mode] = (losses, [p.detach().clone() for p in model.parameters()], list(opt._gsteps), model, opt, gs if mode == "graph" else None)
    le, lg = runs["eager"][0], runs["graph"][0]
    assert runs["eager"][2] == runs["graph"][2] == [5] * len(runs["eager"][2])
    assert dcv.is_deterministic()
    assert le[2:] == lg
    for a, b in zip(runs["eager"][1], runs["graph"][1]):
        assert torch.equal(_bits(a), _bits(b))
    _, before, _, model, opt, gs = runs["graph"]
    stopped = 3
    opt.param_groups[stopped]["lr"] = 0.0
    gs(x, y)
    torch.cuda.synchronize()
    halted = {id(p) for p in opt.param_groups[stopped]["params"]}
    for p, old in zip(model.parameters(), before):
        if p.grad is None:
            continue
        same = torch.equal(_bits(p.detach()), _bits(old))
        assert same == (id(p) in halted), "a group with lr 0 must stop, every other group must move"
