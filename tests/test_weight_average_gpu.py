"""Weight averaging on the HIP path: dcv_avg_update bit for bit on exact operands (every size class, grid caps that make workgroups
walk rounds, guard floats around avg, p untouched), the bitwise copy at count 0, general values against float64 within a derived bound,
the count read from a device word; AveragedModel (SWA and EMA) on the tiny model against the float64 recurrence over per-step parameter
snapshots, with one launch per update; the averaged copy's forward on its own weights; training untouched; the captured step with the
update inside the graph; the checkpoint round trip and torch's own state dict; a frozen prefix; SWALR; a layout mismatch.

The launch plan of dcv_avg_update is restated here (avg_plan, from csrc/avg.hip).  Model-level tests build the tiny model of
tests/golden/tiny_e2e.npz (depth 12, 3 channels, 32 x 32, B 2).  Needs an MI355X (-m gpu)."""
from collections import namedtuple

import numpy as np
import pytest
import torch
from torch.optim import swa_utils

from conftest import load_golden
from oracle import dichavit_oracle as orc

# ---- csrc/avg.hip restated ---------------------------------------------------------------------------------------------------------
ILP, LANES, GRID_CAP = 4, 256, 2048  # DCV_AVG_ILP, workgroup size, DCV_AVG_GRID_CAP
CHUNK4 = ILP * LANES                 # float4 per chunk

AvgPlan = namedtuple("AvgPlan", "n4 tail nchunks grid rounds_min rounds_max ragged4")


def avg_plan(n, grid_cap=0):
    """n floats = n4 float4 + a scalar tail of n % 4 (workgroup 0); chunks of CHUNK4 float4, chunk c to workgroup c % grid; the last chunk
    is ragged when n4 % CHUNK4; grid = min(chunks, cap), at least 1."""
    n4 = n // 4
    nchunks = -(-n4 // CHUNK4)
    grid = max(1, min(nchunks, grid_cap if grid_cap > 0 else GRID_CAP))
    return AvgPlan(n4, n % 4, nchunks, grid, nchunks // grid, -(-nchunks // grid), n4 % CHUNK4)


# one float4 chunk past one full round of the default grid, its last chunk ragged (777 float4), and a scalar tail of 3
PAST_ONE_ROUND = 4 * (GRID_CAP * CHUNK4 + 777) + 3
SIX_CHUNKS = 4 * (5 * CHUNK4 + 300) + 2  # five full chunks and a ragged one: grid caps 1 and 3 make workgroups walk 6 and 2 rounds
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4099, SIX_CHUNKS]
GUARD = 64
SENT_BITS = 0x5A5AC3C3  # the guard floats' bit pattern

pytestmark = pytest.mark.gpu


def test_launch_arithmetic_restated():
    p = avg_plan(PAST_ONE_ROUND)
    assert (p.nchunks, p.grid, p.rounds_min, p.rounds_max, p.ragged4, p.tail) == (GRID_CAP + 1, GRID_CAP, 1, 2, 777, 3)
    assert avg_plan(SIX_CHUNKS, 1)[3:6] == (1, 6, 6) and avg_plan(SIX_CHUNKS, 3)[3:6] == (3, 2, 2) and avg_plan(SIX_CHUNKS)[3:6] == (6, 1, 1)
    assert avg_plan(3) == AvgPlan(0, 3, 0, 1, 0, 0, 0) and avg_plan(4099).nchunks == 1 and avg_plan(4099).tail == 3


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def _bits(t):
    return t.view(torch.int32)


def _guarded(n, dev):
    """A buffer of n floats inside a larger one, GUARD sentinel floats on either side (the offset keeps the 16-byte alignment)."""
    full = torch.empty(n + 2 * GUARD, dtype=torch.float32, device=dev)
    _bits(full).fill_(SENT_BITS)
    return full, full[GUARD:GUARD + n]


def _exact_operands(n, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randint(-1024, 1025, (n,), device=dev, generator=gen).float() / 256
    p = torch.randint(-1024, 1025, (n,), device=dev, generator=gen).float() / 256
    return a, p


# (mode name, count, ema weight, w): SWA counts with count + 1 a power of two up to 128, EMA weights 2^-1 .. 2^-10 at a count > 0
EXACT_WEIGHTS = [("swa", (1 << k) - 1, 0.0, 2.0 ** -k) for k in range(8)] + [("ema", 5, 2.0 ** -k, 2.0 ** -k) for k in range(1, 11)]


def _check_exact(hip, n, grid_cap):
    dev = "cuda"
    a0, p0 = _exact_operands(n, dev, 1000 + n % 997)
    full_a, a = _guarded(n, dev)
    full_p, p = _guarded(n, dev)
    p.copy_(p0)
    p_before = _bits(full_p).clone()
    for name, count, ew, w in EXACT_WEIGHTS:
        a.copy_(a0)
        hip.avg_update(a, p, n, hip.AVG_SWA if name == "swa" else hip.AVG_EMA, ema_weight=ew, n_averaged=count, grid_cap=grid_cap)
        want = (a0.double() + w * (p0.double() - a0.double())).float()  # every intermediate is exact in fp32, so this IS the fp32 result
        same = _bits(a) == _bits(want)
        assert bool(same.all()), f"n {n} cap {grid_cap} {name} count {count} w {w}: {int((~same).sum())} differ, first at {int((~same).nonzero()[0])}"
        g = _bits(full_a)
        assert bool((g[:GUARD] == SENT_BITS).all()) and bool((g[GUARD + n:] == SENT_BITS).all()), "dcv_avg_update wrote outside avg"
    assert torch.equal(_bits(full_p), p_before), "dcv_avg_update wrote to p or around it"


@pytest.mark.parametrize("grid_cap", [0, 1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_bit_for_bit_on_exact_operands(hip, n, grid_cap):
    """Operands multiples of 2^-8 in [-4, 4], weights powers of two: p - a, w (p - a) and the sum are exact in fp32, so the kernel must
    return the float64 value cast to fp32, whichever branch of the two-sided lerp it takes (w = 1/2 takes the upper one)."""
    _check_exact(hip, n, grid_cap)


def test_kernel_bit_for_bit_past_one_round_of_the_default_grid(hip):
    """GRID_CAP + 1 chunks on GRID_CAP workgroups: workgroup 0 walks twice (its second chunk is the ragged one), the others once, and
    workgroup 0 also takes the 3-float tail."""
    p = avg_plan(PAST_ONE_ROUND)
    assert p.rounds_max == 2 and p.rounds_min == 1 and p.ragged4 and p.tail
    _check_exact(hip, PAST_ONE_ROUND, 0)


@pytest.mark.parametrize("mode", ["swa", "ema"])
def test_copy_at_count_zero_is_bitwise(hip, mode):
    dev = "cuda"
    n = 4 * (CHUNK4 + 300) + 3  # a full chunk, a ragged one and the tail each hold every special value
    # -0, denormals, +-inf, NaNs with payloads (quiet and signalling), 1, -pi, +0
    special = torch.from_numpy(np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFA00001, 0x7F812345,
                                         0x3F800000, 0xC0490FDB, 0x00000000], dtype=np.uint32).view(np.int32)).to(dev)
    p = torch.randn(n, device=dev)
    pb = _bits(p)
    for start in (0, 5, 4 * CHUNK4 + 2, n - special.numel()):
        pb[start:start + special.numel()] = special
    full_a, a = _guarded(n, dev)
    a.fill_(1.25)
    before = pb.clone()
    hip.avg_update(a, p, n, hip.AVG_SWA if mode == "swa" else hip.AVG_EMA, ema_weight=0.0 if mode == "swa" else 0.001, n_averaged=0)
    assert torch.equal(_bits(a), before) and torch.equal(pb, before)
    g = _bits(full_a)
    assert bool((g[:GUARD] == SENT_BITS).all()) and bool((g[GUARD + n:] == SENT_BITS).all())


def test_kernel_general_values_against_float64(hip):
    """a ~ 0.05 N(0,1), p = a + 1e-3 N(0,1); the reference is float64 with the same fp32 weight.  Bound 3 * 2^-24 * max(|a|, |p|) per
    element, derived: d = p - a is rounded once (|d| <= 2 max, times w < 1/2 or 1 - w <= 1/2: at most 2^-24 max), the fused multiply-add
    once (the result is a convex combination, so at most 2^-24 max again), 1 - w is exact for w in [1/2, 1]; 2 of the 3 units are used."""
    dev = "cuda"
    n = (1 << 20) + 4 * 333 + 3
    gen = torch.Generator(device=dev).manual_seed(7)
    a0 = 0.05 * torch.randn(n, device=dev, generator=gen)
    p = a0 + 1e-3 * torch.randn(n, device=dev, generator=gen)
    bound = 3 * 2.0 ** -24 * torch.maximum(a0.abs(), p.abs()).double()
    cases = [("swa", c, 0.0, float(np.float32(1) / np.float32(c + 1))) for c in (1, 2, 4, 99, 12344)]
    cases += [("ema", 3, float(1.0 - d), float(np.float32(1.0 - d))) for d in (0.9, 0.999, 0.9999)]
    for name, count, ew, w in cases:
        a = a0.clone()
        hip.avg_update(a, p, n, hip.AVG_SWA if name == "swa" else hip.AVG_EMA, ema_weight=ew, n_averaged=count)
        want = a0.double() + w * (p.double() - a0.double())
        err = (a.double() - want).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{name} count {count} w {w:.9g}: worst error / bound = {worst:.3f}")
        assert bool((err <= bound).all()), (name, count, worst)


@pytest.mark.parametrize("mode", ["swa", "ema"])
def test_count_from_a_device_word(hip, mode):
    dev = "cuda"
    n = 4 * (2 * CHUNK4 + 77) + 1
    gen = torch.Generator(device=dev).manual_seed(11)
    a0, p = torch.randn(n, device=dev, generator=gen), torch.randn(n, device=dev, generator=gen)
    m, ew = (hip.AVG_SWA, 0.0) if mode == "swa" else (hip.AVG_EMA, 0.1)
    for count in range(6):
        word = torch.tensor([count, -99], dtype=torch.int64, device=dev)  # the neighbour word is not the kernel's business
        by_value, by_word = a0.clone(), a0.clone()
        hip.avg_update(by_value, p, n, m, ema_weight=ew, n_averaged=count)
        hip.avg_update(by_word, p, n, m, ema_weight=ew, n_averaged=12345, n_averaged_dev=word[0])  # the by-value count is ignored
        assert torch.equal(_bits(by_value), _bits(by_word)), count
        assert word.tolist() == [count, -99]
        assert torch.equal(_bits(by_value), _bits(p)) == (count == 0)


# ---- model level ---------------------------------------------------------------------------------------------------------------------
class Cfg(dict):
    """A DictConfig stand-in that copy.deepcopy can take apart (dunder lookups are not keys)."""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return self.get(k)


def build(device, num_classes=None, **cfg_over):
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("tiny_e2e")
    K = meta["num_classes"] if num_classes is None else num_classes
    cfgd = dict(meta["cfg"], **cfg_over)
    cfg = Cfg(cfgd, in_channel_names=[f"c{i}" for i in range(meta["n_channels"])], img_size=[meta["img"]], num_classes=K)
    model = dcv.dichavit(cfg, mapper={k: list(v) for k, v in meta["mapper"].items()})
    st = orc.make_state(orc.state_shapes(meta["cfg"], meta["n_channels"], meta["img"], K), meta["seed"])
    model.load_state_dict({**st, "adaptive_interface.0": st["proxies"]}, strict=True)
    model = model.to(device).train()
    model.stochastic_weight_rounding = False
    assert len(model.feature_extractor.blocks) == 12
    return model


def batch(device, seed=3):
    x, y = orc.make_batch(seed, 2, 3, 32, 5)
    return x.to(device), y.to(device)


CE = torch.nn.CrossEntropyLoss()
LR, WD, EMA_DECAY = 1e-3, 0.05, 0.9


def step(model, opt, x, y):
    opt.zero_grad()
    if opt.capturable:
        opt.advance()
    out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    loss = CE(out, y) + extra
    loss.backward()
    opt.step()


def named(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}


Run = namedtuple("Run", "model opt averaged snaps calls")


def eager_run(device, kind, steps=5, averager=True, hip=None, prepare=None, capturable=False):
    """`steps` eager HipAdamW steps on the shared batch with update_parameters after each; a snapshot of every parameter after each
    step; the calls of hip.avg_update counted per update."""
    import diverse_channel_vit_amd as dcv
    model = build(device)
    if prepare is not None:
        prepare(model)
    x, y = batch(device)
    opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=LR, weight_decay=WD, model=model, capturable=capturable)
    avg = dcv.AveragedModel(model, avg=kind, decay=EMA_DECAY) if averager else None
    snaps, calls = [], []
    with pytest.MonkeyPatch.context() as mp:
        n_calls = [0]
        if hip is not None:
            real = hip.avg_update

            def counted(*a, **k):
                n_calls[0] += 1
                return real(*a, **k)

            mp.setattr(hip, "avg_update", counted)
        for _ in range(steps):
            step(model, opt, x, y)
            if avg is not None:
                before = n_calls[0]
                avg.update_parameters(model)
                calls.append(n_calls[0] - before)
            snaps.append(named(model))
    torch.cuda.synchronize()
    return Run(model, opt, avg, snaps, calls)


@pytest.fixture(scope="module")
def runs(gpu_device, hip):
    """Five eager steps with an update after each, once per averaging rule, shared (read-only) by the tests below."""
    return {kind: eager_run(gpu_device, kind, hip=hip) for kind in ("swa", "ema")}


def expected_average(snaps, kind):
    """The float64 recurrence over the snapshots with the fp32 weights the kernel uses: the first update copies."""
    exp = {n: t.double() for n, t in snaps[0].items()}
    for k in range(1, len(snaps)):
        w = float(np.float32(1) / np.float32(k + 1)) if kind == "swa" else float(np.float32(1.0 - EMA_DECAY))
        for n, t in snaps[k].items():
            exp[n] = exp[n] + w * (t.double() - exp[n])
    return exp


@pytest.mark.parametrize("kind", ["swa", "ema"])
def test_model_average_follows_the_float64_recurrence(runs, kind):
    """Every named parameter of averaged.module — the head, `proxies`, the channel-embedding and positional tables outside the encoder
    range included — within 5 * 3 * 2^-24 * max|snapshots| of the float64 recurrence (five updates of the kernel's derived per-update
    bound); n_averaged == 5; exactly one dcv_avg_update per update."""
    r = runs[kind]
    assert r.calls == [1] * 5 and int(r.averaged.n_averaged) == 5 and r.averaged.n_averaged.is_cuda
    exp = expected_average(r.snaps, kind)
    got = dict(r.averaged.module.named_parameters())
    assert set(got) == set(exp) and len(got) > 150
    for must in ("classifer_head.weight", "proxies", "feature_extractor.pos_embed", "feature_extractor.patch_embed.channel_embed.weight"):
        assert must in got
    moved = 0
    for n, e in exp.items():
        bound = 5 * 3 * 2.0 ** -24 * max(float(s[n].abs().max()) for s in r.snaps)
        err = float((got[n].detach().double() - e).abs().max())
        assert err <= bound, f"{kind} {n}: {err:.3e} > {bound:.3e}"
        moved += int(not torch.equal(r.snaps[0][n], r.snaps[-1][n]))
    assert moved > 140  # the average is over weights that actually moved
    assert not torch.equal(got["classifer_head.weight"], r.snaps[-1]["classifer_head.weight"])


def test_the_copy_runs_on_its_own_weights(runs, gpu_device):
    r = runs["swa"]
    x, _ = batch(gpu_device)
    mine = r.averaged.module
    was = mine.training
    with torch.no_grad():
        out_avg = mine.eval()(x, "train", None).clone()
        out_wrapped = r.averaged(x, "train", None).clone()  # forward() is the copy's forward
        mine.train(was)
        fresh = build(gpu_device)
        fresh.load_state_dict(mine.state_dict(), strict=True)
        out_fresh = fresh.eval()(x, "train", None).clone()
        r.model.eval()
        out_model = r.model(x, "train", None).clone()
        r.model.train()
    assert torch.equal(_bits(out_avg), _bits(out_fresh)) and torch.equal(_bits(out_avg), _bits(out_wrapped))
    assert not torch.equal(out_avg, out_model) and not torch.equal(out_fresh, out_model)
    assert mine._arena is not None and mine._arena.data_ptr() != r.model._arena.data_ptr()
    assert mine.feature_extractor._owner() is mine and mine._dp is None


def test_training_is_untouched(runs, gpu_device):
    without = eager_run(gpu_device, "swa", averager=False)
    for kind in ("swa", "ema"):
        for (n, a), (_, b) in zip(runs[kind].model.named_parameters(), without.model.named_parameters()):
            assert torch.equal(_bits(a.detach()), _bits(b.detach())), (kind, n)


@pytest.mark.parametrize("kind", ["swa", "ema"])
def test_captured_step_with_the_update_inside(runs, gpu_device, kind):
    """GraphedTrainStep(..., averager=avg, warmup=2) called three times = two warm-up steps + three replays = five eager steps with an
    update after each: the model's and the averaged parameters bit for bit (deterministic mode), n_averaged == 5 in both."""
    import diverse_channel_vit_amd as dcv
    assert dcv.is_deterministic()
    model = build(gpu_device)
    x, y = batch(gpu_device)
    opt = dcv.HipAdamW(list(model.parameters()), lr=LR, weight_decay=WD, model=model, capturable=True)
    avg = dcv.AveragedModel(model, avg=kind, decay=EMA_DECAY)
    gs = dcv.GraphedTrainStep(model, opt, "train", None, CE, 1.0, warmup=2, averager=avg)
    for _ in range(3):
        gs(x, y)
    torch.cuda.synchronize()
    r = runs[kind]
    assert int(avg.n_averaged) == 5 == int(r.averaged.n_averaged)
    for (n, a), (_, b) in zip(model.named_parameters(), r.model.named_parameters()):
        assert torch.equal(_bits(a.detach()), _bits(b.detach())), ("model", n)
    for (n, a), (_, b) in zip(avg.module.named_parameters(), r.averaged.module.named_parameters()):
        assert torch.equal(_bits(a.detach()), _bits(b.detach())), ("averaged", n)


def test_checkpoint_round_trip_and_torchs_state_dict(runs, gpu_device, tmp_path):
    import diverse_channel_vit_amd as dcv
    x, y = batch(gpu_device)
    a = eager_run(gpu_device, "ema", steps=2)
    path = str(tmp_path / "ckpt.pt")
    dcv.save_checkpoint(path, a.model, a.opt, epoch=2, averaged=a.averaged)
    model = build(gpu_device)
    opt = dcv.HipAdamW(list(model.parameters()), lr=LR, weight_decay=WD, model=model)
    avg = dcv.AveragedModel(model, avg="ema", decay=EMA_DECAY)
    assert dcv.load_checkpoint(path, model, opt, averaged=avg) == 2 and int(avg.n_averaged) == 2
    for m, o, v in ((a.model, a.opt, a.averaged), (model, opt, avg)):
        step(m, o, x, y)
        v.update_parameters(m)
    assert int(avg.n_averaged) == 3 == int(a.averaged.n_averaged)
    for (n, p), (_, q) in zip(model.named_parameters(), a.model.named_parameters()):
        assert torch.equal(_bits(p.detach()), _bits(q.detach())), ("model", n)
    for (n, p), (_, q) in zip(avg.module.named_parameters(), a.averaged.module.named_parameters()):
        assert torch.equal(_bits(p.detach()), _bits(q.detach())), ("averaged", n)
    assert not torch.equal(avg.module.classifer_head.weight, model.classifer_head.weight)
    # torch's own class, fed the same five snapshots on the CPU: its state dict loads into ours and holds the same average
    r = runs["swa"]
    twin = build(torch.device("cpu"))
    theirs = swa_utils.AveragedModel(twin)
    for snap in r.snaps:
        twin.load_state_dict({k: v.cpu() for k, v in snap.items()}, strict=False)
        theirs.update_parameters(twin)
    ours = dcv.AveragedModel(build(gpu_device))
    ours.load_state_dict(theirs.state_dict(), strict=True)
    assert int(ours.n_averaged) == 5
    for (n, p), (_, q) in zip(ours.module.named_parameters(), r.averaged.module.named_parameters()):
        bound = 5 * 3 * 2.0 ** -24 * max(float(s[n].abs().max()) for s in r.snaps)
        assert float((p.detach().double() - q.detach().double()).abs().max()) <= 2 * bound, n  # each within `bound` of the float64 recurrence


def test_frozen_prefix(gpu_device):
    """freeze_prefix(6), three steps with updates: the average of a parameter that never moves is that parameter, bit for bit; the
    parameters that take gradients differ from their average."""
    r = eager_run(gpu_device, "swa", steps=3, prepare=lambda m: m.freeze_prefix(6))
    frozen = trained = 0
    avg_params = dict(r.averaged.module.named_parameters())
    for n, p in r.model.named_parameters():
        same = torch.equal(_bits(p.detach()), _bits(avg_params[n].detach()))
        if not p.requires_grad:
            assert same, n
            assert torch.equal(_bits(p.detach()), _bits(r.snaps[0][n]))
            frozen += 1
        elif p.grad is not None:
            assert not same, n
            trained += 1
    assert frozen >= 6 * 12 + 5 and trained == 6 * 12 + 4


def test_swalr_drives_the_capturable_optimizer(gpu_device):
    """SWALR only edits param_groups[i]["lr"]: stepped once with swa_lr = 0 and anneal_epochs = 1 the lr is 0, and one further step of a
    capturable HipAdamW leaves every parameter bit-identical — the optimizer reads the scheduler's value."""
    r = eager_run(gpu_device, "swa", steps=1, averager=False, capturable=True)
    x, y = batch(gpu_device)
    sched = swa_utils.SWALR(r.opt, swa_lr=0.0, anneal_epochs=1)
    sched.step()
    assert all(g["lr"] == 0.0 for g in r.opt.param_groups)
    before = named(r.model)
    step(r.model, r.opt, x, y)
    torch.cuda.synchronize()
    for n, p in r.model.named_parameters():
        assert torch.equal(_bits(p.detach()), _bits(before[n])), n
    assert not torch.equal(before["classifer_head.weight"], build(gpu_device).classifer_head.weight)  # the first step, at lr 1e-3, did move


def test_layout_mismatch_is_refused_before_any_launch(gpu_device, hip, monkeypatch):
    import diverse_channel_vit_amd as dcv
    model = build(gpu_device)
    other = dcv.AveragedModel(build(gpu_device, num_classes=7))
    calls = []
    monkeypatch.setattr(hip, "avg_update", lambda *a, **k: calls.append(a))
    with pytest.raises(ValueError, match="not the same architecture"):
        other.update_parameters(model)
    assert not calls and int(other.n_averaged) == 0
