"""Model-level parity of the HIP path (through the reference's plugin surface) against
  (1) the golden vectors captured from the REAL reference (tests/golden/*.npz, fp32 CPU), and
  (2) the oracle (fp64 CPU restatement, itself pinned to those goldens) for every parameter gradient.

Stated tolerance (north_star: "within a stated bf16/fp32 tolerance"): activations are bf16
(8 significant bits), every accumulation / statistic / residual is fp32.  We require
  logits: |err| <= 3e-2 * max|logits| ;  losses: |err| <= 5e-3 (abs) ;
  per-parameter gradient: relative L2 error <= 5e-2 and cosine >= 0.998 (tensors with norm above a floor).
Needs an MI355X (-m gpu)."""
import math
import os
import random

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import dichavit_oracle as orc

pytestmark = pytest.mark.gpu


class Cfg(dict):
    __getattr__ = dict.get


def build(meta, device, train=True):
    import diverse_channel_vit_amd as dcv
    cfg = Cfg(meta["cfg"], in_channel_names=[f"c{i}" for i in range(meta["n_channels"])], img_size=[meta["img"]],
              num_classes=meta["num_classes"])
    model = dcv.dichavit(cfg, mapper={k: list(v) for k, v in meta["mapper"].items()})
    shapes = orc.state_shapes(meta["cfg"], meta["n_channels"], meta["img"], meta["num_classes"], chammi="Allen" in meta["mapper"])
    st = orc.make_state(shapes, meta["seed"])
    sd = model.state_dict()
    assert set(sd.keys()) - {"adaptive_interface.0"} == set(st.keys())
    model.load_state_dict({**st, "adaptive_interface.0": st["proxies"]}, strict=True)
    model = model.to(device)
    model.train(train)
    return model, st


def oracle_grads(meta, x, y, ch, idx, chammi=False):
    shapes = orc.state_shapes(meta["cfg"], meta["n_channels"], meta["img"], meta["num_classes"], chammi="Allen" in meta["mapper"])
    sd = orc.make_state(shapes, meta["seed"], dtype=torch.float64)
    for v in sd.values():
        v.requires_grad_(True)
    fn = orc.chammi_loss if chammi else orc.train_loss
    loss, main, extra, out = fn(sd, x.double(), y, meta["cfg"], ch, idx)
    loss.backward()
    return sd, loss.item(), extra.item(), out.detach()


def check_grads(model, sd_ref, rel_tol=5e-2, cos_tol=0.998):
    worst = (0.0, None)
    n = 0
    for name, p in model.named_parameters():
        if name.startswith("adaptive_interface"):
            continue
        ref = sd_ref[name].grad
        if ref is None:
            assert p.grad is None, f"{name}: expected no grad"
            continue
        assert p.grad is not None, f"{name}: missing grad"
        g = p.grad.detach().double().cpu()
        rn = ref.norm().item()
        if rn < 1e-7:
            assert g.norm().item() < 1e-5
            continue
        rel = (g - ref).norm().item() / rn
        cos = (g * ref).sum().item() / (g.norm().item() * rn + 1e-30)
        if rel > worst[0]:
            worst = (rel, name)
        assert rel <= rel_tol and cos >= cos_tol, f"{name}: rel L2 err {rel:.3e}, cos {cos:.5f}"
        n += 1
    assert n > 100
    return worst


@pytest.mark.parametrize("name", ["tiny_e2e", "so2sat_s", "jumpcp_s", "so2sat_s/fused_ln", "jumpcp_s/fused_ln"])
def test_train_step_parity(gpu_device, name):
    """One train step against the real reference's golden and, gradient by gradient, against the fp64 oracle.  The `/fused_ln` variants force the
    forward LayerNorm into the residual GEMMs' epilogue (dcv_gemm_nt_resid_ln) at these small row counts, where it is off by default
    (model.fuse_ln_min_tiles): same goldens, same tolerances; `jumpcp_s_b16` and the bench-grid tests run it at its default size."""
    name, _, variant = name.partition("/")
    meta, a = load_golden(name)
    model, _ = build(meta, gpu_device)
    if variant == "fused_ln":
        model.fuse_ln_min_tiles = 0
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    out, extra = model(x.to(gpu_device), meta["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    assert extra.shape == torch.Size([])
    main = torch.nn.CrossEntropyLoss()(out, y.to(gpu_device))
    loss = main + 1.0 * extra
    loss.backward()
    lg = a["logits"]
    assert np.abs(out.detach().cpu().numpy() - lg).max() <= 3e-2 * np.abs(lg).max(), np.abs(out.detach().cpu().numpy() - lg).max()
    assert abs(extra.item() - float(a["extra"])) <= 2e-2 * abs(float(a["extra"])) + 1e-6
    assert abs(loss.item() - float(a["loss"])) <= 5e-3
    # golden gradient norms from the real reference
    for k, v in a.items():
        if k.startswith("gnorm/"):
            p = dict(model.named_parameters())[k[6:]]
            gn = float(v)
            if gn > 1e-6:
                assert abs(p.grad.norm().item() - gn) <= 5e-2 * gn, (k, p.grad.norm().item(), gn)
    assert model.proxies.grad is None
    # every gradient tensor against the oracle
    ch = meta["mapper"][meta["chunk"]]
    sd_ref, loss_ref, extra_ref, out_ref = oracle_grads(meta, x, y, ch, list(range(len(ch))))
    worst = check_grads(model, sd_ref)
    print(f"{name}: loss {loss.item():.6f} (ref {loss_ref:.6f}) worst grad rel err {worst}")


def test_no_channel_embed_mode(gpu_device):
    """use_channelvit_channels=False (VERDICT r2 missing 7; models/dichavit.py:83-95, 121, 409): the model has no channel_embed parameter
    (state dict without that key), the tokeniser adds no channel offset; one train step against the real reference's golden and the oracle;
    and the combinations the reference itself cannot run in this mode fail the same way."""
    meta, a = load_golden("nochannel_embed")
    model, _ = build(meta, gpu_device)
    assert not any("channel_embed" in k for k in model.state_dict())
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    out, extra = model(x.to(gpu_device), meta["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    loss = torch.nn.CrossEntropyLoss()(out, y.to(gpu_device)) + extra
    loss.backward()
    lg = a["logits"]
    assert np.abs(out.detach().cpu().numpy() - lg).max() <= 3e-2 * np.abs(lg).max()
    assert abs(extra.item() - float(a["extra"])) <= 2e-2 * abs(float(a["extra"])) + 1e-6
    assert abs(loss.item() - float(a["loss"])) <= 5e-3
    _golden_grad_check(model, a)
    ch = meta["mapper"][meta["chunk"]]
    sd_ref, *_ = oracle_grads(meta, x, y, ch, list(range(len(ch))))
    check_grads(model, sd_ref)
    # random channel subsets (enable_sample, hcs_sampling = none) work without embeddings ...
    model.feature_extractor.patch_embed.enable_sample = True
    random.seed(5)
    o2, _ = model(x.to(gpu_device), meta["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    assert o2.shape == out.shape
    # ... embedding-driven sampling does not (the reference asserts, :150-152), nor does the proxy term (unbound channel_embed, :399-402)
    model.cfg["hcs_sampling"] = "lowest_cosine_prob"
    with pytest.raises(AssertionError):
        model(x.to(gpu_device), meta["chunk"], None)
    model.cfg["hcs_sampling"] = "none"
    model.cfg["proxy_loss_lambda"] = 0.001
    with pytest.raises(UnboundLocalError):
        model(x.to(gpu_device), meta["chunk"], None)


def test_drop_path_in_a_captured_step_draws_new_masks(gpu_device):
    """drop_path_rate > 0 under GraphedTrainStep: the keep masks come from torch.rand on the device generator inside the captured region, which
    torch.cuda.graph advances per replay.  With the learning rate at zero, stochastic weight rounding off and the same batch every time,
    the replayed losses can differ through the masks only — they must differ, and eager steps from the same weights must span the same
    range.  A pinned drop_path_sampler (host-made masks) is refused at construction."""
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("drop_path")
    model, _ = build(meta, gpu_device)
    model.stochastic_weight_rounding = False
    opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=0.0, weight_decay=0.0, model=model, capturable=True)
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    x, y = x.to(gpu_device), y.to(gpu_device)
    model.drop_path_sampler = lambda bi, br, B, dev: torch.ones(B)
    with pytest.raises(ValueError):
        dcv.GraphedTrainStep(model, opt, meta["chunk"], None, torch.nn.CrossEntropyLoss(), 1.0)
    model.drop_path_sampler = None
    gs = dcv.GraphedTrainStep(model, opt, meta["chunk"], None, torch.nn.CrossEntropyLoss(), 1.0)
    torch.manual_seed(5)
    losses = [gs(x, y).item() for _ in range(8)]
    assert len({round(v, 6) for v in losses[1:]}) >= 4, losses  # replays (after the capturing call) draw different masks
    eager = []
    for _ in range(8):
        opt.zero_grad()
        out, extra = model(x, meta["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        eager.append((torch.nn.CrossEntropyLoss()(out, y) + extra).item())
    lo, hi = min(eager), max(eager)
    assert all(lo - 0.5 * (hi - lo) - 1e-3 <= v <= hi + 0.5 * (hi - lo) + 1e-3 for v in losses), (losses, eager)


def test_drop_path_parity(gpu_device):
    """drop_path_rate = 0.4 (VERDICT r2 missing 6; stochastic depth, vit.py:37-56, 397-398; per-block rates linspace(0, rate, depth)): one
    train step with the keep masks the REAL reference drew (tests/golden/drop_path.npz; injected through model.drop_path_sampler, as the
    HCS subsets are) against its logits, losses and every gradient, and against the oracle with the same masks.  Forward: the residual
    epilogues multiply the branch by keep_b / keep_prob; backward: the bf16 copy of the stream's gradient that feeds a branch carries
    the same factor (dcv_ln_bwd_scaled)."""
    meta, a = load_golden("drop_path")
    model, _ = build(meta, gpu_device)
    model.stochastic_weight_rounding = False
    rates = model.feature_extractor.drop_path_rates
    assert rates[0] == 0.0 and abs(rates[-1] - 0.4) < 1e-6
    order = [(bi, br) for bi, r in enumerate(rates) if r > 0 for br in ("attn", "mlp")]
    masks = {k: torch.from_numpy(a["keep"][i]) for i, k in enumerate(order)}
    asked = []

    def sampler(bi, branch, B, dev):
        asked.append((bi, branch))
        return masks[(bi, branch)]

    model.drop_path_sampler = sampler
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    out, extra = model(x.to(gpu_device), meta["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    assert asked == order  # the reference's draw order: every block with a non-zero rate, attention branch first
    loss = torch.nn.CrossEntropyLoss()(out, y.to(gpu_device)) + extra
    loss.backward()
    lg = a["logits"]
    assert np.abs(out.detach().cpu().numpy() - lg).max() <= 3e-2 * np.abs(lg).max()
    assert abs(loss.item() - float(a["loss"])) <= 5e-3
    _golden_grad_check(model, a)
    shapes = orc.state_shapes(meta["cfg"], meta["n_channels"], meta["img"], meta["num_classes"])
    sd = orc.make_state(shapes, meta["seed"], dtype=torch.float64)
    for v in sd.values():
        v.requires_grad_(True)
    ch = meta["mapper"][meta["chunk"]]
    l_ref, *_ = orc.train_loss(sd, x.double(), y, meta["cfg"], ch, list(range(len(ch))), drop_masks=[masks[k] for k in order])
    l_ref.backward()
    check_grads(model, sd)
    # eval mode: no drop, no draw
    model.eval()
    asked.clear()
    with torch.inference_mode():
        oe = model(x.to(gpu_device), meta["chunk"], None)
    assert not asked
    ref_eval, _ = orc.forward({k: v.detach() for k, v in sd.items()}, x.double(), meta["cfg"], ch, list(range(len(ch))))
    assert (oe.cpu().double() - ref_eval).abs().max().item() <= 3e-2 * ref_eval.abs().max().item()
    # the default sampler: Bernoulli(keep_prob) masks on the device, scaled by 1 / keep_prob
    model.train()
    model.drop_path_sampler = None
    torch.manual_seed(0)
    sc = model._drop_path_scales(4096, gpu_device)
    assert sc[0] is None
    for bi in (1, 6, 11):
        keep = 1.0 - rates[bi]
        for t in sc[bi]:
            vals = t.unique().cpu().numpy()
            assert all(min(abs(v), abs(v - 1.0 / keep)) < 1e-5 for v in vals) and abs((t > 0).float().mean().item() - keep) < 0.04


def test_gradient_accumulation_keeps_the_arena(gpu_device):
    """the second and later backward passes of an optimiser step write into a scratch arena that autograd adds into .grad, so
    .grad keeps aliasing model._grad_arena and HipAdamW / clip_grad_norm_ stay on their one-launch paths; the accumulated gradient equals
    the sum of the single-pass gradients, and the fused update equals per-parameter updates."""
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("so2sat_s")
    batches = [orc.make_batch(900 + i, 4, 18, 32, 17) for i in range(3)]
    ce = torch.nn.CrossEntropyLoss()

    def run(model, idx):
        for i in idx:
            x, y = batches[i]
            out, extra = model(x.to(gpu_device), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
            (ce(out, y.to(gpu_device)) + extra).backward()

    model, _ = build(meta, gpu_device)
    model.stochastic_weight_rounding = False
    run(model, [0, 1, 2])
    ga = model._grad_arena
    assert model._grad_scratch is not None
    for p, o in zip(model._enc_params, model._enc_off):
        assert p.grad is not None and p.grad.data_ptr() == ga.data_ptr() + 4 * o
    acc = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    singles = None
    for i in range(3):
        m2, _ = build(meta, gpu_device)
        m2.stochastic_weight_rounding = False
        run(m2, [i])
        g = {n: p.grad.detach().clone() for n, p in m2.named_parameters() if p.grad is not None}
        singles = g if singles is None else {n: singles[n] + g[n] for n in g}
    for n, g in acc.items():
        assert (g - singles[n]).abs().max().item() <= 1e-5 * singles[n].abs().max().item() + 1e-9, n
    # the optimiser sees arena-aliased gradients: one fused launch; compare with torch's AdamW on copies
    ref_params = {n: p.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.04, model=model)
    opt.step()
    for n, p in model.named_parameters():
        if n not in acc:
            continue
        q = torch.nn.Parameter(ref_params[n].clone())
        q.grad = acc[n].clone()
        torch.optim.AdamW([q], lr=1e-3, weight_decay=0.04).step()
        assert (p.detach() - q.detach()).abs().max().item() <= 2e-6, n


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
def test_hcs_subsets_parity(gpu_device, rounding):
    """Six recorded HCS draws (1 .. 6 of 6 channels) against the reference's outputs.  Loss tolerance: 5e-3 with round-to-nearest weight copies
    (measured 1e-4 .. 2.1e-3).  With the default STOCHASTIC copies one forward carries twice the weight-rounding variance (unbiased: it averages
    out over steps, which is why the loss curves are 10x closer with it): the six draws measured 5e-4 .. 5.1e-3 in round 4, the largest on the
    single-channel draw (17 tokens); it had been 4.88e-3 — 98 % of the old common bound — before the forward LayerNorm moved into the residual
    GEMM's epilogue, which changes 0.2 % of the bf16 LayerNorm outputs by one ulp.  A one-step loss with stochastic copies is therefore held to
    1e-2 (4 sigma of the measured spread), the gradient and logit bounds are common to both modes."""
    meta, a = load_golden("hcs")
    model, _ = build(meta, gpu_device)
    model.stochastic_weight_rounding = rounding == "stochastic"
    loss_tol = 5e-3 if rounding == "nearest" else 1e-2
    x, y = orc.make_batch(42, 3, 6, 32, 7)
    for k, d in enumerate(meta["draws"]):
        picked = a[f"d{k}_picked"].tolist()
        model.hcs_sampler = lambda m, chunk, cur, picked=picked: (picked, [cur.index(c) for c in picked])
        model.zero_grad(set_to_none=True)
        out, extra = model(x.to(gpu_device), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss = torch.nn.CrossEntropyLoss()(out, y.to(gpu_device)) + extra
        loss.backward()
        lg = a[f"d{k}_logits"]
        assert np.abs(out.detach().cpu().numpy() - lg).max() <= 3e-2 * np.abs(lg).max()
        assert abs(loss.item() - float(a[f"d{k}_loss"])) <= loss_tol, (k, abs(loss.item() - float(a[f"d{k}_loss"])))
        g = model.feature_extractor.patch_embed.channel_embed.weight.grad.cpu().numpy()
        ref = a[f"d{k}_gchan"]
        assert np.linalg.norm(g - ref) <= 5e-2 * np.linalg.norm(ref), (k, np.linalg.norm(g - ref), np.linalg.norm(ref))
        gp = model.feature_extractor.patch_embed.proj.weight.grad.norm().item()
        assert abs(gp - float(a[f"d{k}_gnorm_proj"])) <= 5e-2 * gp
    # the built-in sampler follows the reference's draw order (python RNG part is reproducible)
    model.hcs_sampler = None
    model.feature_extractor.patch_embed.counter.clear()
    model.cfg["hcs_sampling"] = "lowest_cosine"
    random.seed(3)
    model(x.to(gpu_device), "train", None)
    assert sorted(model.feature_extractor.patch_embed.counter.keys()) == sorted(a["d2_picked"].tolist())


def test_hcs_subset_stays_on_the_device(gpu_device):
    """VERDICT r3 item 7 / SURVEY 8f row 2: the reference's HCS branch moves the sampled subset to the host every step
    (dichavit.py:178/184/200).  Here the draw (same python-RNG and torch-RNG calls in the same order) stays on the device: sequence length
    from the host-drawn subset size, every use of the subset a device gather, picks counted on the device and read lazily.  Checked: three
    training steps run with torch's sync debug mode set to "error" (any synchronising call raises); under the same seeds the legacy path
    (hcs_on_device = False: .cpu() per step, counted in model.host_syncs) gives bit-identical logits and the same pick histogram."""
    meta, _ = load_golden("hcs")
    x, y = orc.make_batch(42, 3, 6, 32, 7)
    xg, yg = x.to(gpu_device), y.to(gpu_device)
    ce = torch.nn.CrossEntropyLoss()
    res = {}
    for on_dev in (False, True):
        model, _ = build(meta, gpu_device)
        model.cfg["hcs_sampling"], model.cfg["hcs_sampling_temp"] = "lowest_cosine_prob", 1000.0
        model.hcs_on_device = on_dev
        pe = model.feature_extractor.patch_embed
        random.seed(17)
        torch.manual_seed(23)
        for _ in range(2):  # warm-up: arena, caches, index tensors
            out, extra = model(xg, "train", None)
            (ce(out, yg) + extra).backward()
        pe.counter.clear()
        torch.cuda.synchronize()
        s0 = model.host_syncs
        outs = []
        if on_dev:
            torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(3):
                model.zero_grad(set_to_none=True)
                out, extra = model(xg, "train", None)
                (ce(out, yg) + extra).backward()
                outs.append(out.detach())
        finally:
            torch.cuda.set_sync_debug_mode("default")
        res[on_dev] = ([o.clone() for o in outs], dict(pe.counter), model.host_syncs - s0)
    assert res[False][2] == 3 and res[True][2] == 0
    assert res[False][1] == res[True][1] and sum(res[True][1].values()) >= 3
    for a_, b_ in zip(res[False][0], res[True][0]):
        assert a_.shape == b_.shape and torch.equal(a_, b_)


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
def test_chammi_chunks_parity(gpu_device, rounding):
    """Three forward/backward passes with 3/4/5 channels (different sequence lengths), gradients
    accumulate across them (trainer.py:846-935); features out; proxy main loss.  The proxy logits multiply the
    feature error by 1/temperature = 14, so the single-pass loss tolerance is 1e-2 with round-to-nearest weight
    copies and 3e-2 (0.7 % of the loss) with the default stochastically rounded ones (twice the rounding variance
    per pass, no bias over passes: see the loss-curve tests)."""
    import diverse_channel_vit_amd as dcv
    meta, a = load_golden("chammi")
    model, _ = build(meta, gpu_device)
    model.stochastic_weight_rounding = rounding == "stochastic"
    shapes = orc.state_shapes(meta["cfg"], 12, meta["img"], meta["num_classes"], chammi=True)
    sd = orc.make_state(shapes, meta["seed"], dtype=torch.float64)
    for v in sd.values():
        v.requires_grad_(True)
    for chunk in ["Allen", "HPA", "CP"]:
        ch = meta["mapper"][chunk]
        x, y = orc.make_batch(meta["seed"] + len(ch), 2, len(ch), meta["img"], meta["num_classes"])
        feat, extra = model(x.to(gpu_device), chunk, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss = dcv.proxy_loss(model.proxies, feat, y.to(gpu_device), model.scale) + 1.0 * extra
        loss.backward()
        ref = a[f"{chunk}_feat"]
        assert np.abs(feat.detach().cpu().numpy() - ref).max() <= 3e-2 * np.abs(ref).max()
        assert abs(extra.item() - float(a[f"{chunk}_extra"])) <= 2e-2 * abs(float(a[f"{chunk}_extra"])) + 1e-6
        assert abs(loss.item() - float(a[f"{chunk}_loss"])) <= (3e-2 if rounding == "stochastic" else 1e-2)
        l2, _, _, _ = orc.chammi_loss(sd, x.double(), y, meta["cfg"], ch, list(range(len(ch))))
        l2.backward()
    check_grads(model, sd)


def test_eval_new_channels_parity(gpu_device):
    meta, a = load_golden("eval_newch")
    model, _ = build(meta, gpu_device, train=False)
    x, _ = orc.make_batch(62, 3, 5, 32, 9)
    with torch.inference_mode():
        for init in ["zero", "avg_2", "avg_3", "replicate", "avg_2_not_in_chunk", "avg_3_not_in_chunk", "random"]:
            out = model(x.to(gpu_device), "test", "train", init_first_layer=None, new_channel_init=init)
            assert isinstance(out, torch.Tensor)
            ref = a["test_" + init]
            assert np.abs(out.cpu().numpy() - ref).max() <= 3e-2 * np.abs(ref).max(), init
        out = model(x.to(gpu_device), "valid", None, init_first_layer=None, new_channel_init=None)
        assert np.abs(out.cpu().numpy() - a["valid_none"]).max() <= 3e-2 * np.abs(a["valid_none"]).max()
    with pytest.raises(ValueError):
        model(x.to(gpu_device), "test", "train", new_channel_init="bogus")


def test_plugin_contract(gpu_device):
    """The trainer's call pattern (trainer.py:1164-1166, 312-320, 986-1006, 1299-1319) on the HIP path."""
    import diverse_channel_vit_amd as dcv
    from diverse_channel_vit_amd import models
    meta, _ = load_golden("so2sat_s")
    cfg = Cfg(meta["cfg"], in_channel_names=[f"c{i}" for i in range(18)], img_size=[32], num_classes=17)
    model = getattr(models, "dichavit")(cfg, mapper={"train": list(range(18))})
    assert isinstance(model, dcv.DiChaViT)
    keys = meta["state_keys"]
    assert sorted(model.state_dict().keys()) == sorted(keys)
    model = model.to(gpu_device)
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = dcv.HipAdamW(params, lr=4.9e-5, weight_decay=0.04, model=model)
    x, y = orc.make_batch(5, 4, 18, 32, 17)
    x, y = x.to(gpu_device), y.to(gpu_device)
    losses = []
    for it in range(3):
        opt.zero_grad()
        output = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=it)
        assert isinstance(output, tuple)
        out, extra_loss = output
        assert extra_loss.shape == torch.Size([])
        loss = torch.nn.CrossEntropyLoss()(out, y) + extra_loss * 1.0
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
        opt.step()
        losses.append(loss.item())
    assert losses[2] < losses[0]
    assert model.proxies.grad is None
    # checkpoint round trip with and without the DDP "module." prefix
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model2 = dcv.dichavit(cfg, mapper={"train": list(range(18))}).to(gpu_device)
    model2.load_state_dict({k[len("module."):]: v for k, v in {"module." + k: v for k, v in sd.items()}.items()})
    model.eval(); model2.eval()
    with torch.inference_mode():
        o1 = model(x, "train", None, new_channel_init=None)
        o2 = model2(x, "train", None, new_channel_init=None)
    assert torch.equal(o1, o2)
    assert model.scale == pytest.approx(math.sqrt(1 / meta["cfg"]["temperature"]))
    assert model.feature_extractor.patch_embed.mapper["train"] == list(range(18))
    with pytest.raises(RuntimeError):
        model(x.cpu(), "train", None)


_CURVE_BATCHES = {}


def _run_curve(gpu_device, name, stochastic, seed=None, prescaled=None):
    import diverse_channel_vit_amd as dcv
    meta, a = load_golden(name)
    model, _ = build(meta, gpu_device)
    model.stochastic_weight_rounding = stochastic
    if prescaled is not None:  # the pre-scaled-q attention entries (default) or the plain ones
        model.attn_prescaled = prescaled
    if seed is not None:  # the draw of the stochastic weight rounding (cfg.weight_rounding_seed; 1 by default)
        model._sr_seed = torch.full((1,), int(seed), dtype=torch.int32, device=gpu_device)
    opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=meta["lr"], weight_decay=meta["wd"],
                       betas=tuple(meta["betas"]), eps=meta["eps"], model=model)
    # the curve's batches are generated (numpy legacy RandomState, on the host: seconds per curve at bs 32) once per curve and kept on the device for the
    # other rounding seeds / builds of the same test; _CURVE_BATCHES.clear() at the end of a test hands the memory back
    if name not in _CURVE_BATCHES:
        _CURVE_BATCHES.clear()
        _CURVE_BATCHES[name] = [tuple(t.to(gpu_device) for t in orc.make_batch(meta["seed"] + 100 + i, meta["B"], meta["n_channels"], meta["img"], meta["num_classes"]))
                                for i in range(meta["n_batches"])]
    batches = _CURVE_BATCHES[name]
    ref = a["losses"][:, 0]
    errs = []
    for s in range(meta["steps"]):
        x, y = batches[s % meta["n_batches"]]
        opt.zero_grad()
        out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss = torch.nn.CrossEntropyLoss()(out, y) + extra
        loss.backward()
        opt.step()
        errs.append(abs(loss.item() - ref[s]))
    return np.array(errs), ref


def _curve_report(tag, e, ref):
    print(f"{tag} |err|: step0 {e[0]:.2e} max {e.max():.3e} mean {e.mean():.3e} tail20 max {e[-20:].max():.3e} steps above 1e-3: {int((e > 1e-3).sum())} "
          f"(ref loss {ref[0]:.3f} -> {ref[-1]:.3f})")


def test_loss_curve_100_steps(gpu_device):
    """100 optimiser steps on the HIP path (bf16 MFMA operands, fp32 master weights, fused HipAdamW) against the reference's fp32 CPU curve
    of the So2Sat-shaped model at bs 8 over 4 REPEATING batches (tests/golden/curve100_so2sat_s.npz; the loss falls 2.78 -> 0.026: the run
    memorises its batches).  SMOKE BOUND ONLY since round 4.

    Finding (round 4; reproduce with DCV_FUSE_LN_MIN_TILES=0 — at this model's 2 312 token rows the fusion is off by default).  Rounds 2-3 treated this curve as well conditioned and asserted it at 1.2 x one build's value (step 0 1.06e-3, max
    4.575e-3, mean 4.759e-4, last 20 steps 1.108e-4).  Moving the forward LayerNorm into the residual GEMM's epilogue — the same arithmetic:
    mean / rstd equal to 1e-6, 0.2 % of the bf16 outputs different by one ulp (test_gemm_nt_resid_ln) — moved it to step 0 6.06e-4, max 1.056e-2,
    mean 7.582e-4, last 20 6.097e-5: better at both ends, 2.3x worse at its worst early step.  A curve that a one-ulp perturbation moves by that
    much measures the conditioning of a memorising trajectory, like the batch-2 curve below; the eleven fp32-atomic runs of round 2 had already
    spread over max 5.0e-3 .. 1.07e-2, mean 4.1e-4 .. 7.2e-4.  The arithmetic claim (north_star: within 1e-3) is carried by the two
    DISTINCT-batch curves (test_loss_curve_distinct_batches_*), whose mean did not move in the fourth digit under the same change.  This test
    keeps the envelope of all equally correct builds seen so far x 1.5 (the round-2 bound) and the contrast with round-to-nearest weight copies
    (Adam's +-lr steps below the bf16 ulp: the copies lag the master coherently, 10x further off)."""
    e_sr, ref = _run_curve(gpu_device, "curve100_so2sat_s", True)
    e_rn, _ = _run_curve(gpu_device, "curve100_so2sat_s", False)
    _curve_report("loss-curve so2sat-s stochastic", e_sr, ref)
    _curve_report("loss-curve so2sat-s nearest   ", e_rn, ref)
    assert e_sr[0] <= 1.5e-3 and e_sr.max() <= 1.6e-2 and e_sr.mean() <= 1.1e-3 and e_sr[-20:].max() <= 2e-4
    assert e_rn[0] <= 1.0e-3 and e_rn.max() <= 7.6e-2 and e_rn.mean() <= 7.4e-3 and e_rn[-20:].max() <= 4.4e-4
    assert e_sr.mean() < 0.5 * e_rn.mean()


def test_loss_curve_distinct_batches_so2sat(gpu_device):
    """The So2Sat-shaped model (18 ch, 32^2, P 8, 17 classes) at bs 8 over 100 DISTINCT batches (tests/golden/curve100_so2sat_s_distinct.npz, the
    real reference's trainer step): nothing is memorised, the loss stays near ln 17, and the comparison measures the arithmetic of the path.
    Bounds FROZEN at round 4's values (deterministic mode: bit-reproducible on a build)."""
    e_sr, ref = _run_curve(gpu_device, "curve100_so2sat_s_distinct", True)
    _curve_report("loss-curve so2sat-s bs8 distinct, stochastic", e_sr, ref)
    # measured in round 4: step 0 2.23e-3 (the very first forward: no update yet), max 2.541e-3, mean 3.412e-4, last 20 <= 3.581e-4, 7 steps above
    # 1e-3; the same build with the LayerNorm as a separate launch (DCV_FUSE_LN=0): 1.65e-3 / 1.705e-3 / 2.953e-4 / 3.736e-4 / 4
    assert e_sr.mean() <= 1e-3, e_sr.mean()             # north_star's criterion on the mean ...
    assert e_sr[-20:].max() <= 1e-3, e_sr[-20:].max()   # ... and on every one of the last 20 steps
    assert e_sr.max() <= 3.3e-3, e_sr.max()             # the worst single step: 1.2 x the worst of ten draws (five rounding seeds x {plain, pre-scaled q}:
    assert int((e_sr > 1e-3).sum()) <= 12               # max 1.02e-3 .. 2.73e-3, mean 2.2e-4 .. 3.3e-4, last 20 <= 4.5e-4, 1 .. 10 steps above 1e-3; profiles/r04_x6_*)


def test_loss_curve_headline_architecture(gpu_device):
    """The same 100 steps on the headline architecture: DiChaViT-S / 8 ch / 224^2 / 161 classes (bs 2, lr 4.9e-5,
    wd 0.04; tests/golden/curve100_jumpcp_s.npz).  At batch 2 the run memorises its 4 batches (loss 5.59 -> 0.088, single
    steps move by up to 0.3), so the trajectory is sensitive: two builds whose kernels differ in the last bf16 bit measured
    stochastic max 2.8e-2 / mean 1.8e-3 / tail 9e-4 and max 6.6e-2 / mean 4.1e-3 / tail 2.2e-3; round-to-nearest copies
    max 1.2e-1..1.5e-1 / mean 1.0e-2..1.4e-2 / tail 5e-3..7e-3 on the same builds.
    With fp32 atomics (round 2) eleven runs of one build spread over max 1.6e-2 .. 6.0e-2, mean 1.5e-3 .. 3.8e-3, tail 7.7e-4 .. 2.6e-3.
    In deterministic mode (round 3, the default) a build is bit-reproducible run to run — but this batch-2 run is chaotic, not just noisy:
    two deterministic builds that differ ONLY in the association order of LayerNorm's dgamma / dbeta partial sums (16 interleaved lanes
    instead of one sequential walk over the 1024 partials) printed step0 1.01e-3 / max 1.460e-2 / mean 1.534e-3 / tail 8.703e-4 and
    step0 1.01e-3 / max 3.328e-2 / mean 2.730e-3 / tail 1.759e-3 — both inside the envelope the atomic runs had drawn.  A bound at
    1.2 x one such value would test the summation order, not the arithmetic; the well-conditioned So2Sat curve above carries the tight
    bound, this one keeps the envelope of all equally correct orders seen so far x 1.5: step0 <= 2.1e-3 (it does not depend on the
    order: no update has happened yet), max <= 0.1, mean <= 6.2e-3, tail <= 3.9e-3; round-to-nearest (contrast only): max <= 0.23, mean <= 2.1e-2."""
    e_sr, ref = _run_curve(gpu_device, "curve100_jumpcp_s", True)
    e_rn, _ = _run_curve(gpu_device, "curve100_jumpcp_s", False)
    _curve_report("loss-curve headline stochastic", e_sr, ref)
    _curve_report("loss-curve headline nearest   ", e_rn, ref)
    assert e_sr[0] <= 2.1e-3 and e_sr.max() <= 0.1 and e_sr.mean() <= 6.2e-3 and e_sr[-20:].max() <= 3.9e-3
    assert e_rn.max() <= 0.23 and e_rn.mean() <= 2.1e-2


def test_loss_curve_distinct_batches_headline_architecture(gpu_device):
    """The headline architecture (DiChaViT-S, 8 ch, 224^2, 161 classes) at batch 8 over 100 DISTINCT batches (tests/golden/curve100_jumpcp_s_b8.npz,
    generated by the real reference: trainer.py:963-1028's step, lr 4.9e-5, wd 0.04).  No batch is seen twice: the loss stays near ln 161 and
    the comparison measures the arithmetic of the path rather than the conditioning of a memorising trajectory.

    What is asserted HERE is weaker than north_star's criterion, and says so: at batch 8 the per-step error moves with the DRAW of the
    stochastic weight rounding as much as with the build — five rounding seeds x {plain, pre-scaled q} (profiles/r04_x6_*): mean 3.4e-4 .. 4.5e-4,
    maximum of the last 20 steps 5.8e-4 .. 1.06e-3 (three of ten draws above 1e-3), worst step 1.44e-3 .. 1.92e-3, 3 .. 11 steps above 1e-3.  So:
    the MEAN meets 1e-3 with a factor two to spare on every draw; "every one of the last 20 steps within 1e-3" does NOT hold on every draw at
    this batch size and is bounded at 1.3e-3.  north_star states the criterion at bs 64; the per-step error is a batch mean and the draw-to-draw
    spread falls with the batch size (profiles/r05_x1_*): test_loss_curve_north_star_criterion asserts the criterion itself, unweakened, at bs 16
    and bs 32 on three rounding seeds each.  These bs-8 bounds were set from the ten-draw spread in round 4 and may only be tightened."""
    e_sr, ref = _run_curve(gpu_device, "curve100_jumpcp_s_b8", True)
    _curve_report("loss-curve headline bs8 distinct, stochastic", e_sr, ref)
    assert e_sr.mean() <= 6e-4, e_sr.mean()               # north_star's 1e-3 on the mean (worst of ten draws 4.5e-4)
    assert e_sr[-20:].max() <= 1.3e-3, e_sr[-20:].max()   # NOT north_star's 1e-3: 1.2 x the worst of ten draws
    assert e_sr[-20:].mean() <= 6e-4, e_sr[-20:].mean()
    assert e_sr.max() <= 2.8e-3, e_sr.max()               # worst of ten draws 1.92e-3
    assert int((e_sr > 1e-3).sum()) <= 14                 # 3 .. 11 over ten draws


@pytest.mark.parametrize("name", ["curve100_jumpcp_s_b16", "curve100_jumpcp_s_b32"])
def test_loss_curve_north_star_criterion(gpu_device, name):
    """north_star: "100-step loss curve within 1e-3 of reference" (quoted at bs 64 per GPU).  VERDICT r4 item 5: test the criterion where it is
    stated instead of re-fitting bounds at bs 8.  Headline architecture, 100 DISTINCT batches from the real reference (trainer.py:963-1028's step,
    train_scripts.sh:5's first-epoch lr) at bs 16 and bs 32 — the largest the reference's CPU path produces here in bounded time (50 min / 2.4 h of
    reference CPU time, 24 / 45 GB of host memory; bs 64 would need > 64 GB).  Three draws of the stochastic weight rounding each; on EVERY draw:
    mean |err| <= 1e-3 and every one of the last 20 steps <= 1e-3.  These two bounds are the criterion, not fitted numbers; the maximum over all
    100 steps is printed and bounded only loosely (early steps carry the un-averaged first-forward difference).  An exceedance is a finding for
    DESIGN section 4, not a new constant."""
    if not os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")):
        pytest.skip(name + ".npz not generated (tests/golden/make_golden.py " + name.replace("curve100_jumpcp_s", "curve_jumpcp") + ")")
    worst = 0.0
    for seed in (1, 2, 3):
        e, ref = _run_curve(gpu_device, name, True, seed=seed)
        _curve_report(f"loss-curve {name} rounding seed {seed}", e, ref)
        assert e.mean() <= 1e-3, (seed, e.mean())
        assert e[-20:].max() <= 1e-3, (seed, e[-20:].max())
        worst = max(worst, e.max())
    print(f"{name}: largest single-step |err| over three draws {worst:.3e}")
    _CURVE_BATCHES.clear()
    assert worst <= 3e-3, worst


def test_loss_curve_prescaled_q_gap(gpu_device):
    """the round that moved the attention arithmetic (pre-scaled q, round 4) also widened curve bounds; this pins what that path may
    cost, at a FIXED rounding seed: the bs-16 headline curve with the pre-scaled-q attention (default) and with the plain entries
    (model.attn_prescaled = False) both meet the criterion, and their mean errors differ by less than the draw-to-draw spread (3e-4)."""
    name = "curve100_jumpcp_s_b16"
    stats = {}
    for ps in (True, False):
        e, ref = _run_curve(gpu_device, name, True, seed=1, prescaled=ps)
        _curve_report(f"loss-curve bs16 pre-scaled q = {ps}", e, ref)
        assert e.mean() <= 1e-3 and e[-20:].max() <= 1e-3, (ps, e.mean(), e[-20:].max())
        stats[ps] = e.mean()
    _CURVE_BATCHES.clear()
    assert abs(stats[True] - stats[False]) <= 3e-4, stats


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
def test_graphed_step_matches_eager(gpu_device, rounding):
    """The HIP-graph replay of the captured step (graph.GraphedTrainStep + capturable HipAdamW) follows the same
    trajectory as eager launches: same losses and parameters up to fp32-atomic ordering noise, and the
    optimiser scalars (step count -> bias corrections, lr) really advance between replays."""
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("so2sat_s")
    x, y = orc.make_batch(77, 4, 18, 32, 17)
    x, y = x.to(gpu_device), y.to(gpu_device)
    ce = torch.nn.CrossEntropyLoss()
    runs = {}
    for mode in ("eager", "graph"):
        model, _ = build(meta, gpu_device)
        model.stochastic_weight_rounding = rounding == "stochastic"
        opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=0.04, model=model,
                           capturable=(mode == "graph"))
        losses = []
        if mode == "eager":
            for s in range(6):
                if s == 4:
                    opt.param_groups[0]["lr"] = 5e-5  # a scheduler edit must be honoured in both modes
                opt.zero_grad()
                out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
                loss = ce(out, y) + extra
                loss.backward()
                opt.step()
                losses.append(loss.item())
        else:
            gs = dcv.GraphedTrainStep(model, opt, "train", None, ce, 1.0, warmup=2)
            # the first call runs 2 eager warm-up steps (= steps 0,1) and then replays (= step 2)
            for s in range(2, 6):
                if s == 4:
                    opt.param_groups[0]["lr"] = 5e-5
                losses.append(gs(x, y).item())
        runs[mode] = (losses, model.feature_extractor.blocks[3].mlp.fc1.weight.detach().clone(), opt._step,
                      None if model._sr_seed is None else int(model._sr_seed.item()))
    le, lg = runs["eager"][0], runs["graph"][0]
    assert runs["eager"][2] == runs["graph"][2] == 6
    for a, b in zip(le[2:], lg):
        assert abs(a - b) <= 2e-3, (le, lg)
    we, wg = runs["eager"][1], runs["graph"][1]
    # nearest: only the order of the fp32 atomic adds of the weight-gradient GEMMs separates the two runs.  Adam's early steps are
    # sign-like (|m / sqrt(v)| ~ 1): an element whose true gradient is ~0 can come out with either sign, and each step in which the
    # two runs disagree moves them apart by up to 2 lr — at most sum_s 2 lr_s = 2 (4 x 1e-4 + 2 x 5e-5) = 1e-3 on single elements
    # (measured maxima: 1.2e-4 .. 2.3e-4, i.e. one or two such steps), while the MEAN over the 590 k elements stays at the noise
    # level.  What the test guards — a replay that read a wrong step count / lr — would move EVERY element by ~lr (mean >= 5e-5).
    # stochastic: both draw the same bits (the seed word is bumped on the device, also by replays: 1 + 6 forwards), but ordering
    # noise can flip single roundings too.
    d = (we - wg).abs()
    print(f"graph vs eager ({rounding}): max |dW| {d.max().item():.2e}, mean {d.mean().item():.2e}")
    # round 3: the tests run in deterministic mode, where the replayed graph and the eager launches execute the same sums in the same
    # order — the weights after six steps are BIT-identical (the bounds above are what the fp32-atomic mode needs)
    import diverse_channel_vit_amd as dcv_
    if dcv_.is_deterministic():
        assert torch.equal(we, wg) and le[2:] == lg
    else:
        assert d.max().item() <= 1e-3 and d.mean().item() <= (5e-6 if rounding == "nearest" else 2e-5), (d.max().item(), d.mean().item())
    assert runs["eager"][3] == runs["graph"][3] == (None if rounding == "nearest" else 7)
    assert lg[-1] < lg[0]


def test_dp_reducer_on_rccl_single_gpu(gpu_device):
    """The data-parallel path of bench.py (dp.DataParallel: per-layer arena buckets all-reduced from inside the
    backward, hooks for the parameters outside the encoder, HipAdamW.finalize) on the real RCCL backend.  Only one
    GPU is available to tests, so the group has world_size 1 and the collectives are forced: this checks the
    plumbing (async all-reduce of arena slices issued from the autograd thread, AVG op, stream waits) — gradients
    must be identical to the single-process run.  Multi-rank arithmetic is covered by tests/test_dp_gloo.py."""
    import os
    import torch.distributed as dist
    import diverse_channel_vit_amd as dcv
    if dist.is_initialized():
        pytest.skip("a process group already exists")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29613")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu_device)
    try:
        meta, _ = load_golden("so2sat_s")
        x, y = orc.make_batch(5, 4, 18, 32, 17)
        x, y = x.to(gpu_device), y.to(gpu_device)
        grads = {}
        # also the bf16 exchange and the no-overlap (one collective after the backward) flags on the RCCL backend
        for mode in ("plain", "dp", "dp_bf16", "dp_no_overlap"):
            model, _ = build(meta, gpu_device)
            if mode != "plain":
                model._ensure_arena(gpu_device)
                dp = dcv.DataParallel(model, min_bucket_bytes=1 << 20, force_collectives=True,
                                      grad_dtype=torch.bfloat16 if mode == "dp_bf16" else torch.float32, overlap=mode != "dp_no_overlap")
                dp.broadcast_parameters(0)
                dp.hook_misc_params()
            opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4, model=model)
            opt.zero_grad()
            out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
            (torch.nn.functional.cross_entropy(out, y) + extra).backward()
            if mode != "plain":
                # 12 blocks (7 MB each) merged/kept + tokeniser + final norm + misc params; no overlap: ONE collective of everything
                assert dp.buckets_launched >= (8 if mode != "dp_no_overlap" else 1)
                dp.finalize()
            grads[mode] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
            opt.step()
        for mode in ("dp", "dp_bf16", "dp_no_overlap"):
            for k, g in grads["plain"].items():
                ref = g.abs().max().item()
                # bf16 exchange: every element rounded to bf16 once (2^-9 relative)
                assert (grads[mode][k] - g).abs().max().item() <= (4e-3 if mode == "dp_bf16" else 1e-3) * ref + 1e-9, (mode, k)
        # and against the checker: every gradient that went through RCCL vs the fp64 oracle on the same batch
        ch = meta["mapper"][meta["chunk"]]
        sd_ref, *_ = oracle_grads(meta, x.cpu(), y.cpu(), ch, list(range(len(ch))))
        check_grads(model, sd_ref)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_bench_two_ranks_as_the_driver_launches_it(gpu_device):
    """`python -m torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2` — the driver's N > 1 command line — end to end on this box's one GPU
    (DCV_BENCH_REHEARSAL=gloo: both ranks on cuda:0, gloo instead of RCCL, which refuses two ranks on one device).  Every rank must leave with exit code 0
    and rank 0 must print exactly ONE JSON line with both exchange modes timed.  Regression: round 5's `status` field was written on the ranks that have no
    line (rank != 0 raised TypeError after the timed region and the launcher tore the job down) — no single-process test executes those branches."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, DCV_BENCH_REHEARSAL="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "16"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["status"] == "ok" and line["n_gpus"] == 2 and line["steps"] == 2 and line["scaling"] == "weak"
    assert line["dp"]["world_size"] == 2 and set(line["dp"]["modes"]) == {"single_allreduce_after_backward", "overlap"}
    assert line["value"] > 0 and abs(line["value"] - 16 * 2 / (line["ms_per_step"] / 1e3)) <= 0.02 * line["value"]  # whole-job images per second
    print(f"two ranks on one GPU over gloo: {line['value']:.0f} img/s, modes {line['dp']['modes']}")


@pytest.mark.timeout(600)
def test_bench_plain_and_full_runs_dump_the_same_outputs(gpu_device, tmp_path):
    """`bench.py --dump-outputs DIR`: a plain run (the headline line only) and a --full run (profiled warm-up steps, events around the dominant
    kernel in the timed region) of the same arguments write float32 / float64 arrays of at most 64 MB, and the same ones bit for bit (deterministic
    reductions, fixed inputs and seeds); only the --full line carries the roofline and the kernel table."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "4"]
    runs = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        out = tmp_path / mode
        r = subprocess.run(base + extra + ["--dump-outputs", str(out)], cwd=root, capture_output=True, text=True, timeout=500)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["status"] == "ok" and line["steps"] == 3 and line["ms_per_step"] > 0
        assert abs(line["value"] - 4 / (line["ms_per_step"] / 1e3)) <= 0.02 * line["value"]
        assert ("roofline" in line and "kernel_table" in line) == (mode == "full")
        assert "cpu_baseline" not in line
        arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
        assert set(arrays) == {"loss", "logits", "params", "grads"}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert arrays["logits"].shape == (4, 161) and arrays["params"].shape == arrays["grads"].shape
        assert np.isfinite(arrays["loss"]) and abs(float(arrays["loss"]) - line["config"]["final_loss"]) <= 1e-5
        runs[mode] = arrays
    for k in runs["plain"]:
        assert np.array_equal(runs["plain"][k], runs["full"][k]), k


def test_base_width_train_step(gpu_device):
    """DiChaViT-Base dimensions (D = 768, 12 heads, MLP 3072; BASELINE config 5's architecture) on a small image:
    one training step against the oracle — exercises every kernel at the wider layout (LN/ortho lanes, GEMM N tiles
    that are not multiples of the tile, 12-head attention)."""
    cfg = dict(name="dichavit", pretrained_model_name="base", patch_size=16, temperature=0.07, learnable_temp=False,
               enable_sample=False, use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none",
               freeze_channel_emb=False, block_type="block", hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.001,
               ortho_loss_v1_lambda=0.001, drop_path_rate=0.0, gamma_s=1.0, gamma_d=4.0, reverse_pos_pairs=True, use_square=False)
    meta = dict(cfg=cfg, mapper={"train": list(range(5))}, n_channels=5, img=64, num_classes=11, seed=91, B=2)
    model, _ = build(meta, gpu_device)
    x, y = orc.make_batch(92, 2, 5, 64, 11)
    out, extra = model(x.to(gpu_device), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    loss = torch.nn.functional.cross_entropy(out, y.to(gpu_device)) + extra
    loss.backward()
    sd_ref, loss_ref, extra_ref, out_ref = oracle_grads(meta, x, y, list(range(5)), list(range(5)))
    assert (out.detach().cpu().double() - out_ref).abs().max().item() <= 3e-2 * out_ref.abs().max().item()
    # Expected error, not a round number: every GEMM output carries the bf16 rounding of its K products, relative error
    # ~ 2^-9 / sqrt(3) per operand, accumulated as a random walk: sigma(K) ~ sqrt(K).  DiChaViT-S (K = 384 / 1536) measures
    # |dloss| <= 2e-3 on its goldens against the 5e-3 bound; Base doubles every K (768 / 3072) -> sqrt(2) per GEMM, and its
    # 12 blocks at twice the residual width add the same factor once more on the logits: 5e-3 * 2 = 1e-2 expected bound
    # (measured 8.7e-3 on MI355X with stochastically rounded weight copies, which add their own ulp/sqrt(12) per weight).
    assert abs(loss.item() - loss_ref) <= 1.2e-2
    worst = check_grads(model, sd_ref)
    print(f"base width: loss {loss.item():.6f} (oracle {loss_ref:.6f}) worst grad rel err {worst}")


def test_resolution_change_parity(gpu_device):
    """Images of another resolution than the model's img_size (48 and 24 px on a 32-px model): the positional grid
    is resampled 4x4 -> 6x6 / 3x3 and its gradient is the exact bicubic adjoint (golden from the reference)."""
    meta, a = load_golden("resolution")
    for img_in in (48, 24):
        model, _ = build(meta, gpu_device)
        x, y = orc.make_batch(96 + img_in, 2, 4, img_in, 6)
        out, extra = model(x.to(gpu_device), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss = torch.nn.functional.cross_entropy(out, y.to(gpu_device)) + extra
        loss.backward()
        ref = a[f"logits_{img_in}"]
        assert np.abs(out.detach().cpu().numpy() - ref).max() <= 3e-2 * np.abs(ref).max()
        assert abs(loss.item() - float(a[f"loss_{img_in}"])) <= 5e-3
        g = model.feature_extractor.pos_embed.grad.cpu().numpy()
        gr = a[f"gpos_{img_in}"]
        assert np.linalg.norm(g - gr) <= 5e-2 * np.linalg.norm(gr), (img_in, np.linalg.norm(g - gr), np.linalg.norm(gr))
        model.eval()
        with torch.inference_mode():
            ev = model(x.to(gpu_device), "train", None, new_channel_init=None)
        assert np.abs(ev.cpu().numpy() - a[f"eval_{img_in}"]).max() <= 3e-2 * np.abs(a[f"eval_{img_in}"]).max()


def test_token_drop_parity(gpu_device):
    """dropout_tokens_hcs (dichavit.py:568-627): the HIP path draws the same token subset as the reference from the
    seeded python RNG, runs the encoder on the kept rows only, and scatters the gradient back."""
    meta, a = load_golden("tokendrop")
    x, y = orc.make_batch(98, 2, 5, 32, 6)
    for k, d in enumerate(meta["draws"]):
        m2 = dict(meta, cfg=dict(meta["cfg"], dropout_tokens_hcs=d["mode"]))
        model, _ = build(m2, gpu_device)
        random.seed(d["pyseed"])
        out, extra = model(x.to(gpu_device), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss = torch.nn.functional.cross_entropy(out, y.to(gpu_device)) + extra
        loss.backward()
        ref = a[f"d{k}_logits"]
        assert np.abs(out.detach().cpu().numpy() - ref).max() <= 3e-2 * np.abs(ref).max(), d
        assert abs(loss.item() - float(a[f"d{k}_loss"])) <= 5e-3
        g = model.feature_extractor.pos_embed.grad.cpu().numpy()
        gr = a[f"d{k}_gpos"]
        assert np.linalg.norm(g - gr) <= 5e-2 * np.linalg.norm(gr), d
        gp = model.feature_extractor.patch_embed.proj.weight.grad.norm().item()
        assert abs(gp - float(a[f"d{k}_gnorm_proj"])) <= 5e-2 * gp
        # eval ignores the option
        model.eval()
        with torch.inference_mode():
            assert model(x.to(gpu_device), "train", None).shape == (2, 6)


def test_fused_input_normalisation(gpu_device):
    """raw uint8 pixels + set_input_normalisation(mean, std) give the same forward/backward as the
    reference's batch format (float32 already normalised on the CPU as (x/255 - mean_c)/std_c), incl. a chunk whose
    channels are a non-identity subset of the global ids."""
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("chammi")
    rs = np.random.RandomState(5)
    mean = rs.uniform(0.02, 0.3, 12).astype(np.float32)
    std = rs.uniform(0.05, 0.2, 12).astype(np.float32)
    ch = meta["mapper"]["HPA"]  # global ids [3,4,5,6]
    raw = torch.from_numpy(rs.randint(0, 256, (2, 4, 64, 64)).astype(np.uint8))
    ref_in = (raw.float() / 255.0 - torch.from_numpy(mean[ch])[None, :, None, None]) / torch.from_numpy(std[ch])[None, :, None, None]
    outs = []
    for fused in (False, True):
        model, _ = build(meta, gpu_device)
        if fused:
            model.set_input_normalisation(mean, std, 255.0)
            x = raw.to(gpu_device)
        else:
            x = ref_in.to(gpu_device)
        feat, extra = model(x, "HPA", init_first_layer=None, new_channel_init=None, cur_epoch=0)
        (feat.square().mean() + extra).backward()
        outs.append((feat.detach().clone(), extra.item(), model.feature_extractor.patch_embed.proj.weight.grad.detach().clone()))
    (f0, e0, g0), (f1, e1, g1) = outs
    assert (f0 - f1).abs().max().item() <= 2e-2 * f0.abs().max().item()
    assert abs(e0 - e1) <= 1e-3 * abs(e0) + 1e-6
    assert (g0 - g1).norm().item() <= 2e-2 * g0.norm().item()
    # and against the checker: the fp64 oracle fed the batch the reference would see (normalised on the host)
    shapes = orc.state_shapes(meta["cfg"], 12, meta["img"], meta["num_classes"], chammi=True)
    sd = orc.make_state(shapes, meta["seed"], dtype=torch.float64)
    for v in sd.values():
        v.requires_grad_(True)
    fr, er = orc.forward(sd, ref_in.double(), meta["cfg"], ch, list(range(len(ch))))
    (fr.square().mean() + er).backward()
    assert (f1.double().cpu() - fr.detach()).abs().max().item() <= 3e-2 * fr.detach().abs().max().item()
    assert abs(e1 - er.item()) <= 2e-2 * abs(er.item()) + 1e-6
    gr = sd["feature_extractor.patch_embed.proj.weight"].grad
    assert (g1.double().cpu() - gr).norm().item() <= 5e-2 * gr.norm().item()
    model, _ = build(meta, gpu_device)
    with pytest.raises(ValueError):
        model(raw.to(gpu_device), "HPA")



def test_grad_scaler_flow_of_the_reference_trainer(gpu_device):
    """The reference's `use_amp` flow (trainer.py:861, 921-935; default off): scaler.scale(loss).backward(); scaler.unscale_(opt);
    clip; scaler.step(opt); scaler.update() — driven through the hand-written backward, the gradient arena and HipAdamW (VERDICT r3 missing 5;
    INTEGRATION.md claims it works).  The loss scale is a power of two, so every scaled gradient is the unscaled one times 2^k exactly (bf16
    and fp32 share an exponent range): after unscale_ the step must retrace the plain flow BIT FOR BIT; and a step whose gradients overflow
    must be skipped (parameters untouched, scale halved)."""
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("so2sat_s")
    ce = torch.nn.CrossEntropyLoss()
    batches = [orc.make_batch(501 + i, 4, 18, 32, 17) for i in range(3)]
    batches = [(x.to(gpu_device), y.to(gpu_device)) for x, y in batches]

    def run(use_scaler):
        model, _ = build(meta, gpu_device)
        model.stochastic_weight_rounding = False
        opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.04, model=model)
        scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 12, growth_interval=1000) if use_scaler else None
        losses = []
        for s in range(3):
            x, y = batches[s]
            opt.zero_grad()
            # the reference's flow wraps forward + loss in autocast when use_amp is set (trainer.py:861); the model switches it off inside
            with torch.autocast("cuda", dtype=torch.float16, enabled=use_scaler):
                out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
                assert out.dtype == torch.float32 and extra.dtype == torch.float32
                loss = ce(out, y) + extra
            if scaler is None:
                loss.backward()
                dcv.clip_grad_norm_(model, 5.0)
                opt.step()
            else:
                scaler.scale(loss).backward()
                scaler.unscale_(opt)
                dcv.clip_grad_norm_(model, 5.0)
                scaler.step(opt)
                scaler.update()
            losses.append(loss.item())
        return model, opt, scaler, losses

    m0, _, _, l0 = run(False)
    m1, opt1, scaler, l1 = run(True)
    assert l0 == l1, (l0, l1)
    for (n0, p0), (n1, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        assert n0 == n1 and torch.equal(p0.detach(), p1.detach()), n0
    assert scaler.get_scale() == 2.0 ** 12
    # an overflowing step: the scaler must see the inf in the arena's gradient views and skip the optimiser step
    before = [p.detach().clone() for p in m1.parameters()]
    x, y = batches[0]
    opt1.zero_grad()
    out, extra = m1(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    loss = ce(out, y) + extra
    scaler.scale(loss * float("inf")).backward()
    scaler.unscale_(opt1)
    scaler.step(opt1)
    scaler.update()
    assert scaler.get_scale() == 2.0 ** 11
    for b, p in zip(before, m1.parameters()):
        assert torch.equal(b, p.detach())


def test_clipping_checkpoint_resume_parity(gpu_device, tmp_path):
    """SURVEY §8f rows 1 and 4 in the reference's own flow (tests/golden/resume.npz: the reference module + torch AdamW,
    clip_grad_norm_(0.5), lr 1e-3, 6 steps): the HIP path reproduces the pre-clip total norms and the losses; a checkpoint
    written after step 3 in the trainer's layout (trainer.py:1292-1328), loaded into a FRESH model + optimizer, continues on
    the same trajectory; state_dict()s have the reference's keys, order and optimizer-state indexing."""
    import diverse_channel_vit_amd as dcv
    meta, a = load_golden("resume")
    ce = torch.nn.CrossEntropyLoss()
    batches = [orc.make_batch(151 + i, meta["B"], 3, meta["img"], meta["num_classes"]) for i in range(3)]
    batches = [(x.to(gpu_device), y.to(gpu_device)) for x, y in batches]

    def make(stochastic=False):
        model, _ = build(meta, gpu_device)
        model.stochastic_weight_rounding = stochastic  # deterministic copies: the resumed run must retrace the uninterrupted one
        opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=meta["lr"], weight_decay=meta["wd"], model=model)
        return model, opt

    def one(model, opt, s):
        x, y = batches[s % 3]
        opt.zero_grad()
        out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss = ce(out, y) + extra
        loss.backward()
        tn = dcv.clip_grad_norm_(model, meta["clip"])
        opt.step()
        return loss.item(), tn.item()

    model, opt = make()
    assert [n for n, p in model.named_parameters() if p.requires_grad] == meta["param_order"]
    run = [one(model, opt, s) for s in range(3)]
    # layout of what gets saved
    osd = opt.state_dict()
    L = meta["ck_layout"]
    assert list(model.state_dict().keys()) == L["model_keys"]
    assert sorted(int(i) for i in osd["state"]) == L["opt_state_ids"] and len(osd["state"]) == L["n_opt_state"]
    assert sorted(osd["state"][1].keys()) == L["opt_state_keys"]
    assert [int(i) for i in osd["param_groups"][0]["params"]] == L["opt_param_ids"]
    for idx in (1, 2, 5, 20, 100):
        ref = a[f"ckpt_opt_norm/{idx}"]
        st = osd["state"][idx]
        assert abs(st["exp_avg"].double().norm().item() - ref[0]) <= 3e-2 * ref[0] + 1e-9
        assert abs(st["exp_avg_sq"].double().norm().item() - ref[1]) <= 6e-2 * ref[1] + 1e-12
        assert int(st["step"]) == 3
    path = str(tmp_path / "ckpt.pt")
    dcv.save_checkpoint(path, model, opt, epoch=7, accuracy=12.5, config=meta["cfg"])
    cont = [one(model, opt, s) for s in range(3, 6)]           # uninterrupted
    model2, opt2 = make()
    # a checkpoint written from a DataParallel/DDP-wrapped model carries "module." prefixes (trainer.py:1313-1318)
    st = torch.load(path, weights_only=True)
    assert set(st.keys()) == {"epoch", "accuracy", "config", "optimizer_params", "model_params", "scheduler_params", "scaler_params", "datetime"}
    st["model_params"] = {"module." + k: v for k, v in st["model_params"].items()}
    torch.save(st, path)
    assert dcv.load_checkpoint(path, model2, opt2, map_location=gpu_device) == 7
    resumed = [one(model2, opt2, s) for s in range(3, 6)]
    model3, opt3 = make(stochastic=True)  # the default training mode, uninterrupted, against the reference's numbers
    full = [one(model3, opt3, s) for s in range(6)]
    losses = np.array([r[0] for r in full])
    norms = np.array([r[1] for r in full])
    print("resume: loss err", np.abs(losses - a["losses"]).max(), "norm rel err", (np.abs(norms - a["total_norms"]) / a["total_norms"]).max(),
          "resumed-vs-uninterrupted", max(abs(r[0] - c[0]) for r, c in zip(resumed, cont)))
    assert np.abs(losses - a["losses"]).max() <= 1.5e-2     # measured 1.4e-3 .. 6.3e-3 across builds (round-to-nearest copies: 3.0e-2); lr is 20x the curve tests'
    assert (np.abs(norms - a["total_norms"]) / a["total_norms"]).max() <= 1e-2
    for r, c in zip(resumed, cont):
        assert abs(r[0] - c[0]) <= 2e-3 and abs(r[1] - c[1]) <= 2e-3 * c[1]
    for n_, p_ in model3.named_parameters():
        if not n_.startswith("adaptive_interface"):
            ref = float(a["final_norm/" + n_])
            # six sign-like Adam steps of lr 1e-3: a gradient element whose sign flips under bf16 noise moves by 2 lr
            assert abs(p_.detach().double().norm().item() - ref) <= 1e-2 * ref + 1e-6, n_


def test_clip_grad_norm_matches_torch(gpu_device):
    """dcv.clip_grad_norm_ against torch.nn.utils.clip_grad_norm_ on the same gradients (fp32 reference of the same op),
    both when clipping bites and when it does not."""
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("tiny_e2e")
    model, _ = build(meta, gpu_device)
    x, y = orc.make_batch(3, 2, 3, 32, 5)
    for max_norm in (0.05, 1e4):
        model.zero_grad()
        out, extra = model(x.to(gpu_device), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        (torch.nn.CrossEntropyLoss()(out, y.to(gpu_device)) + extra).backward()
        ref = [p.grad.detach().clone() for p in model.parameters() if p.grad is not None]
        tot = torch.sqrt(sum((g.double() ** 2).sum() for g in ref))
        coef = min(1.0, max_norm / (tot.item() + 1e-6))
        got = dcv.clip_grad_norm_(model, max_norm)
        assert abs(got.item() - tot.item()) <= 1e-5 * tot.item()
        for p, g in zip([p for p in model.parameters() if p.grad is not None], ref):
            assert torch.allclose(p.grad, g * coef, rtol=1e-5, atol=1e-9)


def test_evaluate_helper(gpu_device):
    """checkpoint.evaluate = eval_regular's loop (trainer.py:385-449): eval mode, bare-tensor forward, top-1 in percent;
    the model's mode is restored."""
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("tiny_e2e")
    model, _ = build(meta, gpu_device)
    batches = [orc.make_batch(60 + i, 4, 3, 32, 5) for i in range(3)]
    acc = dcv.evaluate(model, [{"image": x, "label": y, "channels": None} for x, y in batches], "train", device=gpu_device)
    model.eval()
    with torch.inference_mode():
        hits = sum((model(x.to(gpu_device), "train").argmax(1).cpu() == y).sum().item() for x, y in batches)
    assert abs(acc - 100.0 * hits / 12) < 1e-9
    model.train()
    dcv.evaluate(model, batches, "train", device=gpu_device)
    assert model.training


def _golden_grad_check(model, a, prefix="", rel_tol=5e-2):
    """Gradients against the REAL reference's fixture: every tensor's norm, and 64 evenly spaced entries of it."""
    n = 0
    params = dict(model.named_parameters())
    for k, v in a.items():
        if not k.startswith(prefix + "gnorm/"):
            continue
        name = k[len(prefix) + 6:]
        g = params[name].grad
        assert g is not None, name
        gn = float(v)
        if gn < 1e-7:
            continue
        assert abs(g.norm().item() - gn) <= rel_tol * gn, (name, g.norm().item(), gn)
        samp = a[prefix + "gsamp/" + name]
        idx = np.unique(np.linspace(0, g.numel() - 1, min(64, g.numel())).astype(np.int64))
        mine = g.detach().flatten()[torch.from_numpy(idx).to(g.device)].double().cpu().numpy()
        assert np.linalg.norm(mine - samp) <= 8e-2 * np.linalg.norm(samp) + 1e-3 * gn / math.sqrt(g.numel()) * math.sqrt(len(idx)), name
        n += 1
    assert n > 100
    return n


def test_headline_batch16_multi_round_gemm_parity(gpu_device):
    """The headline architecture at batch 16 against the real reference (tests/golden/jumpcp_s_b16.npz): M = 25 104 token
    rows -> 297 tiles of 256 x 128 (more than the 256 persistent workgroups: the multi-round walk) and the 256 x 384 kernel
    (M >= 4096) both run INSIDE a model-level golden; logits, loss, and every gradient tensor of the reference."""
    meta, a = load_golden("jumpcp_s_b16")
    model, _ = build(meta, gpu_device)
    model.stochastic_weight_rounding = False
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], 8, 224, 161)
    out, extra = model(x.to(gpu_device), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    loss = torch.nn.CrossEntropyLoss()(out, y.to(gpu_device)) + extra
    loss.backward()
    lg = a["logits"]
    assert np.abs(out.detach().cpu().numpy() - lg).max() <= 3e-2 * np.abs(lg).max()
    assert abs(extra.item() - float(a["extra"])) <= 2e-2 * abs(float(a["extra"])) + 1e-6
    assert abs(loss.item() - float(a["loss"])) <= 5e-3
    _golden_grad_check(model, a)


def test_base_32_channels_6273_tokens_train_step(gpu_device):
    """BASELINE config 5's architecture as a TRAIN step: DiChaViT-Base (D = 768, 12 heads), 32 channels x 196
    patches + CLS = 6 273 tokens, batch 1, against the real reference (tests/golden/base32_train.npz — the largest channel count whose
    saved fp32 attention matrices fit the build container): logits, losses and every parameter gradient's norm and samples.  The
    whole-model backward at a long sequence: attention dQ / dK / dV over 49 key tiles x 49 query tiles per head, GEMMs with K = 768 / 3072."""
    meta, a = load_golden("base32_train")
    model, _ = build(meta, gpu_device)
    model.stochastic_weight_rounding = False
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], 32, 224, 161)
    out, extra = model(x.to(gpu_device), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    loss = torch.nn.CrossEntropyLoss()(out, y.to(gpu_device)) + extra
    loss.backward()
    lg = a["logits"]
    err = np.abs(out.detach().cpu().numpy() - lg).max()
    print(f"base/32ch/N=6273 train step: max |dlogit| {err:.3e} (max |logit| {np.abs(lg).max():.3f}) loss {loss.item():.6f} (reference {float(a['loss']):.6f})")
    assert err <= 3e-2 * np.abs(lg).max()
    assert abs(extra.item() - float(a["extra"])) <= 2e-2 * abs(float(a["extra"])) + 1e-6
    assert abs(loss.item() - float(a["loss"])) <= 1.2e-2  # Base width: sqrt(2) per GEMM and per residual width over DiChaViT-S's 5e-3 (test_base_width_train_step)
    _golden_grad_check(model, a)


def test_deterministic_mode_train_step_is_bit_reproducible(gpu_device):
    """with diverse_channel_vit_amd.set_deterministic(True) (the tests' default; the reference sets
    cudnn.deterministic = True, utils.py:394-401) two runs of the headline architecture's train step at batch 16 — weight gradients split
    over ~250 workgroups per product, second stream on — give bit-identical logits, loss and gradients for every parameter, with
    stochastically rounded weight copies (same seed) as in training."""
    import diverse_channel_vit_amd as dcv
    assert dcv.is_deterministic()
    meta, a = load_golden("jumpcp_s_b16")
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], 8, 224, 161)
    x, y = x.to(gpu_device), y.to(gpu_device)
    runs = []
    for rep in range(2):
        model, _ = build(meta, gpu_device)
        out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss = torch.nn.CrossEntropyLoss()(out, y) + extra
        loss.backward()
        torch.cuda.synchronize()
        runs.append((out.detach().clone(), loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
        del model
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][2].keys() == runs[1][2].keys() and len(runs[0][2]) > 100
    diff = [n for n in runs[0][2] if not torch.equal(runs[0][2][n], runs[1][2][n])]
    assert not diff, f"{len(diff)} gradient tensors differ between two deterministic runs, e.g. {diff[:3]}"


def test_chammi_hcs_nonidentity_mapper_parity(gpu_device):
    """BASELINE config 3 as specified: CHAMMI 12-channel model with enable_sample=True.  The subsets the reference drew are
    pinned through hcs_sampler; on HPA / CP the sampled GLOBAL ids (rows of channel_embed / channel_emb_proxies) differ from
    their POSITIONS in the chunk's tensor.  Features, losses, and the gradients accumulated over a round's
    three chunks against the real reference."""
    import diverse_channel_vit_amd as dcv
    meta, a = load_golden("chammi_hcs")
    k = 0
    for rnd in range(2):
        model, _ = build(meta, gpu_device)
        model.stochastic_weight_rounding = False
        for d in meta["draws"][3 * rnd:3 * rnd + 3]:
            ch = meta["mapper"][d["chunk"]]
            picked = a[f"d{k}_picked"].tolist()
            model.hcs_sampler = lambda m, chunk, cur, picked=picked: (picked, [cur.index(c) for c in picked])
            x, y = orc.make_batch(d["batch_seed"], 2, len(ch), meta["img"], meta["num_classes"])
            feat, extra = model(x.to(gpu_device), d["chunk"], init_first_layer=None, new_channel_init=None, cur_epoch=0)
            loss = dcv.proxy_loss(model.proxies, feat, y.to(gpu_device), model.scale) + 1.0 * extra
            loss.backward()
            ref = a[f"d{k}_feat"]
            assert np.abs(feat.detach().cpu().numpy() - ref).max() <= 3e-2 * np.abs(ref).max(), d
            assert abs(extra.item() - float(a[f"d{k}_extra"])) <= 2e-2 * abs(float(a[f"d{k}_extra"])) + 1e-6
            # Derived tolerance, not "measured plus margin".  proxy_loss (loss_fn.py:7-21) is cross-entropy over the
            # logits -|s f^ - s p^_k|^2 = 2 s^2 cos(f, p_k) + const with s^2 = 1/temperature = 14.29 and f^, p^ unit vectors, so
            # g = d loss / d f^ = 2 s^2 sum_k (softmax_k - y_k) p^_k with |g| <= 2 s^2 sqrt(2) = 40.4 (|softmax - y|_2 <= sqrt 2).
            #   worst case:  |d loss| <= 40.4 e,  e = batch mean of |f^_hip - f^_ref|, the error of the NORMALISED feature;
            #   expected:    the bf16 rounding error of f^ has no preferred direction among the D = 384 coordinates while g is one
            #                fixed direction, so d loss = <g, df^> has standard deviation 40.4 e / sqrt(D) = 2.06 e: asserted at 3 sigma.
            # e itself is bounded at 8e-3 (measured 2e-3 .. 5.7e-3: largest on the 1-channel draws, whose 197-token sequences
            # average the rounding of fewer tokens into the CLS feature) — that bound is what a regression in the kernels would break.
            fh = torch.nn.functional.normalize(feat.detach().double().cpu(), dim=-1)
            fr = torch.nn.functional.normalize(torch.from_numpy(ref).double(), dim=-1)
            e = (fh - fr).norm(dim=-1).mean().item()
            dl = abs(loss.item() - float(a[f"d{k}_loss"]) - (extra.item() - float(a[f"d{k}_extra"])))
            gmax = 2 * math.sqrt(2) / meta["cfg"]["temperature"]
            print(f"chammi-hcs draw {k} ({d['chunk']}, {len(picked)} ch): normalised-feature error {e:.3e}  |d main loss| {dl:.3e}  "
                  f"3 sigma {3 * gmax * e / math.sqrt(fh.shape[-1]):.3e}  worst case {gmax * e:.3e}")
            assert e <= 8e-3, (d, e)
            assert dl <= 3 * gmax * e / math.sqrt(fh.shape[-1]) + 1e-5, (d, dl, e)
            k += 1
        assert sorted(model.feature_extractor.patch_embed.counter.keys()) == sorted({c for j in range(3 * rnd, 3 * rnd + 3) for c in a[f"d{j}_picked"].tolist()})
        _golden_grad_check(model, a, prefix=f"r{rnd}/")


def test_base_64_channels_12545_tokens_forward(gpu_device):
    """BASELINE config 5 as a WHOLE model: DiChaViT-Base, 64 channels x 196 patches + CLS = 12 545 tokens, batch 1, forward
    logits against the real reference's (tests/golden/base64_fwd.npz; the reference materialises 7.5 GB of attention
    scores per layer for this)."""
    meta, a = load_golden("base64_fwd")
    model, _ = build(meta, gpu_device, train=False)
    x, _ = orc.make_batch(112, 1, 64, 224, 161)
    with torch.inference_mode():
        out = model(x.to(gpu_device), "train", None, init_first_layer=None, new_channel_init=None)
    lg = a["logits"]
    err = np.abs(out.cpu().numpy() - lg).max()
    print(f"base/64ch/N=12545 forward: max |dlogit| {err:.3e} (max |logit| {np.abs(lg).max():.3f})")
    assert err <= 3e-2 * np.abs(lg).max()


def test_base_64_channels_12545_tokens_train_step_against_the_oracle_on_the_device(gpu_device):
    """BASELINE config 5 as a whole-model TRAIN step at its full size (VERDICT r4 missing 5): DiChaViT-Base, 64 channels x 196 patches + CLS =
    12 545 tokens, batch 1 — forward, losses, backward, every parameter gradient.  The real reference cannot produce a backward fixture at this
    size in the build container (90 GB of saved fp32 attention matrices against 64 GB of host memory; its forward logits are
    tests/golden/base64_fwd.npz, checked by the test above), so the CHECKER here is the oracle — the pinned restatement of the reference
    (tests/test_oracle_golden.py) — run in fp32 ON THE DEVICE, where its 122 GB of activations fit (test infrastructure only: the product never
    imports it).  Tolerances are those of the golden train-step tests: logits 3e-2 of max, loss 1.2e-2 (Base width), every gradient 5e-2
    relative L2 and cosine 0.998."""
    free, _ = torch.cuda.mem_get_info()
    if free < 150e9:
        pytest.skip("needs 150 GB of free device memory for the fp32 checker")
    meta, a = load_golden("base64_fwd")
    model, st = build(meta, gpu_device)
    model.stochastic_weight_rounding = False
    x, y = orc.make_batch(112, 1, 64, 224, 161)
    x, y = x.to(gpu_device), y.to(gpu_device)
    out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    loss = torch.nn.CrossEntropyLoss()(out, y) + extra
    loss.backward()
    lg = a["logits"]
    assert np.abs(out.detach().cpu().numpy() - lg).max() <= 3e-2 * np.abs(lg).max()  # the reference's own forward at this size
    sd = {k: v.to(gpu_device).float().requires_grad_(True) for k, v in st.items()}
    ch = list(range(64))
    ref_loss, _, ref_extra, ref_logits = orc.train_loss(sd, x, y, meta["cfg"], ch, ch)
    ref_loss.backward()
    err = (out.detach() - ref_logits.detach()).abs().max().item()
    print(f"base/64ch/N=12545 train step: max |dlogit| {err:.3e} (max |logit| {ref_logits.abs().max().item():.3f}) loss {loss.item():.6f} (oracle {ref_loss.item():.6f})")
    assert err <= 3e-2 * ref_logits.abs().max().item()
    assert abs(extra.item() - ref_extra.item()) <= 2e-2 * abs(ref_extra.item()) + 1e-6
    assert abs(loss.item() - ref_loss.item()) <= 1.2e-2
    worst, n_checked = 0.0, 0
    for name, p in model.named_parameters():
        if name not in sd or name.startswith("adaptive_interface"):
            continue
        r = sd[name].grad
        if p.grad is None:
            assert r is None or float(r.abs().max()) == 0.0, name
            continue
        g, r = p.grad.double().flatten(), r.double().flatten()
        rel = ((g - r).norm() / r.norm()).item()
        cos = (torch.dot(g, r) / (g.norm() * r.norm())).item()
        assert rel <= 5e-2 and cos >= 0.998, (name, rel, cos)
        worst = max(worst, rel)
        n_checked += 1
    assert n_checked > 100
    print(f"   {n_checked} gradients, worst relative L2 error {worst:.3e}")
    del sd, ref_loss, ref_logits
    torch.cuda.empty_cache()


def test_pos_table_early_out_with_several_channels(gpu_device):
    """The reference's interpolate_pos_encoding early-out hit with C > 1 (4 channels x 4 patches = the model's 16 positions):
    pos_embed[1+t] per token ACROSS the channels.  tests/golden/resolution_quirk.npz."""
    meta, a = load_golden("resolution_quirk")
    model, _ = build(meta, gpu_device)
    x, y = orc.make_batch(196, 2, 4, meta["img_in"], 6)
    out, extra = model(x.to(gpu_device), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
    loss = torch.nn.functional.cross_entropy(out, y.to(gpu_device)) + extra
    loss.backward()
    assert np.abs(out.detach().cpu().numpy() - a["logits"]).max() <= 3e-2 * np.abs(a["logits"]).max()
    assert abs(loss.item() - float(a["loss"])) <= 5e-3
    fe = model.feature_extractor
    for key, p in (("gpos", fe.pos_embed), ("gchan", fe.patch_embed.channel_embed.weight), ("gcls", fe.cls_token)):
        g, ref = p.grad.cpu().numpy(), a[key]
        assert np.linalg.norm(g - ref) <= 5e-2 * np.linalg.norm(ref), (key, np.linalg.norm(g - ref), np.linalg.norm(ref))
    gp = fe.patch_embed.proj.weight.grad.norm().item()
    assert abs(gp - float(a["gnorm_proj"])) <= 5e-2 * gp
    model.eval()
    with torch.inference_mode():
        ev = model(x.to(gpu_device), "train", None, new_channel_init=None)
    assert np.abs(ev.cpu().numpy() - a["eval"]).max() <= 3e-2 * np.abs(a["eval"]).max()


def test_hcs_projected_input_mode(gpu_device):
    """hcs_sampling=lowest_cosine_prob_proj (dichavit.py:156-161): the projected-input cosine matrix from the tokeniser kernels
    against the reference's, the step on the subsets the reference drew, and the built-in sampler's bookkeeping."""
    meta, a = load_golden("hcs_proj")
    model, _ = build(meta, gpu_device)
    x, y = orc.make_batch(44, 3, 6, 32, 7)
    xg = x.to(gpu_device)
    model._ensure_arena(gpu_device)
    with torch.no_grad():
        cos = model._proj_cosine(xg, list(range(6)))
    assert np.abs(cos.cpu().numpy() - a["cos"]).max() <= 5e-3
    for k, d in enumerate(meta["draws"]):
        picked = a[f"d{k}_picked"].tolist()
        model.hcs_sampler = lambda m, chunk, cur, picked=picked: (picked, [cur.index(c) for c in picked])
        model.zero_grad(set_to_none=True)
        out, extra = model(xg, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss = torch.nn.CrossEntropyLoss()(out, y.to(gpu_device)) + extra
        assert np.abs(out.detach().cpu().numpy() - a[f"d{k}_logits"]).max() <= 3e-2 * np.abs(a[f"d{k}_logits"]).max()
        assert abs(loss.item() - float(a[f"d{k}_loss"])) <= 5e-3
    model.hcs_sampler = None
    model.feature_extractor.patch_embed.counter.clear()
    random.seed(11)
    out, _ = model(xg, "train", None)
    assert 1 <= len(model.feature_extractor.patch_embed.counter) <= 6 and out.shape == (3, 7)
    model.cfg["hcs_sampling"] = "lowest_cosine_proj"  # the reference rejects every other *_proj spelling (:206)
    with pytest.raises(ValueError):
        model(xg, "train", None)


def test_eval_subset_channels_and_feature_dump(gpu_device, tmp_path):
    """SURVEY §8f row 4 remainder.  eval_subset_channels (trainer.py:474-545): the sweep REPLACES mapper[chunk] by the selected
    positions and evaluates on the sliced batch — logits must equal the oracle's for those channel ids.  dump_features
    (eval_morphem70k's feature pass, trainer.py:645-690): per-chunk .npy files of eval-mode features with the leave-one-out
    channel initialisation, equal to the oracle's features."""
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("eval_newch")  # train [0..4], test [0,1,5,3,6]: 7-channel model, 9 classes
    model, st = build(meta, gpu_device, train=False)
    batches = [orc.make_batch(300 + i, 3, 5, 32, 9) for i in range(2)]
    res = dcv.eval_subset_channels(model, batches, meta["mapper"]["train"], chunk_name="test", only_sizes=[5, 2], device=gpu_device)
    assert len(res[5]) == 1 and len(res[2]) == 10
    assert model.feature_extractor.patch_embed.mapper["test"] == [3, 4]  # the last combination stays, as in the reference
    sd = {k: v.double() for k, v in st.items()}
    sel = [1, 3]
    model.feature_extractor.patch_embed.mapper["test"] = sel
    x = batches[0][0]
    with torch.inference_mode():
        out = model(x[:, sel].to(gpu_device), "test", None, new_channel_init="")
    ref, _ = orc.forward(sd, x[:, sel].double(), meta["cfg"], sel, [0, 1])
    assert (out.cpu().double() - ref).abs().max().item() <= 3e-2 * ref.abs().max().item()
    hits = sum(int((orc.forward(sd, xb[:, sel].double(), meta["cfg"], sel, [0, 1])[0].argmax(-1) == yb).sum()) for xb, yb in batches)
    combos = [list(c) for c in __import__("itertools").combinations(range(5), 2)]
    # the accounting (correct / total per combination, combination order) exactly, against the argmax of the model's own logits ...
    own = 0
    with torch.inference_mode():
        for xb, yb in batches:
            own += int((model(xb[:, sel].to(gpu_device), "test", None, new_channel_init="").argmax(-1).cpu() == yb).sum())
    assert abs(res[2][combos.index(sel)] - 100.0 * own / 6) < 1e-9
    # ... and against the oracle with at most one sample flipped by a bf16 near-tie
    assert abs(res[2][combos.index(sel)] - 100.0 * hits / 6) <= 100.0 / 6 + 1e-9
    # feature dump with leave-one-out initialisation on a CHAMMI-style (headless) model
    meta2, _ = load_golden("chammi")
    model2, st2 = build(meta2, gpu_device, train=False)
    loaders = {c: [orc.make_batch(400 + len(meta2["mapper"][c]) + i, 2, len(meta2["mapper"][c]), meta2["img"], 14)[0] for i in range(2)]
               for c in ("Allen", "HPA")}
    paths = dcv.dump_features(model2, loaders, str(tmp_path / "feats"), "features.npy", training_chunks="Allen_CP",
                              new_channel_init="avg_2", device=gpu_device)
    assert [p.split("/")[-2] for p in paths] == ["Allen", "HPA"]
    sd2 = {k: v.double() for k, v in st2.items()}
    E = sd2["feature_extractor.patch_embed.channel_embed.weight"]
    for c, pth in zip(("Allen", "HPA"), paths):
        f = np.load(pth)
        assert f.shape == (4, 384) and f.dtype == np.float32
        rows = orc.eval_channel_embed(E, meta2["mapper"], c, "Allen_CP", "avg_2")
        ch = meta2["mapper"][c]
        ref = torch.cat([orc.forward(sd2, xb.double(), meta2["cfg"], ch, list(range(len(ch))), channel_embed_rows=rows)[0] for xb in loaders[c]])
        assert np.abs(f - ref.numpy()).max() <= 3e-2 * ref.abs().max().item(), c


def test_graph_replays_without_host_sync_follow_eager(gpu_device):
    """the capturable optimiser's scalars (lr, weight decay, bias corrections 1/(1-b^t), which change 4x over the
    first steps) reach the device BY VALUE in stream order (dcv_adamw_set_hyper), so a host that enqueues many replays ahead of
    the device cannot overwrite a step's scalars before it runs.  12 replays are queued with NO host sync in between and a
    changing lr; losses and weights must follow the eager run that syncs every step."""
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("so2sat_s")
    x, y = orc.make_batch(78, 4, 18, 32, 17)
    x, y = x.to(gpu_device), y.to(gpu_device)
    ce = torch.nn.CrossEntropyLoss()
    lrs = [1e-4 * (1 + (s % 5)) for s in range(14)]
    out = {}
    for mode in ("eager", "graph"):
        model, _ = build(meta, gpu_device)
        model.stochastic_weight_rounding = False
        opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=lrs[0], weight_decay=0.04, model=model,
                           capturable=(mode == "graph"))
        if mode == "eager":
            for s in range(14):
                opt.param_groups[0]["lr"] = lrs[s]
                opt.zero_grad()
                o, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
                loss = ce(o, y) + extra
                loss.backward()
                opt.step()
                torch.cuda.synchronize()
            out[mode] = (loss.item(), model.feature_extractor.blocks[5].attn.qkv.weight.detach().clone(), opt._step)
        else:
            opt.param_groups[0]["lr"] = lrs[0]
            gs = dcv.GraphedTrainStep(model, opt, "train", None, ce, 1.0, warmup=2)
            # warm-up steps 0,1 run inside the first call with param_groups' lr at call time: feed them lrs[0], lrs[1]
            real_advance = opt.advance
            state = {"s": 0}

            def advance():
                opt.param_groups[0]["lr"] = lrs[state["s"]]
                state["s"] += 1
                real_advance()

            opt.advance = advance
            for s in range(12):  # first call: 2 eager warm-ups + capture + replay = steps 0, 1, 2; then 11 more replays
                loss = gs(x, y)   # no .item(), no synchronize: the host runs ahead of the device
            torch.cuda.synchronize()
            out[mode] = (loss.item(), model.feature_extractor.blocks[5].attn.qkv.weight.detach().clone(), opt._step)
    assert out["eager"][2] == out["graph"][2] == 14
    assert abs(out["eager"][0] - out["graph"][0]) <= 2e-3, (out["eager"][0], out["graph"][0])
    diff = (out["eager"][1] - out["graph"][1]).abs()
    # fp32-atomic ordering noise can flip the sign of a near-zero gradient element, which moves Adam's sign-like step by up to
    # 2 lr (1e-3) on single elements; scalars of the WRONG step (the race this test guards) would shift every element by ~lr
    assert diff.max().item() <= 1.5e-3 and diff.mean().item() <= 2e-5, (diff.max().item(), diff.mean().item())


def _two_rank_worker(rank, world, port, q, grad_dtype, overlap, backend="gloo"):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    # gloo: both ranks on cuda:0 (RCCL refuses two ranks on one device); nccl (= RCCL): one GPU per rank, real asynchronous collectives
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import diverse_channel_vit_amd as dcv
        meta, _ = load_golden("tiny_e2e")
        ce = torch.nn.CrossEntropyLoss()
        batches = {(r, k): orc.make_batch(500 + 10 * r + k, 2, 3, 32, 5) for r in range(world) for k in range(2)}
        model, _ = build(meta, dev)
        model.stochastic_weight_rounding = False
        model.wgrad_stream = (grad_dtype == "float32" and overlap)  # one of the three variants keeps the two-stream hand-over under test
        dp = dcv.DataParallel(model, min_bucket_bytes=1 << 18, grad_dtype=getattr(torch, grad_dtype), overlap=overlap)
        dp.broadcast_parameters(0)
        dp.hook_misc_params()  # before the first forward (INTEGRATION.md order)
        for k in range(2):  # two backward passes per step
            x, y = batches[(rank, k)]
            o, extra = model(x.to(dev), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
            (ce(o, y.to(dev)) + extra).backward()
        torch.cuda.synchronize()
        got = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}
        res = None
        if rank == 0:  # single-process sum over both ranks' batches and both passes, divided by the world size
            ref_model, _ = build(meta, dev)
            ref_model.stochastic_weight_rounding = False
            for k in range(2):
                for r in range(world):
                    x, y = batches[(r, k)]
                    o, extra = ref_model(x.to(dev), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
                    (ce(o, y.to(dev)) + extra).backward()
            worst = 0.0
            for n, p in ref_model.named_parameters():
                if p.grad is None:
                    assert n not in got, n
                    continue
                ref = p.grad.detach().double().cpu() / world
                rel = (got[n] - ref).norm().item() / (ref.norm().item() + 1e-30)
                worst = max(worst, rel)
            res = worst
        q.put((rank, res, dp.buckets_launched, len(dp._hooks)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("grad_dtype,overlap", [("float32", True), ("bfloat16", True), ("float32", False)])
def test_dp_two_ranks_real_model_two_backwards(gpu_device, grad_dtype, overlap):
    """The REAL model + HIP kernels under DataParallel on TWO ranks (both on this box's one GPU; gloo, because RCCL refuses two
    ranks on one device — dp stages gloo reductions through the host), two backward passes per optimiser step, INTEGRATION.md's
    call order, no explicit finalize: gradients must equal the single-process sum over both ranks' batches / world size."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, q, grad_dtype, overlap)) for r in range(2)]
    for p in procs:
        p.start()
    import queue as _q
    import time as _t
    res, t0 = [], _t.time()
    while len(res) < 2:
        try:
            res.append(q.get(timeout=2))
        except _q.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or _t.time() - t0 > 500:
                for p in procs:
                    if p.is_alive():
                        p.terminate()
                pytest.fail(f"a rank exited with {dead} (or timed out)")
    for p in procs:
        p.join(60)
    for rank, worst, nb, nh in res:
        assert nb >= (2 if overlap else 1) and nh <= 8
        if rank == 0:
            print(f"two ranks, two backward passes: worst relative gradient difference vs single-process sum {worst:.2e}")
            # fp32 exchange: the atomic ordering noise of the weight-gradient GEMMs only; bf16 exchange: every bucket element rounded to bf16
            # once per pass (2^-9 relative per element)
            assert worst <= (2e-3 if grad_dtype == "float32" else 8e-3), worst


def _torch_ddp_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import diverse_channel_vit_amd as dcv
        meta, _ = load_golden("tiny_e2e")
        ce = torch.nn.CrossEntropyLoss()
        batches = {r: orc.make_batch(700 + r, 2, 3, 32, 5) for r in range(world)}
        model, _ = build(meta, dev)
        model.stochastic_weight_rounding = False
        ddp = DDP(model, device_ids=[0], find_unused_parameters=True)  # trainer.py:1185, verbatim
        opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.04, model=model)
        x, y = batches[rank]
        opt.zero_grad()
        o, extra = ddp(x.to(dev), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        (ce(o, y.to(dev)) + extra).backward()
        torch.cuda.synchronize()
        got = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}
        opt.step()  # the fused optimiser reads the arena the DDP reducer wrote the averaged gradients back into
        torch.cuda.synchronize()
        w_after = model.feature_extractor.blocks[0].attn.qkv.weight.detach().double().cpu()
        res = None
        if rank == 0:
            ref_model, _ = build(meta, dev)
            ref_model.stochastic_weight_rounding = False
            ropt = dcv.HipAdamW([p for p in ref_model.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.04, model=ref_model)
            ropt.zero_grad()
            for r in range(world):
                x, y = batches[r]
                o, extra = ref_model(x.to(dev), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
                ((ce(o, y.to(dev)) + extra) / world).backward()
            worst = 0.0
            for n, p in ref_model.named_parameters():
                if p.grad is None:
                    assert n not in got, n
                    continue
                ref = p.grad.detach().double().cpu()
                worst = max(worst, (got[n] - ref).norm().item() / (ref.norm().item() + 1e-30))
            ropt.step()
            torch.cuda.synchronize()
            wr = ref_model.feature_extractor.blocks[0].attn.qkv.weight.detach().double().cpu()
            res = (worst, (w_after - wr).abs().max().item())
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_torch_ddp_wrapper_of_the_reference_trainer(gpu_device):
    """Row a16 as the reference's trainer does it, unchanged: `DDP(model, device_ids=[local_rank], find_unused_parameters=True)`
    (trainer.py:1185) around THIS model — two ranks (both on this box's one GPU, gloo), one step: torch's reducer walks the autograd graph
    through the hand-written encoder node, copies the arena's gradient views into its buckets, averages, writes them back, and the fused
    HipAdamW then steps from the arena.  Gradients equal the single-process average over both ranks' batches; the updated weights agree."""
    import socket
    import queue as _q
    import time as _t
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_torch_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res, t0 = [], _t.time()
    while len(res) < 2:
        try:
            res.append(q.get(timeout=2))
        except _q.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or _t.time() - t0 > 500:
                for p in procs:
                    if p.is_alive():
                        p.terminate()
                pytest.fail(f"a rank exited with {dead} (or timed out)")
    for p in procs:
        p.join(60)
    for rank, r in res:
        if rank == 0:
            worst, dw = r
            print(f"torch DDP around the model: worst relative gradient difference vs single-process average {worst:.2e}, max |dW| after the step {dw:.2e}")
            assert worst <= 2e-3 and dw <= 2.1e-3  # Adam's first step moves every weight by ~lr = 1e-3: a wrong gradient sign would show as 2e-3


@pytest.mark.timeout(600)
@pytest.mark.parametrize("grad_dtype,overlap", [("float32", True), ("bfloat16", True), ("float32", False)])
def test_dp_two_ranks_rccl_two_gpus(gpu_device, grad_dtype, overlap):
    """the same two-rank check over REAL RCCL — one GPU per rank, asynchronous all-reduces issued from the
    weight-gradient stream while the backward continues, the autograd-engine end-of-backward callback as the only synchronisation.
    Needs two visible GPUs: skipped on the one-GPU test boxes (no run on more than one GPU exists yet: DESIGN.md section 5), runs
    wherever `pytest -m gpu` sees a multi-GPU node."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device)")
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, q, grad_dtype, overlap, "nccl")) for r in range(2)]
    for p in procs:
        p.start()
    import queue as _q
    import time as _t
    res, t0 = [], _t.time()
    while len(res) < 2:
        try:
            res.append(q.get(timeout=2))
        except _q.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or _t.time() - t0 > 500:
                for p in procs:
                    if p.is_alive():
                        p.terminate()
                pytest.fail(f"a rank exited with {dead} (or timed out)")
    for p in procs:
        p.join(60)
    for rank, worst, nb, nh in res:
        assert nb >= (2 if overlap else 1) and nh <= 8
        if rank == 0:
            print(f"two ranks over RCCL: worst relative gradient difference vs single-process sum {worst:.2e}")
            assert worst <= (2e-3 if grad_dtype == "float32" else 8e-3), worst


class _EmulatedWork:
    def __init__(self, done, dev, broken=False):
        self.done, self.dev, self.broken = done, dev, broken

    def wait(self):
        if not self.broken:
            torch.cuda.current_stream(self.dev).wait_event(self.done)  # what ProcessGroupNCCL's Work.wait() does: a stream wait, no host block
        return True


class _EmulatedRccl:
    """Stands in for ``torch.distributed`` (DataParallel's dist_module) with RCCL's STREAM semantics, for one rank of a two-rank job on a
    one-GPU box: every all-reduce runs asynchronously on a stream of its own, ordered after the issuing stream's position at the call
    (an event recorded there), completes LATE (a spin kernel first), averages in place with what the peer rank contributed to the same
    collective, and hands back a Work whose wait() is a stream wait.  peer=None: the recording pass of the peer rank (its k-th buffer is
    copied on the collective's stream)."""

    class ReduceOp:
        SUM, AVG = "sum", "avg"

    def __init__(self, dev, peer=None, delay_cycles=12_000_000, broken_wait=False):  # ~5 ms per collective on this clock
        self.dev, self.peer, self.delay, self.broken = dev, peer, delay_cycles, broken_wait
        # high priority: HIP maps streams onto a few hardware queues, and a collective stream that shares its queue with the compute stream
        # would run in enqueue order with it — nothing would be asynchronous and the missing-wait control would pass for the wrong reason
        self.stream = torch.cuda.Stream(dev, priority=-1)
        self.rec, self.k = [], 0

    def is_initialized(self):
        return True

    def get_world_size(self, group=None):
        return 2

    def get_backend(self, group=None):
        return "nccl"

    def broadcast(self, t, src=0, group=None, async_op=False):
        return None

    def all_reduce(self, buf, op=None, group=None, async_op=False):
        assert async_op and buf.is_cuda
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        buf.record_stream(self.stream)
        with torch.cuda.stream(self.stream):
            # every allocation BEFORE the spin kernel: one behind it may reach hipMalloc, which synchronises the device — the host would
            # sit out the delay and the late collective would no longer be late (the missing-wait control then fails to fail)
            if self.peer is None:
                keep = torch.empty_like(buf)
            else:
                other = self.peer[self.k]
                assert other.shape == buf.shape and other.dtype == buf.dtype, (self.k, other.shape, buf.shape)
                other32, tmp = other.float(), torch.empty(buf.shape, dtype=torch.float32, device=buf.device)
            done = torch.cuda.Event()
            self.stream.wait_event(ev)
            torch.cuda._sleep(self.delay)
            if self.peer is None:
                self.rec.append(keep.copy_(buf.detach()))
            else:
                tmp.copy_(buf)
                tmp.add_(other32).mul_(0.5 if op == self.ReduceOp.AVG else 1.0)
                buf.copy_(tmp)
            done.record(self.stream)
        self.k += 1
        return _EmulatedWork(done, self.dev, self.broken)


@pytest.mark.parametrize("two_streams", [True, False])
@pytest.mark.parametrize("grad_dtype,overlap", [("float32", True), ("bfloat16", True), ("float32", False)])
def test_dp_async_collectives_emulated_on_one_gpu(gpu_device, grad_dtype, overlap, two_streams):
    """gloo is synchronous through the host and RCCL refuses two ranks on one device, so the ORDERING of the default
    data-parallel backward — buckets handed over from the weight-gradient stream while the backward continues, the autograd engine's
    end-of-backward callback as the only synchronisation — was never run against collectives that are really asynchronous and really
    change the data.  Here they are (_EmulatedRccl): rank 1's contributions are recorded in a first pass, then rank 0 runs with
    collectives that land late on their own stream.  The gradients are snapshotted ON THE COMPUTE STREAM straight after backward()
    (no device synchronisation before: a consumer that did not wait would read un-averaged values) and must equal the single-process
    sum over both ranks' batches / 2.  Control: the same run with a wait() that does nothing must FAIL that comparison."""
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("tiny_e2e")
    dev = gpu_device
    ce = torch.nn.CrossEntropyLoss()
    batches = {r: orc.make_batch(700 + r, 2, 3, 32, 5) for r in range(2)}

    def one_rank(rank, comm):
        model, _ = build(meta, dev)
        model.stochastic_weight_rounding = False
        model.wgrad_stream = two_streams  # buckets handed over from the weight-gradient stream (True) or from the compute stream (the default)
        dp = dcv.DataParallel(model, min_bucket_bytes=1 << 18, grad_dtype=getattr(torch, grad_dtype), overlap=overlap, dist_module=comm)
        dp.hook_misc_params()
        snaps = []
        x, y = batches[rank][0].to(dev), batches[rank][1].to(dev)
        for step in range(2):  # the second step reuses the arena, the side stream and the events of the first
            model.zero_grad(set_to_none=True)
            # snapshot buffers exist BEFORE the backward: an allocation after it may reach hipMalloc, which synchronises the device and
            # would hide a missing wait (the control below failed to fail for exactly that reason once)
            bufs = {n: torch.empty_like(p) for n, p in model.named_parameters()}
            o, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
            (ce(o, y) + extra).backward()
            snap = {}
            for n, p in model.named_parameters():
                if p.grad is not None:
                    snap[n] = bufs[n].copy_(p.grad.detach())  # stream-ordered only
            snaps.append(snap)
        torch.cuda.synchronize()
        return snaps, dp

    rec = _EmulatedRccl(dev, peer=None)
    one_rank(1, rec)
    assert len(rec.rec) >= 2 * (2 if overlap else 1)

    ref_model, _ = build(meta, dev)
    ref_model.stochastic_weight_rounding = False
    for r in range(2):
        x, y = batches[r]
        o, extra = ref_model(x.to(dev), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        (ce(o, y.to(dev)) + extra).backward()
    torch.cuda.synchronize()
    ref = {n: p.grad.detach().double() / 2 for n, p in ref_model.named_parameters() if p.grad is not None}

    def worst_of(snap):
        assert snap.keys() == ref.keys()
        return max((snap[n].double() - ref[n]).norm().item() / (ref[n].norm().item() + 1e-30) for n in ref)

    snaps, dp = one_rank(0, _EmulatedRccl(dev, peer=[t.clone() for t in rec.rec]))
    assert dp.buckets_launched >= 2 * (2 if overlap else 1)
    tol = 2e-3 if grad_dtype == "float32" else 8e-3
    for step, snap in enumerate(snaps):
        w = worst_of(snap)
        print(f"emulated asynchronous collectives, step {step}: worst relative gradient difference vs single-process sum {w:.2e}")
        assert w <= tol, (step, w)
    # control: the test can see a missing wait
    snaps_bad, _ = one_rank(0, _EmulatedRccl(dev, peer=[t.clone() for t in rec.rec], broken_wait=True))
    assert worst_of(snaps_bad[0]) > 10 * tol, "a wait() that does nothing went unnoticed: the emulation has no teeth"


@pytest.mark.parametrize("private,group,two_streams", [(False, False, True), (True, False, True), (False, False, False), (True, True, False)])
def test_backward_scratch_and_grouping_fallbacks(gpu_device, private, group, two_streams):
    """The backward's switches (dichavit.py, _BackwardScratch and _block_backward): per-layer scratch or two shared buffers with reader waits, a block's four weight
    gradients in one grouped launch or in four, one stream or two.  Every combination is the same arithmetic up to the split of the weight-gradient
    sums over the token rows: the gradients must agree with the default configuration's (private scratch, grouped, one stream) to fp32 rounding."""
    meta, a = load_golden("so2sat_s")
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    grads = {}
    for cfg in ("default", "variant"):
        model, _ = build(meta, gpu_device)
        model.stochastic_weight_rounding = False
        if cfg == "variant":
            model.wgrad_private_scratch, model.wgrad_group, model.wgrad_stream = private, group, two_streams
        for _ in range(2):  # a second pass reuses the scratch the first one left in the allocator
            model.zero_grad(set_to_none=True)
            out, extra = model(x.to(gpu_device), meta["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
            (torch.nn.CrossEntropyLoss()(out, y.to(gpu_device)) + extra).backward()
        torch.cuda.synchronize()
        grads[cfg] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    assert grads["default"].keys() == grads["variant"].keys()
    for n, g in grads["variant"].items():
        ref = grads["default"][n]
        err = (g - ref).abs().max().item()
        assert err <= 1e-5 * ref.abs().max().item() + 1e-9, (n, err, ref.abs().max().item())


def test_weight_gradients_on_second_stream_match_one_stream(gpu_device):
    """The backward runs the weight-gradient GEMMs on a second HIP stream (dichavit.py, _BackwardScratch: wgrad_stream).  Same
    kernels on the same operands as the one-stream backward: every gradient must agree up to the order of the fp32 atomic adds of
    the split reductions (each launch's own order is not fixed either), over several steps (the scratch buffers the side stream
    reads are reused every layer and every step) and against the fp64 oracle."""
    meta, a = load_golden("so2sat_s")
    x, y = orc.make_batch(meta["seed"] + 1, meta["B"], meta["C_in"], meta["img"], meta["num_classes"])
    grads = {}
    for mode in (True, False):
        model, _ = build(meta, gpu_device)
        model.wgrad_stream = mode
        for _ in range(3):  # repeated backward passes: same result every time
            model.zero_grad(set_to_none=True)
            out, extra = model(x.to(gpu_device), meta["chunk"], None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
            (torch.nn.CrossEntropyLoss()(out, y.to(gpu_device)) + extra).backward()
        torch.cuda.synchronize()
        grads[mode] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        if mode:
            ch = meta["mapper"][meta["chunk"]]
            sd_ref, *_ = oracle_grads(meta, x, y, ch, list(range(len(ch))))
            check_grads(model, sd_ref)
    assert grads[True].keys() == grads[False].keys()
    for n, g in grads[True].items():
        ref = grads[False][n]
        err = (g - ref).abs().max().item()
        assert err <= 1e-5 * ref.abs().max().item() + 1e-9, (n, err, ref.abs().max().item())
