"""DiChaViT.forward_views and one complete DINO step on the MI355X: a two-block model at the tiny width (D = 192), 3 channels, B 2, 224 x 224
global and 96 x 96 local views, stochastic weight rounding on.  No test asserts that the loss falls."""
import pytest
import torch

from conftest import load_golden
from switch_pairs import install_recorder

pytestmark = pytest.mark.gpu

CHUNK, B, K = "train", 2, 1000


class Cfg(dict):
    def __getattr__(self, key):  # missing settings read as None; dunder lookups (copy.deepcopy's) must still fail
        if key.startswith("__"):
            raise AttributeError(key)
        return self.get(key)


def new_model(device, seed=3):
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("tiny_e2e")
    torch.manual_seed(seed)
    cfg = Cfg(meta["cfg"], in_channel_names=["c0", "c1", "c2"], img_size=[224], num_classes=meta["num_classes"])
    model = dcv.dichavit(cfg, mapper={CHUNK: [0, 1, 2]})
    fe = model.feature_extractor
    fe.blocks = torch.nn.ModuleList(list(fe.blocks)[:2])  # before the first forward: the arena is laid out from the blocks that are left
    model.classifer_head.requires_grad_(False)  # forward_views does not return the classifier head's output
    model.proxies.requires_grad_(False)
    model = model.to(device).train()
    assert model.stochastic_weight_rounding
    return model


def views(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2 * B, 3, 224, 224, generator=g).cuda(), torch.randn(3 * B, 3, 96, 96, generator=g).cuda()


def names(log, start=0):
    return [n for n, _ in log[start:]]


def test_one_stochastic_refresh_per_call(gpu_device, monkeypatch):
    model = new_model(gpu_device)
    xg, xl = views()
    model.forward_views([xg], CHUNK)  # builds the arena and the seed word
    seed0 = int(model._sr_seed.item())
    log = install_recorder(monkeypatch.setattr)
    feats, extra = model.forward_views([xg, xl], CHUNK)
    assert feats.shape == (5 * B, model.dim) and feats.requires_grad and extra.shape == ()
    n = names(log)
    assert n.count("cast_bf16_sr") == 1 and n.count("cast_transpose_bf16_sr") == 1 and n.count("cast_bf16") == 0 and n.count("cast_transpose_bf16") == 0
    assert int(model._sr_seed.item()) == seed0 + 1
    assert not model._copies_held
    (feats.square().mean() + extra).backward()
    n = names(log)
    assert n.count("cast_bf16_sr") == 1 and int(model._sr_seed.item()) == seed0 + 1, "the backward must not refresh the copies"
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    start = len(log)  # two plain forwards, for contrast: one refresh each
    model(xg, CHUNK)
    model(xg, CHUNK)
    assert names(log, start).count("cast_bf16_sr") == 2 and int(model._sr_seed.item()) == seed0 + 3


def test_single_view_has_the_bits_of_forward_with_features(gpu_device):
    model = new_model(gpu_device)
    xg, _ = views()
    model.forward_views([xg], CHUNK)
    G = torch.randn(2 * B, model.dim, generator=torch.Generator().manual_seed(5)).cuda()
    got = []
    for call in ("taps", "views"):
        model._sr_seed.fill_(17)
        for p in model.parameters():
            p.grad = None
        if call == "taps":
            (_, extra), taps = model.forward_with_features(xg, CHUNK, layers=1, pool="cls")
            feat = taps[0]
        else:
            feat, extra = model.forward_views([xg], CHUNK)
        torch.autograd.backward([feat, extra], [G, torch.ones_like(extra)])  # one backward: the encoder node frees its state in it
        got.append((feat.detach().clone(), extra.detach().clone(), {n: None if p.grad is None else p.grad.clone() for n, p in model.named_parameters()}))
    (f0, e0, g0), (f1, e1, g1) = got
    assert torch.equal(f0, f1) and torch.equal(e0, e1)
    assert sum(g is not None for g in g0.values()) > 20
    for n in g0:
        assert (g0[n] is None) == (g1[n] is None), n
        if g0[n] is not None:
            assert torch.equal(g0[n], g1[n]), n


def test_two_views_in_one_backward_give_the_sum_of_their_gradients(gpu_device):
    """forward_views([xg, xl]) and ONE backward against two separate forward_views([x]) + backward passes on the same weight bits (the seed word
    is set before every call; no HCS, no DropPath in this model).  Every view is its own encoder node and the nodes meet in one backward: a
    parameter's gradient must be the sum of the nodes' gradients — one fp32 addition, so bit for bit for the encoder's parameters, each of which
    gets one gradient per node.  The embeddings also collect the regularisers' gradients, in an order autograd chooses: 1e-6 of their largest
    entry."""
    model = new_model(gpu_device)
    xg, xl = views()
    model.forward_views([xg], CHUNK)
    g = torch.Generator().manual_seed(9)
    Gg, Gl = torch.randn(2 * B, model.dim, generator=g).cuda(), torch.randn(3 * B, model.dim, generator=g).cuda()

    def grads(batches, ups):
        model._sr_seed.fill_(23)
        for p in model.parameters():
            p.grad = None
        feats, extra = model.forward_views(batches, CHUNK)
        ((feats * torch.cat(ups)).sum() + extra).backward()
        return {n: None if p.grad is None else p.grad.detach().clone() for n, p in model.named_parameters()}

    one, two, both = grads([xg], [Gg]), grads([xl], [Gl]), grads([xg, xl], [Gg, Gl])
    swapped = grads([xl, xg], [Gl, Gg])
    enc = {id(p) for p in model._enc_param_list()}
    exact = 0
    for n, p in model.named_parameters():
        if one[n] is None:
            assert both[n] is None, n
            continue
        want = one[n] + two[n]
        assert bool(want.any()), n
        if id(p) in enc:
            assert torch.equal(both[n], want), f"{n}: {(both[n] - want).abs().max().item():.3e} off the sum of the views' gradients"
            assert torch.equal(swapped[n], want), n
            exact += 1
        else:
            tol = 1e-6 * want.abs().max().item()
            assert (both[n] - want).abs().max().item() <= tol and (swapped[n] - want).abs().max().item() <= tol, n
    assert exact == len(enc)
    assert not torch.equal(one["feature_extractor.blocks.0.attn.qkv.weight"], two["feature_extractor.blocks.0.attn.qkv.weight"])


def test_refusals(gpu_device):
    model = new_model(gpu_device)
    xg, _ = views()
    with pytest.raises(ValueError, match="pool"):
        model.forward_views([xg], CHUNK, pool="channel")
    with pytest.raises(ValueError, match="no views"):
        model.forward_views([], CHUNK)
    model._dp = object()
    with pytest.raises(NotImplementedError, match="DataParallel"):
        model.forward_views([xg], CHUNK)
    model._dp = None


def test_one_complete_dino_step(gpu_device, monkeypatch):
    from diverse_channel_vit_amd import AveragedModel, DINOHead, DINOLoss, update_teacher_head
    model = new_model(gpu_device)
    xg, xl = views()
    torch.manual_seed(7)
    head = DINOHead(model.dim, out_dim=K, hidden_dim=64, bottleneck_dim=32).cuda()
    teacher_head = DINOHead(model.dim, out_dim=K, hidden_dim=64, bottleneck_dim=32).cuda()
    teacher_head.load_state_dict(head.state_dict())
    teacher_head.requires_grad_(False)
    crit = DINOLoss(K).cuda()
    crit.center.normal_()
    decay, m_head = 0.75, 0.5
    teacher = AveragedModel(model, avg="ema", decay=decay)
    teacher.update_parameters(model)  # the first update is the copy
    teacher.module.eval()
    params = [p for p in list(model.parameters()) + list(head.parameters()) if p.requires_grad]
    opt = torch.optim.SGD(params, lr=0.05)

    log = install_recorder(monkeypatch.setattr)
    model(xg, CHUNK)
    plain_before = [(n, a) for n, a in log]
    del log[:]

    t_before = {n: p.detach().clone() for n, p in teacher.module.named_parameters()}
    th_before = [p.detach().clone() for p in teacher_head.parameters()]
    c_before = crit.center.clone()
    with torch.no_grad():
        t_feats, _ = teacher.module.forward_views([xg], CHUNK)
        t_logits = teacher_head(t_feats)
    feats, extra = model.forward_views([xg, xl], CHUNK)
    loss = crit(head(feats), t_logits, 0.04, n_views=5) + extra
    opt.zero_grad(set_to_none=True)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for name, p in list(model.named_parameters()) + list(head.named_parameters()):
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), f"{name}: no finite gradient"
    assert any(bool(p.grad.any()) for p in model.feature_extractor.blocks[0].parameters())
    opt.step()
    for n, p in teacher.module.named_parameters():
        assert torch.equal(p, t_before[n]), f"teacher {n} changed before update_parameters"
    assert torch.equal(crit.center, c_before)
    tsum = crit._tsum.clone()
    teacher.update_parameters(model)
    update_teacher_head(teacher_head, head, m_head)
    crit.update_center()
    s_now = dict(model.named_parameters())
    moved = 0
    for n, p in teacher.module.named_parameters():
        want = t_before[n] + (1 - decay) * (s_now[n].detach() - t_before[n])
        assert torch.allclose(p, want, rtol=0, atol=1e-6 * max(1.0, want.abs().max().item())), f"teacher {n}"
        moved += int(not torch.equal(p, t_before[n]))
    assert moved > 20
    for b, t, s in zip(th_before, teacher_head.parameters(), head.parameters()):
        assert torch.allclose(t, m_head * b + (1 - m_head) * s.detach(), rtol=0, atol=1e-6)
    assert (tsum - t_logits.sum(0)).abs().max().item() <= 1e-4 * max(1.0, t_logits.abs().max().item())
    assert torch.equal(crit.center, c_before * 0.9 + tsum * ((1.0 - 0.9) / (2 * B)))

    del log[:]
    model(xg, CHUNK)
    assert [(n, a) for n, a in log] == plain_before, "model(x, chunk) no longer launches what it launched before the DINO step"
