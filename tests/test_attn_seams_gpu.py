"""The persistent dK / dV kernel (csrc/attn_bwd3.hip, attn_bwd_dkdv3p_kernel) where a workgroup walks SEVERAL items: the seam between two items
(dK / dV of the previous item leave through region R, the next item's K / V rows arrive there, the Q / dO ring runs on) in both regimes
(in_loop: trickled over the tiles; !in_loop: all at the seam), with both item maps and every remainder class of dcv_dkdv3_launch.

Two checks per shape of CASES, on the pre-scaled-q chain (attn_fwd3<true>, attn_bwd_dq2<true>, attn_bwd_dkdv3p, TAIL2 / ranged dkdv2<true>):
 A. batch-slice bit identity: image b of the batched run == the same image run alone (B = 1: one item per workgroup, the path
    test_attention_prescaled_q holds against fp32).  No kernel of the chain sums across (batch, head) pairs or uses atomics, and an item's
    arithmetic does not depend on the workgroup that runs it, so anything a seam gets wrong breaks the identity with no tolerance to hide in.
 B. the batched run against the materialised softmax in float64, element by element, at test_attention_prescaled_q's bounds.
Needs an MI355X (256 CUs: the premise `max walk >= 2` is asserted with the device's CU count, not skipped): run with -m gpu."""
import math
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

K3_KEYS = 256  # attn_bwd3.hip:32

Plan = namedtuple("Plan", "B N H Nq cus rem split key_hi nkt items G nt in_loop kv_t0 xcd_map walk_max walk_min tail last_keys idle_waves part_keys")


def dkdv3_plan(B, N, H, Nq, cus):
    """dcv_dkdv3_launch (attn_bwd3.hip:497-510) and the kernel's item dealing (attn_bwd3.hip:53-81, 354-357, 392-397) restated.
    tail: which launch of dcv_dkdv2_range (attn_bwd.hip:506-514) takes the remainder keys; last_keys / idle_waves / part_keys describe the last
    256-key block of a (batch, head): a wave is idle when its first key is >= key_hi (attn_bwd3.hip:395), partly filled when it has 1..63 keys."""
    Nq = N if Nq is None else Nq
    rem = N % K3_KEYS
    split = rem != 0 and rem <= 128 and N > K3_KEYS
    key_hi = N - rem if split else N
    nkt = (key_hi + K3_KEYS - 1) // K3_KEYS
    items = B * H * nkt
    G = min(items, cus)
    nt = (Nq + 63) // 64
    BH = B * H
    xcd_map = BH % 8 == 0 and G % 8 == 0
    if xcd_map:  # per XCD: (BH / 8) * nkt items dealt round-robin to G / 8 workgroups
        m, w = (BH // 8) * nkt, G // 8
    else:
        m, w = items, G
    last_keys = key_hi - (nkt - 1) * K3_KEYS
    return Plan(B=B, N=N, H=H, Nq=Nq, cus=cus, rem=rem, split=split, key_hi=key_hi, nkt=nkt, items=items, G=G, nt=nt, in_loop=nt >= 16,
                kv_t0=(nt - 12) & ~1, xcd_map=xcd_map, walk_max=-(-m // w), walk_min=m // w,
                tail="none" if not split else ("tail2" if rem <= 64 else "ranged"), last_keys=last_keys,
                idle_waves=4 - (last_keys + 63) // 64, part_keys=last_keys % 64)


def item_of(p, g, k):
    """k-th item of workgroup g as (batch-head, key block), None behind the last one (attn_bwd3.hip:62-81)."""
    if p.xcd_map:
        m = (g >> 3) + k * (p.G >> 3)
        if m >= (p.B * p.H >> 3) * p.nkt:
            return None
        return (m // p.nkt) * 8 + (g & 7), m % p.nkt
    m = g + k * p.G
    if m >= p.B * p.H * p.nkt:
        return None
    return m // p.nkt, m % p.nkt


def walks(p):
    """{(batch-head, key block): (workgroup, position in its walk, length of its walk)}; every item exactly once."""
    out = {}
    for g in range(p.G):
        its = []
        while (it := item_of(p, g, len(its))) is not None:
            its.append(it)
        for k, it in enumerate(its):
            assert it not in out
            out[it] = (g, k, len(its))
    assert len(out) == p.items
    return out


def _classes(p, w, b):
    """Walk positions of image b's items: {(walk length, 'first' | 'middle' | 'last')}."""
    cl = set()
    for bh in range(b * p.H, (b + 1) * p.H):
        for kt in range(p.nkt):
            _, k, L = w[(bh, kt)]
            if k == 0:
                cl.add((L, "first"))
            if k == L - 1:
                cl.add((L, "last"))
            if 0 < k < L - 1:
                cl.add((L, "middle"))
    return cl


def pick_images(p, at_least=8):
    """The images compared one by one: all of them when that is cheap (N <= 600), else a cover of every position in a walk — first, middle
    and last item of a workgroup that walks walk_max items and of one that walks walk_min — plus, for the plain item map, an image whose items
    lie on two walk rounds (its first items are the k-th of the last workgroups, the rest the (k + 1)-th of the first ones), filled up to
    `at_least` with images spread evenly over the batch."""
    if p.N <= 600 or p.B <= at_least:
        return list(range(p.B))
    w = walks(p)
    per_image = [_classes(p, w, b) for b in range(p.B)]
    want = set().union(*per_image)
    chosen, have = [], set()
    for b in range(p.B):
        if per_image[b] - have:
            chosen.append(b)
            have |= per_image[b]
    assert have == want
    if not p.xcd_map:
        for b in range(p.B):
            ks = {w[(bh, kt)][1] for bh in range(b * p.H, (b + 1) * p.H) for kt in range(p.nkt)}
            if len(ks) > 1:
                if b not in chosen:
                    chosen.append(b)
                break
    for i in range(at_least):
        b = (i * p.B) // at_least + p.B // (2 * at_least)
        if len(chosen) < at_least and b not in chosen:
            chosen.append(b)
    for b in range(p.B):
        if len(chosen) < at_least and b not in chosen:
            chosen.append(b)
    return sorted(chosen)


# (B, N, H, Nq or None = all) -> what dkdv3_plan must say for a 256-CU device: in_loop, XCD item map, tail kind, (walk max, walk min).
# Chosen from the launch arithmetic; tests/test_attn_seams_cpu.py asserts that the table covers every regime.
Case = namedtuple("Case", "B N H Nq in_loop xcd tail walk")
CASES = [
    Case(48, 1569, 6, None, True, True, "tail2", (7, 6)),    # headline N, uneven walk
    Case(45, 1177, 6, None, True, False, "none", (6, 5)),    # plain map; partial item (153 keys: one idle wave, a 25-key wave) mid-walk
    Case(40, 981, 6, None, True, True, "none", (4, 3)),      # nt 16, kv_t0 4: stores and K / V rows overlap on R for four tiles; 21-key wave
    Case(44, 1040, 6, None, True, True, "tail2", (5, 4)),    # nt 17: odd nt at the overlap
    Case(48, 1024, 6, None, True, True, "none", (5, 4)),     # no remainder, nt 16
    Case(48, 960, 6, None, False, True, "none", (5, 4)),     # nt 15: the other side of the boundary; 192 keys: one idle wave
    Case(27, 1373, 6, None, True, False, "ranged", (4, 3)),  # ranged tail behind a multi-item walk
    Case(35, 785, 6, None, False, False, "tail2", (3, 2)),   # longest !in_loop model N
    Case(32, 589, 6, None, False, True, "ranged", (2, 1)),   # CHAMMI
    Case(24, 393, 6, None, False, True, "none", (2, 1)),     # 137 keys: one idle wave, a 9-key wave
    Case(48, 289, 6, None, False, True, "tail2", (2, 1)),    # so2sat; one key block per pair
    Case(64, 197, 6, None, False, True, "none", (2, 1)),     # N <= 256: a 5-key wave
    Case(90, 130, 3, None, False, False, "none", (2, 1)),    # three heads: one idle wave, a 2-key wave
    Case(64, 1569, 6, 1, False, True, "tail2", (9, 9)),      # the last block's call at the bench shape
    Case(43, 1569, 6, 1, False, False, "tail2", (7, 6)),     # the same with the plain map
    Case(40, 600, 6, 33, False, True, "ranged", (2, 1)),     # 1 < Nq < 64: a partial only tile
]
_IDS = [f"B{c.B}-N{c.N}-H{c.H}-Nq{c.Nq or 'all'}" for c in CASES]


def _close(a, b, rtol, atol, what=""):  # as in test_kernels_gpu.py, in float64
    a, b = a.double(), b.double()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max().item():.4g} (ref max {b.abs().max().item():.4g})"


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def _premise(case):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = dkdv3_plan(case.B, case.N, case.H, case.Nq, cus)
    print(f"\nplan at {cus} CUs: items {p.items} on {p.G} workgroups, walk {p.walk_max}/{p.walk_min}, nt {p.nt} "
          f"({'in_loop, kv_t0 %d' % p.kv_t0 if p.in_loop else '!in_loop'}), {'XCD' if p.xcd_map else 'plain'} map, rem {p.rem} -> tail {p.tail}, "
          f"last block {p.last_keys} keys ({p.idle_waves} idle waves, {p.part_keys}-key wave)")
    assert p.walk_max >= 2 and (p.in_loop, p.xcd_map, p.tail, (p.walk_max, p.walk_min)) == (case.in_loop, case.xcd, case.tail, case.walk), \
        f"this device has {cus} CUs (an MI355X has 256): the plan {p} does not walk the seams this case is in the table for"
    return p


def _run(hip, qs, dO, B, N, H, Nq):
    """The pre-scaled chain on NaN-filled outputs: o, lse, dqkv."""
    D = H * 64
    o = torch.full((B, N, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, H, N), float("nan"), device="cuda")
    dqkv = torch.full((B, N, 3 * D), float("nan"), dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(2, B, H, N, device="cuda")
    hip.attn_fwd(qs, o, lse, B, N, H, 64, 64 ** -0.5, nq=Nq, prescaled=True)
    hip.attn_bwd(qs, o, dO, lse, ws, dqkv, B, N, H, 64, 64 ** -0.5, nq=Nq, prescaled=True)
    torch.cuda.synchronize()
    return o, lse, dqkv


_last = {}


def _batched(hip, case, p):
    """Inputs and the batched run of a case (kept for the case's second test: one entry).  Every image has its own data (one generator over the
    whole tensor); every third compared image carries test_attention_prescaled_q's spike (one query x 4, one late key equal to it)."""
    if _last.get("case") != case:
        _last.clear()
        B, N, H = case.B, case.N, case.H
        D = H * 64
        nq = p.Nq
        c = 64 ** -0.5 * math.log2(math.e)
        g = torch.Generator(device="cpu").manual_seed(1000 * N + B)
        qkv = (torch.randn(B, N, 3 * D, generator=g) * 1.5).to(torch.bfloat16).cuda()
        images = pick_images(p)
        for b in images[::3]:
            qkv[b, N // 2, :64] *= 4
            qkv[b, N - 1, D:D + 64] = qkv[b, N // 2, :64]
        qs = qkv.clone()
        qs[:, :, :D] = (qkv[:, :, :D].float() * c).to(torch.bfloat16)
        del qkv
        dO = torch.full((B, N, D), float("nan"), dtype=torch.bfloat16, device="cuda")  # rows >= Nq are not the kernels' to read
        dO[:, :nq] = torch.randn(B, nq, D, generator=g).to(torch.bfloat16).cuda()
        _last.update(case=case, qs=qs, dO=dO, images=images, out=_run(hip, qs, dO, B, N, H, case.Nq))
    return _last["qs"], _last["dO"], _last["images"], _last["out"]


def _where(p, w, b, bad):
    """Names the first mismatching rows of dK / dV of image b as items: (head, key block) -> workgroup, walk position."""
    rows = bad.reshape(p.N, 3, p.H, 64).any(-1)  # [N, slot, H]
    msg = []
    for slot, nm in enumerate(["dQ", "dK", "dV"]):
        idx = rows[:, slot].nonzero()
        if len(idx) == 0:
            continue
        hit = sorted({(int(h), int(n) // K3_KEYS) for n, h in idx.tolist()})[:6]
        lo, hi = int(idx[:, 0].min()), int(idx[:, 0].max())
        s = f"{nm}: {len(idx)} (row, head) pairs, rows {lo}..{hi}"
        if slot:
            s += ", items " + ", ".join(
                f"(head {h}, block {kt}{'' if kt < p.nkt else ' = tail launch'})" + (" -> workgroup %d, item %d of %d" % w[(b * p.H + h, kt)] if kt < p.nkt else "")
                for h, kt in hit)
        msg.append(s)
    return "; ".join(msg)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_batch_slice_bit_identity(hip, case):
    """A: o, lse and dqkv (dQ, dK, dV; for Nq < N the zero dQ rows >= Nq too) of image b in the batched run are bit-identical to image b run alone,
    for images that cover every position in a walk (pick_images).  The forward and dQ kernels are per (batch, head, tile) with an XCD remap of
    blockIdx only (attn_common.hpp: attn_block_to_tile), so the identity is asserted through the public entries for the whole chain."""
    p = _premise(case)
    qs, dO, images, (o, lse, dqkv) = _batched(hip, case, p)
    N, H, nq = case.N, case.H, p.Nq
    assert len(images) >= min(8, case.B)
    print(f"images compared bit for bit: {images}")
    w = walks(p)
    for b in images:
        o1, lse1, d1 = _run(hip, qs[b:b + 1].contiguous(), dO[b:b + 1].contiguous(), 1, N, H, case.Nq)
        assert torch.equal(o[b, :nq].view(torch.int16), o1[0, :nq].view(torch.int16)), f"o of image {b} differs from the image run alone"
        assert torch.equal(lse[b, :, :nq], lse1[0, :, :nq]), f"lse of image {b} differs from the image run alone"
        bad = dqkv[b].view(torch.int16) != d1[0].view(torch.int16)
        assert not bad.any(), f"dqkv of image {b}: {int(bad.sum())} elements differ from the image run alone: {_where(p, w, b, bad)}"
        if nq < N:
            assert not dqkv[b, nq:, :H * 64].any(), f"dQ rows >= Nq of image {b} are not zero"
    assert bool(torch.isfinite(dqkv.float()).all()), "NaN pre-fill left in dqkv (or a non-finite gradient) in an image that was not compared"


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_batched_against_float64(hip, case):
    """B: the batched run's o, lse and dqkv against the materialised softmax in float64 from the operands the kernels saw, one image at a time,
    at test_attention_prescaled_q's bounds (O 2e-2 / 2e-2, LSE 1e-4 / 3e-3, dQ / dK / dV rtol 3e-2 and atol 3e-2 max|ref| of the image's slot)."""
    p = _premise(case)
    qs, dO, images, (o, lse, dqkv) = _batched(hip, case, p)
    N, H, nq = case.N, case.H, p.Nq
    D = H * 64
    scale = 64 ** -0.5
    c = scale * math.log2(math.e)
    worst = {"dK": 0.0, "dV": 0.0}
    for b in images:
        qr = qs[b].double()
        qr[:, :D] /= c  # what the kernels see, unscaled
        qr.requires_grad_(True)
        q, k, v = qr.reshape(N, 3, H, 64).permute(1, 2, 0, 3)
        s = (q[:, :nq] @ k.transpose(-1, -2)) * scale
        o_ref = (s.softmax(-1) @ v).transpose(0, 1).reshape(nq, D)
        lse_ref = torch.logsumexp(s, -1)
        (o_ref * dO[b, :nq].double()).sum().backward()
        _close(o[b, :nq], o_ref.detach(), 2e-2, 2e-2, f"O, image {b}")
        _close(lse[b, :, :nq], lse_ref.detach(), 1e-4, 3e-3, f"LSE, image {b}")
        g = qr.grad.reshape(N, 3, D)
        d = dqkv[b].double().reshape(N, 3, D)
        for i, nm in enumerate(["dQ", "dK", "dV"]):
            ref = g[:, i]
            _close(d[:, i], ref, 3e-2, 3e-2 * ref.abs().max().item(), f"{nm}, image {b}")
            if i:
                worst[nm] = max(worst[nm], ((d[:, i] - ref).norm() / ref.norm()).item())
        del qr, s, o_ref, lse_ref, g
    print(f"{len(images)} images against float64: worst relative L2 error dK {worst['dK']:.2e}, dV {worst['dV']:.2e}")
