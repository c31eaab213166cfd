"""dcv_patch_dgrad (csrc/patch_dgrad.hip) where its waves walk several tiles and where the zero kernel walks planes and strides inside one: the launch
plan restated, operands on which the kernel's fp32 arithmetic is exact, the comparison rule of tests/test_patch_dgrad_walk_gpu.py, and the proof, without a
GPU, that the rule flags a pipeline defect.

The walk.  patch_dgrad_kernel gives wave w of workgroup g the tiles g*8 + w, + stride, + 2 stride, ... (stride = 8 G) and alternates two register buffers:
position 0, 2, 4, ... of a walk is multiplied out of f0 / ok0, position 1, 3, 5, ... out of f1 / ok1, and a wave leaves by the first exit (line 108) when
its walk is odd, by the second (line 112) when it is even.  pd_launch caps G at cus / S only when there are more than 8 (cus / S) tiles; below that every
wave has one tile, which is all that tests/test_input_grad_gpu.py reaches.

Exact operands.  With u = 2^-15 every dY value is an integer in [-7, 7] times 2^-3 and every W value an integer times 2^-12, all bf16 numbers:
  dims 0..5 of a token's dY row  the six base-15 digits of its row index, each minus 7; dim 6 is 1; the other dims are drawn from [-7, 7]
  column p of W                  2 and 30 at dims 2k, 2k + 1 for k = p % 3, zero at the other four digit dims, 1 at dim 6, 512 r with r drawn from [-5, 5] elsewhere
so that pixel p of a token is, in units of u, 2 (d_2k + 15 d_2k+1) + 1 + 512 R: an odd integer (never zero) whose residue mod 512 names two digits of the
row, and any three consecutive pixels name the row.  Every float4 the kernel stores therefore says which token it was computed from: two different tokens
never have equal outputs, whichever tiles a defect confuses.  Every product is an integer of at most 7 * 2560 units and a sum over D <= 768 of their
magnitudes stays below 768 * 7 * 2560 = 13.8e6 < 2^24, so every partial sum in any order is exact in fp32; the per-channel scale is a signed power of two
(distinct magnitudes, negative for even c: a single channel has a negative one) and multiplies exactly.  The expectation is the float64 result cast to fp32, compared with torch.equal.

Valid masks.  A tile's mask is min(16, wp - 16 jc) leading lanes: it depends on the chunk jc = t % chunks alone, so two tiles can differ in it only through
jc.  The strides at 256 CUs are powers of two; every walking case has an odd number of chunks >= 3 and wp % 16 != 0, so jc changes with every step of a walk
and full and partly valid tiles follow each other in both buffers (asserted from the plan: a wave exists whose f1 tile has MORE valid lanes than the ok0
in force while it is multiplied, so that a swapped mask leaves NaN behind).

emulate() is a plain transcription of lines 98-114 with float64 tile arithmetic and flat-address stores into a NaN-prefilled buffer between guards, with one
of five defects switched in.  It runs at a reduced CU count (REDUCED_CUS, 8 where the shape allows) on a smaller batch of the same case, chosen so that the
same walk lengths occur: the defect tests exercise the rule and the operands, not a plan at 256 CUs; the premises of the table at 256 CUs are asserted
separately.  Defect (d), a stale f0 for the third tile, needs a walk of three: on the cases that are in the table for walks of 1 and 2 it changes nothing and
is asserted to change nothing; every other defect is flagged on every walking case."""
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CUS = 256
PD_WAVES = 8
GUARD = 4096
UNIT_DY, UNIT_W = 2.0 ** -3, 2.0 ** -12
DY_MAX, W_RAND_MAX, W_RAND_STEP = 7, 5, 512
REDUCED_CUS = (8, 16, 32)

# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The cases.  lengths: the walk lengths dgrad_plan must show at 256 CUs (asserted below and, with the device's CU count, on the GPU).
Case = namedtuple("Case", "P D B Ct chans H W scale lengths")
WALK_CASES = [
    Case(8, 192, 509, 1, (0,), 16, 264, False, (1, 2)),                      # S = 1: a round is 2048 tiles; 3054 tiles
    Case(8, 192, 398, 4, (3, 0, 1), 19, 300, True, (3, 4)),                  # 7164 tiles; channel subset, border 3 x 4, wp = 37
    Case(8, 384, 340, 3, (2, 0, 1), 12, 328, True, (1, 2)),                  # 3060 tiles; one patch row per plane (hp = 1), wp = 41
    Case(8, 384, 597, 2, (1, 0), 16, 376, False, (3, 4)),                    # 7164 tiles; wp = 47
    Case(8, 768, 102, 5, (4, 1), 24, 536, True, (1, 2)),                     # 3060 tiles; hp = 3, five chunks (wp = 67)
    Case(8, 768, 1031, 1, (0,), 16, 264, True, (3, 4)),                      # 6186 tiles
    Case(16, 192, 509, 1, (0,), 35, 532, True, (1, 2)),                      # 3054 tiles; border 3 x 4
    Case(16, 192, 1031, 1, (0,), 32, 528, False, (3, 4)),                    # 6186 tiles
    Case(16, 384, 85, 4, (2, 3, 0), 32, 592, True, (1, 2)),                  # S = 2: a round is 1024 tiles; 1530 tiles; wp = 37
    Case(16, 384, 199, 3, (1, 2, 0), 37, 536, True, (3, 4)),                 # 3582 tiles; border 5 x 8
    Case(16, 768, 255, 2, (1,), 20, 656, True, (1, 2)),                      # S = 4: a round is 512 tiles; 765 tiles; hp = 1, wp = 41
    Case(16, 768, 299, 1, (0,), 32, 528, False, (3, 4)),                     # 1794 tiles
    Case(16, 768, 67, 8, (6, 2, 7, 0, 3, 5, 1), 32, 528, True, (5, 6)),      # 2814 tiles: five and a half rounds
]
# the zero kernel: more planes than its grid has rows (B Ct = 20500 > 16384); more float4 per plane than its 64 columns of 256 threads cover (17956 > 16384)
ZERO_CASES = [
    Case(8, 192, 4100, 5, (3, 0), 8, 8, True, (4, 5)),
    Case(8, 384, 1, 2, (1,), 268, 268, True, (0, 1)),
]


def case_id(c):
    return f"P{c.P}-D{c.D}-B{c.B}-C{len(c.chans)}of{c.Ct}-{c.H}x{c.W}"


WALK_IDS = [case_id(c) for c in WALK_CASES]
ZERO_IDS = [case_id(c) for c in ZERO_CASES]

# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The plans.
Plan = namedtuple("Plan", "P D B C H W cus Q S hp wp chunks tiles G stride walks")
Where = namedtuple("Where", "t b c i jc valid g wave pos length slot exit")


def dgrad_plan(P, D, B, C, H, W, cus):
    """pd_launch (patch_dgrad.hip:135-146), the instance table (patch_dgrad.hip:160-167) and the kernel's dealing (patch_dgrad.hip:86-88, 97-114)
    restated.  Q pixel columns per workgroup, S = P P / Q slices (every slice walks the same tiles), tiles of 16 tokens of one patch row
    (patch_dgrad.hip:139-140), G workgroups per slice capped at cus / S (patch_dgrad.hip:141-143), stride = 8 G (patch_dgrad.hip:97).
    walks[(g, wave)] is the wave's tile list g*8 + wave, + stride, ... (patch_dgrad.hip:98, 105, 109, 113); every tile is dealt exactly once."""
    Q = {(16, 192): 256, (16, 384): 128}.get((P, D), 64)
    S = P * P // Q
    hp, wp = H // P, W // P
    chunks = (wp + 15) // 16
    tiles = B * C * hp * chunks
    G = min(-(-tiles // PD_WAVES), max(cus // S, 1))
    stride = G * PD_WAVES
    walks = {(g, w): list(range(g * PD_WAVES + w, tiles, stride)) for g in range(G) for w in range(PD_WAVES)}
    dealt = sorted(t for ts in walks.values() for t in ts)
    assert dealt == list(range(tiles)), "a tile is dealt twice or not at all"
    return Plan(P, D, B, C, H, W, cus, Q, S, hp, wp, chunks, tiles, G, stride, walks)


def plan_of(case, cus, B=None):
    return dgrad_plan(case.P, case.D, case.B if B is None else B, len(case.chans), case.H, case.W, cus)


def valid_lanes(p, t):
    """lanes of tile t that hold a token: j = 16 jc + (lane & 15) < wp (patch_dgrad.hip:24-27)"""
    return min(16, p.wp - 16 * (t % p.chunks))


def where(p, t):
    """Tile t in plan terms: (b, c, i, jc) as pd_tile decodes it (patch_dgrad.hip:58-63), its valid lanes, and the wave that has it: workgroup, wave,
    position in the walk, walk length, buffer (0: f0 / ok0, 1: f1 / ok1) and the exit the wave leaves by (0: line 99 with no tile, 1: line 108, 2: line 112)."""
    r, jc = divmod(t, p.chunks)
    bc, i = divmod(r, p.hp)
    b, c = divmod(bc, p.C)
    pos, t0 = divmod(t, p.stride)
    g, wave = divmod(t0, PD_WAVES)
    L = len(p.walks[(g, wave)])
    return Where(t, b, c, i, jc, valid_lanes(p, t), g, wave, pos, L, pos & 1, 2 - (L & 1))


def wave_exit(L):
    return 0 if L == 0 else 2 - (L & 1)


def lengths(p):
    return tuple(sorted({len(ts) for ts in p.walks.values()}))


def exits(p):
    return tuple(sorted({wave_exit(len(ts)) for ts in p.walks.values()}))


def slot_valids(p):
    """{(buffer, valid lanes)} over all tiles"""
    return {(k & 1, valid_lanes(p, t)) for ts in p.walks.values() for k, t in enumerate(ts)}


def stale_mask_shows(p):
    """a wave has an f1 tile with more valid lanes than the ok0 in force when it is multiplied: ok0 is the mask of the tile after it when the walk has one
    (reloaded at line 110), of the tile before it otherwise.  With ok0 in place of ok1 those lanes are not stored: NaN stays behind."""
    for ts in p.walks.values():
        for k in range(1, len(ts), 2):
            if valid_lanes(p, ts[k]) > valid_lanes(p, ts[k + 1] if k + 1 < len(ts) else ts[k - 1]):
                return True
    return False


def walk_premises(p):
    """what every walking case needs for each injected defect to be observable; returns the list of what is missing"""
    miss = []
    if p.tiles <= p.stride:
        miss.append("no wave has a second tile")
    if not (p.wp % 16 and p.chunks >= 2):
        miss.append("no partly valid tiles next to full ones")
    partial = {s for s, v in slot_valids(p) if v < 16}
    full = {s for s, v in slot_valids(p) if v == 16}
    if partial != {0, 1} or full != {0, 1}:
        miss.append("full and partly valid tiles do not both land in f0 and in f1")
    if not stale_mask_shows(p):
        miss.append("ok0 never has fewer lanes than the ok1 it would replace")
    if p.hp == p.chunks:
        miss.append("hp == chunks hides a row index computed with the wrong one")
    if not any(len(ts) % 2 == 0 and ts for ts in p.walks.values()):
        miss.append("no wave leaves by the second exit")
    return miss


ZeroPlan = namedtuple("ZeroPlan", "gx gy planes per walks_planes e_strides")


def zero_plan(B, Ct, H, W):
    """the zero kernel's launch (patch_dgrad.hip:172-176) and its two loops (patch_dgrad.hip:122, 128): gy rows walk the planes when there are more
    than 16384, gx <= 64 columns of 256 threads stride over the H (W / 4) float4 of a plane when there are more than 64 * 256"""
    planes, per = B * Ct, H * (W // 4)
    gx = min(-(-per // 256), 64)
    gy = min(planes, 16384)
    return ZeroPlan(gx, gy, planes, per, planes > gy, per > gx * 256)


def zero_launched(case):
    """patch_dgrad.hip:170-171"""
    return len(case.chans) < case.Ct or case.H % case.P != 0 or case.W % case.P != 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Operands and expectation.
Operands = namedtuple("Operands", "dY W ch_idx scale")


def channel_scale(C):
    """signed powers of two, a different magnitude for every channel, negative for even c"""
    assert C <= 8
    return torch.tensor([(-1.0) ** (c + 1) * 2.0 ** ((3 * c) % 8 - 3) for c in range(C)], dtype=torch.float32)


def operands(case, B=None):
    """dY [B C n, D] and W [D, P P] in bf16, ch_idx int32 [C], scale fp32 [C] or None (see the module docstring); the first rows of a larger batch of the
    same case are the rows of a smaller one"""
    B = case.B if B is None else B
    P, D, C = case.P, case.D, len(case.chans)
    M = B * C * (case.H // P) * (case.W // P)
    assert M < 15 ** 6 and D * DY_MAX * W_RAND_MAX * W_RAND_STEP < 2 ** 24
    g = torch.Generator().manual_seed(1000 * P + D + 7 * case.H + case.W)
    W = torch.randint(-W_RAND_MAX, W_RAND_MAX + 1, (D, P * P), generator=g) * W_RAND_STEP
    pix = torch.arange(P * P)
    W[:6] = 0
    W[2 * (pix % 3), pix] = 2
    W[2 * (pix % 3) + 1, pix] = 30
    W[6] = 1
    dY = torch.randint(-DY_MAX, DY_MAX + 1, (M, D), generator=g, dtype=torch.int16)
    rows = torch.arange(M)
    for k in range(6):
        dY[:, k] = (rows // 15 ** k % 15 - 7).to(torch.int16)
    dY[:, 6] = 1
    dYb, Wb = dY.to(torch.bfloat16) * UNIT_DY, (W.float() * UNIT_W).to(torch.bfloat16)  # small integers times a power of two: exact
    assert torch.equal(Wb.float(), W.float() * UNIT_W)
    return Operands(dYb, Wb, torch.tensor(case.chans, dtype=torch.int32), channel_scale(C) if case.scale else None)


def expected_dx(case, ops, B=None, chunk_rows=2048):
    """dx [B, Ct, H, W]: the float64 product, scale and col2im cast to fp32, on the device the operands are on (about chunk_rows tokens at a time).  Asserts
    that the cast changes nothing: the expectation is exact."""
    B = case.B if B is None else B
    P, C, H, Wd = case.P, len(case.chans), case.H, case.W
    hp, wp = H // P, Wd // P
    n = hp * wp
    dev = ops.dY.device
    sc = (ops.scale if ops.scale is not None else torch.ones(C, device=dev)).double().view(1, C, 1, 1)
    W64, ch = ops.W.double(), ops.ch_idx.long()
    out = torch.zeros(B, case.Ct, H, Wd, dtype=torch.float32, device=dev)
    batch_chunk = max(1, chunk_rows // (C * n))
    for b0 in range(0, B, batch_chunk):
        b1 = min(B, b0 + batch_chunk)
        G = ops.dY[b0 * C * n:b1 * C * n].double() @ W64
        G = G.view(b1 - b0, C, hp, wp, P, P).permute(0, 1, 2, 4, 3, 5).reshape(b1 - b0, C, hp * P, wp * P) * sc
        G32 = G.float()
        assert torch.equal(G32.double(), G), "the expectation is not exact in fp32"
        out[b0:b1, ch, :hp * P, :wp * P] = G32
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The comparison rule.
def check_dx(case, p, buf, expected, guard=GUARD, limit=6):
    """buf: the flat fp32 buffer the kernel wrote into, NaN-prefilled, dx between two guard regions of `guard` floats.  Returns the list of findings
    (empty: pass): guards intact, every element written, channels outside ch_idx and the dropped border exactly zero, dx bit-equal to the expectation;
    on a mismatch the first wrong tiles in plan terms."""
    B, Ct, H, W, P, C = p.B, case.Ct, p.H, p.W, p.P, p.C
    numel = B * Ct * H * W
    assert buf.numel() == numel + 2 * guard and tuple(expected.shape) == (B, Ct, H, W)
    out = []
    if not (bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + numel:]).all())):
        out.append("guard region overwritten")
    dx = buf[guard:guard + numel].view(B, Ct, H, W)
    unwritten = int(torch.isnan(dx).sum())
    if unwritten:
        out.append(f"{unwritten} elements not written")
    unused = [c for c in range(Ct) if c not in case.chans]
    if unused and bool((dx[:, unused] != 0).any()):
        out.append("channels outside ch_idx are not exactly 0")
    Hh, Ww = p.hp * P, p.wp * P
    if bool((dx[:, :, Hh:] != 0).any()) or bool((dx[:, :, :, Ww:] != 0).any()):
        out.append("the border the conv drops is not exactly 0")
    if torch.equal(dx, expected):
        return out
    bad = dx != expected  # NaN included
    inner = bad[:, list(case.chans), :Hh, :Ww].reshape(B, C, p.hp, P, p.wp, P).any(5).any(3)  # [B, C, hp, wp]: wrong tokens
    pad = torch.zeros(B, C, p.hp, p.chunks * 16, dtype=torch.bool, device=bad.device)
    pad[..., :p.wp] = inner
    tiles_bad = pad.view(B, C, p.hp, p.chunks, 16).any(-1).flatten().nonzero().flatten()  # t = ((b C + c) hp + i) chunks + jc
    outside = int(bad.sum()) - int(bad[:, list(case.chans), :Hh, :Ww].sum())
    lines = [f"{int(bad.sum())} elements differ from the exact expectation: {len(tiles_bad)} of {p.tiles} tiles"
             + (f", {outside} elements outside the GEMM's reach" if outside else "")
             + f" (G {p.G} workgroups x {p.S} slices, stride {p.stride})"]
    for t in tiles_bad[:limit].tolist():
        w = where(p, t)
        lines.append(f"  tile {t} (b {w.b}, c {w.c}, patch row {w.i}, chunk {w.jc}, {w.valid} valid lanes): workgroup {w.g}, wave {w.wave}, "
                     f"position {w.pos} of a walk of {w.length}, buffer f{w.slot}, the wave leaves by exit {w.exit}")
    out.append("\n".join(lines))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The emulation.
DEFECTS = {
    "a": "pd_tile of the f1 slot multiplies f0's fragments",
    "b": "the f1 slot stores under ok0",
    "c": "the last tile of a wave that leaves by the second exit is skipped",
    "d": "f0 is not reloaded: the third tile reuses the first tile's fragments",
    "e": "pd_load's row index divides by chunks where it needs hp",
}


def emulate(case, p, ops, defect=None, guard=GUARD):
    """patch_dgrad_kernel (lines 86-114, pd_load lines 24-32, pd_tile lines 58-72) and what patch_dgrad_zero_kernel writes, on a NaN-prefilled flat
    buffer with guards, tile arithmetic in float64, stores by flat address in the order workgroup, wave, walk.  Returns the buffer (fp32 tensor)."""
    P, D, Q, S, C, Ct, H, W = p.P, p.D, p.Q, p.S, p.C, case.Ct, p.H, p.W
    hp, wp, chunks, tiles, stride = p.hp, p.wp, p.chunks, p.tiles, p.stride
    n = hp * wp
    numel = p.B * Ct * H * W
    buf = np.full(guard + numel + guard, np.nan, dtype=np.float32)
    dY = ops.dY.double().numpy()
    dY = np.concatenate([dY, np.zeros((chunks * wp + n + 16, D))])  # rows a wrong index may reach: zeros
    Wd = ops.W.double().numpy()
    ch = ops.ch_idx.tolist()
    scale = ops.scale.double().numpy() if ops.scale is not None else None
    lanes = np.arange(16)

    # the zero kernel (lines 120-131): whole planes of unused channels, rows >= Hh and columns >= Ww of the others
    if zero_launched(case):
        dx = buf[guard:guard + numel].reshape(p.B, Ct, H, W)
        for ct in range(Ct):
            if ct not in ch:
                dx[:, ct] = 0
        dx[:, :, hp * P:] = 0
        dx[:, :, :, wp * P:] = 0

    def load(t):
        jc, r = t % chunks, t // chunks
        j = jc * 16 + lanes
        valid = j < wp
        div = chunks if defect == "e" else hp  # line 29: n / wp = hp
        row = np.minimum((r // div) * n + (r % div) * wp + j, len(dY) - 1)
        return np.where(valid[:, None], dY[row], 0.0), valid

    def tile(f, ok, t, q0):
        acc = f @ Wd[:, q0:q0 + Q]  # [16 tokens, Q pixels]
        r, jc = divmod(t, chunks)
        bc, i = divmod(r, hp)
        b, c = divmod(bc, C)
        if scale is not None:
            acc = acc * scale[c]
        pp = q0 + np.arange(Q)
        u, v = pp // P, pp % P
        j = jc * 16 + lanes
        addr = guard + (b * Ct + ch[c]) * H * W + (i * P + u)[None, :] * W + j[:, None] * P + v[None, :]
        buf[addr[ok]] = acc[ok]

    for s in range(S):
        q0 = s * Q
        for g in range(p.G):
            for wave in range(PD_WAVES):
                t = g * PD_WAVES + wave
                if t >= tiles:
                    continue
                f0, ok0 = load(t)
                f1, ok1 = None, None
                while True:
                    t1 = t + stride
                    if t1 < tiles:
                        f1, ok1 = load(t1)
                    tile(f0, ok0, t, q0)
                    if t1 >= tiles:
                        break
                    t2 = t1 + stride
                    if t2 < tiles:
                        nf0, ok0 = load(t2)
                        if defect != "d":
                            f0 = nf0
                    if defect == "c" and t2 >= tiles:
                        break
                    tile(f0 if defect == "a" else f1, ok0 if defect == "b" else ok1, t1, q0)
                    if t2 >= tiles:
                        break
                    t = t2
    return torch.from_numpy(buf)


_reduced = {}


def reduced(case):
    """(B, cus): the smallest batch of the case, at the smallest of REDUCED_CUS, whose plan has the walk lengths the case shows at 256 CUs and every
    premise of a walking case"""
    if case not in _reduced:
        for cus in REDUCED_CUS:
            for B in range(1, 65):
                p = plan_of(case, cus, B)
                if lengths(p) == case.lengths and not walk_premises(p):
                    _reduced[case] = (B, cus)
                    return B, cus
        raise AssertionError(f"{case}: no reduced plan with walk lengths {case.lengths}")
    return _reduced[case]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WALK_CASES, ids=WALK_IDS)
def test_the_case_walks_as_listed_at_256_cus(case):
    p = plan_of(case, CUS)
    assert lengths(p) == case.lengths and exits(p) == (1, 2)
    assert walk_premises(p) == []
    assert p.stride == PD_WAVES * (CUS // p.S) and p.tiles > p.stride
    # partly valid tiles (1..15 lanes) in both buffers
    assert {s for s, v in slot_valids(p) if 1 <= v <= 15} == {0, 1}
    # device memory: dY, dx, the expectation and a second dx, plus one float64 chunk of the reference
    M, C = case.B * len(case.chans) * p.hp * p.wp, len(case.chans)
    dx_bytes = 4 * case.B * case.Ct * case.H * case.W
    chunk = max(2048, C * p.hp * p.wp) * (8 * case.D + 3 * 8 * case.P * case.P)
    assert 2 * M * case.D + 2 * dx_bytes + chunk < 200e6


def test_the_table_covers_the_walk():
    plans = {c: plan_of(c, CUS) for c in WALK_CASES}
    for P in (8, 16):
        for D in (192, 384, 768):
            got = set()
            for c in WALK_CASES:
                if (c.P, c.D) == (P, D):
                    got |= set(lengths(plans[c]))
            assert {1, 2, 3, 4} <= got, (P, D, got)
    assert any({5, 6} <= set(lengths(p)) for p in plans.values())
    assert {p.S for p in plans.values()} == {1, 2, 4} and {p.Q for p in plans.values()} == {64, 128, 256}
    for P in (8, 16):
        assert any(c.P == P and p.wp % 16 and p.chunks >= 2 and {s for s, v in slot_valids(p) if 1 <= v <= 15} == {0, 1} for c, p in plans.items())
    assert any(len(c.chans) < c.Ct and list(c.chans) != sorted(c.chans) for c in WALK_CASES)
    assert any(c.H % c.P and c.W % c.P for c in WALK_CASES)
    assert all(p.tiles % p.stride for p in plans.values())  # no whole number of rounds: two walk lengths in every launch
    assert {p.hp for p in plans.values()} >= {1, 2, 3} and {p.chunks for p in plans.values()} >= {3, 5}
    # the cases on which a stale f0 (defect d) cannot show are the ones listed for walks of 1 and 2, one per instance
    assert sorted((c.P, c.D) for c in WALK_CASES if max(c.lengths) < 3) == sorted((P, D) for P in (8, 16) for D in (192, 384, 768))


def test_where_agrees_with_the_walks():
    for case in (WALK_CASES[1], WALK_CASES[12]):
        p = plan_of(case, CUS)
        for (g, wave), ts in list(p.walks.items())[::37]:
            for k, t in enumerate(ts):
                w = where(p, t)
                assert (w.g, w.wave, w.pos, w.length, w.slot, w.exit) == (g, wave, k, len(ts), k & 1, wave_exit(len(ts)))
                assert t == ((w.b * p.C + w.c) * p.hp + w.i) * p.chunks + w.jc and 1 <= w.valid <= 16


def test_one_tile_per_wave_below_the_cap():
    """the shapes of tests/test_input_grad_gpu.py: every wave has at most one tile"""
    for P, D, B, C, H, W in ((16, 384, 2, 8, 224, 224), (8, 192, 3, 3, 36, 44), (16, 192, 2, 1, 48, 272), (8, 384, 1, 4, 136, 168)):
        assert lengths(dgrad_plan(P, D, B, C, H, W, CUS)) in ((1,), (0, 1))


@pytest.mark.parametrize("case", ZERO_CASES, ids=ZERO_IDS)
def test_zero_cases_walk_as_listed(case):
    z = zero_plan(case.B, case.Ct, case.H, case.W)
    assert zero_launched(case) and len(case.chans) < case.Ct
    if case is ZERO_CASES[0]:
        assert z.planes > 16384 and z.gy == 16384 and z.walks_planes and not z.e_strides
    else:
        assert z.per > 16384 and z.gx == 64 and z.e_strides and not z.walks_planes and case.H % case.P and case.W % case.P
    assert lengths(plan_of(case, CUS)) == case.lengths
    assert 4 * case.B * case.Ct * case.H * case.W < 10e6


@pytest.mark.parametrize("case", WALK_CASES, ids=WALK_IDS)
def test_operands_are_exact_and_name_their_token(case):
    B, cus = reduced(case)
    p = plan_of(case, cus, B)
    ops = operands(case, B)
    big = operands(case, min(case.B, B + 3))
    assert torch.equal(big.dY[:len(ops.dY)], ops.dY) and torch.equal(big.W, ops.W)  # a smaller batch is a prefix of the larger one
    # integers in units of 2^-3 and 2^-12 within the documented ranges; magnitudes sum below 2^24 units
    dY, W = ops.dY.double() / UNIT_DY, ops.W.double() / UNIT_W
    assert torch.equal(dY, dY.round()) and torch.equal(W, W.round()) and float(dY.abs().max()) <= DY_MAX
    assert float(W[7:].abs().max()) <= W_RAND_MAX * W_RAND_STEP and bool((W[7:] % W_RAND_STEP == 0).all()) and float(W[:7].abs().max()) <= 30
    mag = dY.abs() @ W.abs()
    assert float(mag.max()) < 2 ** 24
    if ops.scale is not None:
        m, e = torch.frexp(ops.scale)
        assert bool((m.abs() == 0.5).all()) and bool((ops.scale < 0).any()) and len(ops.scale.abs().unique()) == len(ops.scale)
    exp = expected_dx(case, ops, B)
    # every pixel of every token is an odd number of units: never zero; its residue names the token's row
    out = dY @ W  # [M, PP] in units
    assert bool((out % 2 == 1).all())
    k = torch.arange(case.P * case.P) % 3
    digits = ((out - 1) % W_RAND_STEP).long()
    digits = torch.where(digits >= W_RAND_STEP // 2, digits - W_RAND_STEP, digits) // 2  # d_2k + 15 d_2k+1 in [-112, 112]
    rows = torch.arange(len(out))
    want = torch.stack([(rows // 15 ** (2 * kk) % 15 - 7) + 15 * (rows // 15 ** (2 * kk + 1) % 15 - 7) for kk in range(3)], 1)
    assert torch.equal(digits, want[:, k])
    # so the tiles a defect could confuse have different outputs: t, t + stride, t + 2 stride and the next chunk of the patch row
    Hh, Ww = p.hp * case.P, p.wp * case.P
    tok = exp[:, list(case.chans), :Hh, :Ww].reshape(B, p.C, p.hp, case.P, p.wp, case.P).permute(0, 1, 2, 4, 3, 5).reshape(-1, case.P * case.P)
    assert len(tok.unique(dim=0)) == len(tok)
    assert bool((exp[:, list(case.chans), :Hh, :Ww] != 0).all())


@pytest.mark.parametrize("case", WALK_CASES + ZERO_CASES[1:], ids=WALK_IDS + ZERO_IDS[1:])
def test_the_emulated_walk_is_the_expectation(case):
    B, cus = reduced(case) if case in WALK_CASES else (case.B, 8)
    p = plan_of(case, cus, B)
    ops = operands(case, B)
    assert check_dx(case, p, emulate(case, p, ops), expected_dx(case, ops, B)) == []


@pytest.mark.parametrize("case", WALK_CASES, ids=WALK_IDS)
def test_every_injected_defect_is_flagged(case):
    B, cus = reduced(case)
    p = plan_of(case, cus, B)
    ops = operands(case, B)
    exp = expected_dx(case, ops, B)
    for d, what in DEFECTS.items():
        found = check_dx(case, p, emulate(case, p, ops, d), exp)
        if d == "d" and max(case.lengths) < 3:
            assert found == [], "no wave has a third tile, yet a stale f0 shows"
            continue
        assert found, f"defect ({d}) passes the comparison: {what}"
        text = "\n".join(found)
        assert "buffer f" in text or "not written" in text, text
        if d == "a":  # the report names the pipeline stage: every wrong tile sits in the f1 buffer
            assert "buffer f1" in text and "buffer f0" not in text, text
        if d == "b":  # lanes of an f1 tile that the narrower ok0 masks keep their NaN
            assert "not written" in text, text
        if d == "d":
            assert "buffer f0" in text and "buffer f1" not in text and "position 0" not in text, text
        if d == "c":
            assert "not written" in text and "buffer f1" in text and "buffer f0" not in text, text
