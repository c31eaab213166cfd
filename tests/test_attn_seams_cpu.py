"""The case table of tests/test_attn_seams_gpu.py against the launch plan of the persistent dK / dV kernel (dkdv3_plan restates
dcv_dkdv3_launch and the kernel's item dealing, csrc/attn_bwd3.hip), for the 256 CUs of an MI355X: every regime in which a workgroup crosses
a seam between two items is in the table, and no shape of the older kernel-level test crosses one.  Runs without a GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_attn_seams_gpu import CASES, dkdv3_plan, item_of, pick_images, walks  # noqa: E402

CUS = 256
PLANS = [(c, dkdv3_plan(c.B, c.N, c.H, c.Nq, CUS)) for c in CASES]


def test_plan_restates_the_launch_arithmetic():
    """Hand-checked values for three shapes (attn_bwd3.hip:497-510 and 53-81)."""
    p = dkdv3_plan(48, 1569, 6, None, 256)  # 33 remainder keys leave through TAIL2; 288 pairs x 6 blocks; per XCD 216 items on 32 workgroups
    assert (p.rem, p.split, p.key_hi, p.nkt, p.items, p.G, p.nt, p.in_loop, p.kv_t0, p.xcd_map) == (33, True, 1536, 6, 1728, 256, 25, True, 12, True)
    assert (p.walk_max, p.walk_min, p.tail, p.last_keys, p.idle_waves, p.part_keys) == (7, 6, "tail2", 256, 0, 0)
    p = dkdv3_plan(45, 1177, 6, None, 256)  # 270 pairs: not a multiple of 8; rem 153 > 128 stays in the persistent kernel: 64 + 64 + 25 keys
    assert (p.split, p.key_hi, p.nkt, p.items, p.xcd_map, p.walk_max, p.walk_min) == (False, 1177, 5, 1350, False, 6, 5)
    assert (p.nt, p.kv_t0, p.tail, p.last_keys, p.idle_waves, p.part_keys) == (19, 6, "none", 153, 1, 25)
    p = dkdv3_plan(40, 600, 6, 33, 256)  # rem 88 -> the ranged second-form launch from key 512
    assert (p.key_hi, p.nkt, p.items, p.nt, p.in_loop, p.tail, p.walk_max, p.walk_min) == (512, 2, 480, 1, False, "ranged", 2, 1)
    p = dkdv3_plan(1, 1569, 6, None, 256)  # fewer items than CUs: one each, the plain map (G = 36 is not a multiple of 8)
    assert (p.items, p.G, p.xcd_map, p.walk_max) == (36, 36, False, 1)


@pytest.mark.parametrize("case,p", PLANS, ids=[f"B{c.B}-N{c.N}-H{c.H}-Nq{c.Nq or 'all'}" for c in CASES])
def test_every_case_walks_seams_as_the_table_says(case, p):
    assert p.walk_max >= 2
    assert (p.in_loop, p.xcd_map, p.tail, (p.walk_max, p.walk_min)) == (case.in_loop, case.xcd, case.tail, case.walk)
    w = walks(p)  # the dealing covers every item once, and the walk lengths are the plan's
    lengths = {L for _, _, L in w.values()}
    assert max(lengths) == p.walk_max and min(lengths) == p.walk_min
    assert item_of(p, 0, p.walk_max) is None
    # qkv at most 231 MB
    assert case.B * case.N * 3 * case.H * 64 * 2 <= 232e6


def test_the_table_covers_every_regime():
    """Fails when a regime's row is removed from CASES.  All rows are multi-item rows (previous test)."""
    plans = [p for _, p in PLANS]
    assert {p.in_loop for p in plans} == {True, False}
    assert {p.xcd_map for p in plans} == {True, False}
    assert {p.tail for p in plans} == {"none", "tail2", "ranged"}
    assert any(p.rem == 0 for p in plans)
    assert {15, 16, 17} <= {p.nt for p in plans}
    assert any(p.Nq == 1 for p in plans)
    assert any(p.idle_waves > 0 for p in plans) and any(p.part_keys > 0 for p in plans)
    # ... and the combinations the seam code distinguishes
    assert any(p.in_loop and p.kv_t0 == 4 and p.nt == 16 for p in plans) and any(p.in_loop and p.kv_t0 == 4 and p.nt == 17 for p in plans)  # stores and K / V DMA overlap on R
    assert any(p.in_loop and p.kv_t0 >= 8 for p in plans)  # ... and do not
    for in_loop in (True, False):
        assert {p.xcd_map for p in plans if p.in_loop == in_loop} == {True, False}
        assert {p.tail for p in plans if p.in_loop == in_loop} == {"none", "tail2", "ranged"}
        assert any(p.part_keys > 0 for p in plans if p.in_loop == in_loop)
        assert any(p.idle_waves > 0 for p in plans if p.in_loop == in_loop)
    assert any(p.Nq == 1 and p.xcd_map for p in plans) and any(p.Nq == 1 and not p.xcd_map for p in plans)
    assert any(1 < p.Nq < 64 for p in plans)
    assert any(p.N <= 256 for p in plans)  # one key block per pair without a split
    assert any(p.walk_max >= 3 and not p.in_loop for p in plans)  # a middle item in the !in_loop regime


def test_compared_images_cover_every_walk_position():
    for case, p in PLANS:
        images = pick_images(p)
        assert len(images) == len(set(images)) and all(0 <= b < case.B for b in images)
        assert len(images) >= 8
        if case.N <= 600:
            assert images == list(range(case.B))
        w = walks(p)
        have, want = set(), set()
        for (bh, _), (_, k, L) in w.items():
            cl = {(L, "first")} if k == 0 else set()
            if k == L - 1:
                cl.add((L, "last"))
            if 0 < k < L - 1:
                cl.add((L, "middle"))
            want |= cl
            if bh // case.H in images:
                have |= cl
        assert have == want
        for L in {p.walk_max, p.walk_min}:
            assert (L, "first") in have and (L, "last") in have and (L < 3 or (L, "middle") in have)
        if not p.xcd_map:  # an image whose items lie on two rounds of the walk
            assert any(len({w[(bh, kt)][1] for bh in range(b * case.H, (b + 1) * case.H) for kt in range(p.nkt)}) > 1 for b in images)


def test_the_older_kernel_level_shapes_walk_one_item():
    """The gap the seam tests close: every shape of test_attention_prescaled_q gives each workgroup exactly one item on 256 CUs."""
    import test_kernels_gpu
    marks = [m for m in test_kernels_gpu.test_attention_prescaled_q.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "B,N,H,Nq,shift"
    shapes = marks[0].args[1]
    assert len(shapes) >= 8
    for B, N, H, Nq, _ in shapes:
        assert dkdv3_plan(B, N, H, Nq, CUS).walk_max == 1, (B, N, H, Nq)
