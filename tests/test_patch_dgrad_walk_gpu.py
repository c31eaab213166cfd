"""dcv_patch_dgrad (csrc/patch_dgrad.hip) through hip.patch_dgrad at shapes where its waves walk several tiles — both register buffers, both exits of
the walk loop, on the first pass and after going round — and where the zero kernel walks planes and strides inside one, on operands for which the kernel's
fp32 arithmetic is exact: dx bit for bit against the float64 expectation, on NaN-prefilled memory between guards.  A tile multiplied with the other buffer's
fragments, stored under the other buffer's mask or dropped at an exit changes bits here; a mismatch is reported as workgroup, wave, position in the walk
and buffer.  The plans, the operands, the rule and the proof on the CPU that the rule flags such defects are in tests/test_patch_dgrad_walk_cpu.py.
Needs an MI355X: run with -m gpu."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_patch_dgrad_walk_cpu import (GUARD, WALK_CASES, WALK_IDS, ZERO_CASES, ZERO_IDS, check_dx, exits, expected_dx, lengths, operands,  # noqa: E402
                                       plan_of, walk_premises, zero_launched, zero_plan)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu_device):
    from diverse_channel_vit_amd import hip as h
    h.load()
    return h


def _run_and_check(hip, case, p):
    """One call on a NaN-prefilled dx between NaN guards against the exact expectation, then a second call that must give the same bits."""
    ops = operands(case)
    ops = ops._replace(dY=ops.dY.cuda(), W=ops.W.cuda(), ch_idx=ops.ch_idx.cuda(), scale=None if ops.scale is None else ops.scale.cuda())
    exp = expected_dx(case, ops)
    B, Ct, C, H, W = case.B, case.Ct, len(case.chans), case.H, case.W
    numel = B * Ct * H * W

    def call():
        buf = torch.full((GUARD + numel + GUARD,), float("nan"), device="cuda")
        hip.patch_dgrad(ops.dY, ops.W, ops.ch_idx, buf[GUARD:GUARD + numel].view(B, Ct, H, W), B, Ct, C, H, W, case.P, scale=ops.scale)
        torch.cuda.synchronize()
        return buf

    buf = call()
    found = check_dx(case, p, buf, exp)
    assert not found, "\n".join(found)
    del buf
    # the first result is the expectation bit for bit, so a second call that equals the expectation equals the first
    assert torch.equal(call()[GUARD:GUARD + numel].view(B, Ct, H, W), exp), "a second call gives other bits than the first"


@pytest.mark.parametrize("case", WALK_CASES, ids=WALK_IDS)
def test_waves_walk_tiles(hip, case):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = plan_of(case, cus)
    assert lengths(p) == case.lengths and exits(p) == (1, 2) and walk_premises(p) == [], \
        (f"this device has {cus} CUs (an MI355X has 256): walks of {lengths(p)} tiles, exits {exits(p)}, {walk_premises(p)} "
         f"({p.tiles} tiles, stride {p.stride}) are not what this case is in the table for (walks of {case.lengths})")
    _run_and_check(hip, case, p)


@pytest.mark.parametrize("case", ZERO_CASES, ids=ZERO_IDS)
def test_zero_kernel_walks_planes_and_strides(hip, case):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    z = zero_plan(case.B, case.Ct, case.H, case.W)
    assert zero_launched(case) and (z.walks_planes, z.e_strides) == ((True, False) if case is ZERO_CASES[0] else (False, True)), z
    p = plan_of(case, cus)
    assert lengths(p) == case.lengths, f"this device has {cus} CUs (an MI355X has 256): walks of {lengths(p)} tiles, the table says {case.lengths}"
    _run_and_check(hip, case, p)
