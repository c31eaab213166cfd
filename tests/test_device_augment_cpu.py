"""Host side of the device augmentation (diverse_channel_vit_amd/augment.py) and the restatements the GPU tests compare against:
tests/augment_ref.py against the fixture recorded from the real reference (tests/golden/tps_warp.npz) and against torch's CPU interpolate,
tps_coefficients against numpy's pinv, the invariants of DeviceAugment.sample, and the refusals — all raised before anything needs a GPU."""
import math

import numpy as np
import pytest
import torch

import augment_ref as R
from conftest import load_golden


def test_restatement_matches_the_reference_fixture():
    """1e-4 on 0..255 data: the reference's float32 output rounding (2^-17 at 255) and nothing else."""
    meta, z = load_golden("tps_warp")
    assert [c["name"] for c in meta["cases"]] == ["w31", "w64", "w160", "w224", "zero", "far"]
    for c in meta["cases"]:
        n = c["name"]
        got = R.tps_warp_ref(z[n + "_img"], z[n + "_dst"], z[n + "_src"])
        err = np.abs(got - z[n + "_out"]).max()
        print(n, "max |restatement - reference| =", err)
        assert err <= 1e-4, (n, err)


def test_fixture_covers_the_quirks():
    """The zero-displacement case is a zoom, not the identity, and the far case folds more than once."""
    meta, z = load_golden("tps_warp")
    img = z["zero_img"].astype(np.float64)
    assert np.abs(z["zero_dst"] - z["zero_src"]).max() == 0 and np.abs(z["zero_out"] - img).max() > 50
    P, coef = R.tps_coefficients_ref(z["zero_dst"], z["zero_src"], 64)
    co = R.tps_coords(P, coef, 64)
    zoom = (6.3 - 1) / 5  # (steps - 1) / (n - 1) at W = 64
    assert abs(co[0, 10, 0] - 10 * zoom) < 1e-9 and abs(co[1, 0, 10] - 10 * zoom) < 1e-9
    assert abs(co[0, -1, 0] - 63) < 1e-9 and abs(co[0, -2, 0] - 63) < 1e-9  # clamped at the far edge
    P, coef = R.tps_coefficients_ref(z["far_dst"], z["far_src"], 64)
    co = R.tps_coords(P, coef, 64)
    assert co.max() >= 128 and co.min() < -1


def test_fold_is_scipys_reflect():
    ndimage = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(0)
    img = rs.uniform(0, 255, (1, 23, 23))
    co = rs.uniform(-80, 100, (2, 23, 23))
    want = ndimage.map_coordinates(img[0], co, order=1, mode="reflect")
    assert np.abs(R.sample_reflect(img, co)[0] - want).max() <= 1e-9
    assert list(R.fold_reflect(np.array([-47, -24, -23, -1, 0, 22, 23, 45, 46, 47]), 23)) == [0, 22, 22, 0, 0, 22, 22, 0, 0, 1]


@pytest.mark.parametrize("h,w,S", [(201, 215, 224), (460, 500, 224), (143, 150, 224), (3, 1, 4), (5, 2, 3)])
def test_resize_restatement_matches_torch(h, w, S):
    """torch computes its centres and weights in fp32: 9 weight-ulps per axis (augment_ref.crop_bound)."""
    rs = np.random.RandomState(h)
    img = rs.randint(0, 256, (2, h + 3, w + 5)).astype(np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(img[None, :, 2:2 + h, 4:4 + w]).contiguous(), size=(S, S), mode="bilinear",
                                           align_corners=False, antialias=True)[0].numpy()
    got = R.crop_resize_flip_ref(img, (2, 4, h, w), False, S)
    err = np.abs(got - want).max()
    print(h, w, S, "max |restatement - torch| =", err, "bound", R.crop_bound(img, h, w))
    assert err <= R.crop_bound(img, h, w)
    assert np.array_equal(R.crop_resize_flip_ref(img, (2, 4, h, w), True, S), got[:, :, ::-1])


def test_tps_coefficients_match_numpy_pinv():
    import diverse_channel_vit_amd as dcv
    from diverse_channel_vit_amd import augment as A
    rs = np.random.RandomState(3)
    for W in (31, 160, 224):
        src = A.regular_grid(W)
        dst = src + torch.from_numpy(rs.uniform(-0.1 * W, 0.1 * W, (4, 9, 2)))
        coef = dcv.tps_coefficients(dst, src, W)
        assert coef.dtype == torch.float64 and coef.shape == (4, 2, 16)
        P = A.tps_control_points(dst, W)
        assert P.shape == (4, 13, 2) and P[0, 9:].tolist() == [[0, 0], [0, W], [W, 0], [W, W]]
        for b in range(4):
            Pr, cr = R.tps_coefficients_ref(dst[b].numpy(), src.numpy(), W)
            assert np.array_equal(P[b].numpy(), Pr)
            assert np.abs(coef[b].numpy() - cr).max() <= 1e-7 * np.abs(cr).max()
            # the spline interpolates: it takes every control point to its source point
            L = R.tps_L(Pr)
            assert np.abs(L[:13] @ cr.T - np.concatenate([src.numpy(), R.corners(W)])).max() <= 1e-6
    # the regular grid is the reference's point set
    g = np.linspace(0, 64, 3)
    assert sorted(map(tuple, A.regular_grid(64).tolist())) == sorted((a, b) for a in g for b in g)


def test_sample_invariants():
    import diverse_channel_vit_amd as dcv
    B, W = 512, 160
    aug = dcv.DeviceAugment(size=224, generator=torch.Generator().manual_seed(7))
    p = aug.sample(B, W, W)
    i, j, h, w = (p.box[:, k].long() for k in range(4))
    assert p.box.dtype == torch.int32 and bool(((i >= 0) & (j >= 0) & (h >= 1) & (w >= 1) & (i + h <= W) & (j + w <= W)).all())
    assert not bool(p.fallback.any())
    # accepted boxes: w = round(sqrt(A r)), h = round(sqrt(A / r)) with A in area * scale and r in ratio, each side off by at most 1/2
    lo_a, hi_a = 0.8 * W * W, 1.0 * W * W
    hf, wf = h.double(), w.double()
    assert bool(((wf + 0.5) * (hf + 0.5) >= lo_a).all()) and bool(((wf - 0.5) * (hf - 0.5) <= hi_a).all())
    assert bool(((wf + 0.5) / (hf - 0.5) >= 0.9).all()) and bool(((wf - 0.5) / (hf + 0.5) <= 1.1).all())
    assert 0.1 < p.tps.float().mean() < 0.3 and 0.4 < p.flip.float().mean() < 0.6
    assert p.dst.shape == (B, 9, 2) and p.dst.dtype == torch.float64 and float((p.dst - p.src).abs().max()) <= 0.1 * W
    assert float((p.dst - p.src).abs().max()) > 0.09 * W
    assert len(set(map(tuple, p.box.tolist()))) > B // 2  # positions and sizes vary
    # reproducible under a seeded generator, different under another seed
    q = dcv.DeviceAugment(size=224, generator=torch.Generator().manual_seed(7)).sample(B, W, W)
    for a, b in ((p.tps, q.tps), (p.flip, q.flip), (p.box, q.box), (p.dst, q.dst)):
        assert torch.equal(a, b)
    r = dcv.DeviceAugment(size=224, generator=torch.Generator().manual_seed(8)).sample(B, W, W)
    assert not torch.equal(p.tps, r.tps) and not torch.equal(p.box, r.box)


def test_sample_falls_back_to_the_centre_crop():
    import diverse_channel_vit_amd as dcv
    # area up to 4 x the image never fits: every sample takes the fallback, whole image at an aspect inside the range
    p = dcv.DeviceAugment(scale=(2.0, 4.0), ratio=(0.9, 1.1), generator=torch.Generator().manual_seed(0)).sample(16, 100, 100)
    assert bool(p.fallback.all()) and p.box.tolist() == [[0, 0, 100, 100]] * 16
    # image wider than the widest ratio: full height, w = round(H * max ratio), centred
    p = dcv.DeviceAugment(scale=(2.0, 4.0), ratio=(0.5, 1.25), generator=torch.Generator().manual_seed(0)).sample(4, 100, 200)
    assert bool(p.fallback.all()) and p.box.tolist() == [[0, 37, 100, 125]] * 4
    # narrower than the narrowest: full width, h = round(W / min ratio)
    p = dcv.DeviceAugment(scale=(2.0, 4.0), ratio=(0.8, 1.25), generator=torch.Generator().manual_seed(0)).sample(4, 200, 100)
    assert bool(p.fallback.all()) and p.box.tolist() == [[37, 0, 125, 100]] * 4
    # a range that fits only sometimes: both kinds in one batch, every box inside
    p = dcv.DeviceAugment(scale=(0.9, 1.0), ratio=(1.0, 2.0), generator=torch.Generator().manual_seed(1)).sample(256, 64, 64)
    assert bool(p.fallback.any()) and not bool(p.fallback.all())
    assert bool((p.box[:, 0] + p.box[:, 2] <= 64).all()) and bool((p.box[:, 1] + p.box[:, 3] <= 64).all())
    assert p.box[p.fallback].tolist() == [[0, 0, 64, 64]] * int(p.fallback.sum())


def test_refusals_need_no_gpu():
    import diverse_channel_vit_amd as dcv
    from diverse_channel_vit_amd import hip
    aug = dcv.DeviceAugment(size=16)
    for shape in ((2, 3, 30, 32), (2, 3, 20, 20), (1, 1, 1025, 1025)):  # non-square, below 21, above 1024
        x = torch.zeros(shape, dtype=torch.uint8)
        with pytest.raises(ValueError):
            aug.apply(x, aug.sample(shape[0], shape[2], shape[3]))
        P, coef = torch.zeros(shape[0], 13, 2, dtype=torch.float64), torch.zeros(shape[0], 2, 16, dtype=torch.float64)
        with pytest.raises(ValueError):
            hip.tps_warp(x, P, coef, torch.zeros(shape[0], dtype=torch.int32), torch.zeros(shape))
    with pytest.raises(ValueError):  # K > 32
        hip.tps_warp(torch.zeros(1, 1, 32, 32), torch.zeros(1, 33, 2, dtype=torch.float64), torch.zeros(1, 2, 36, dtype=torch.float64),
                     torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, 32, 32))
    with pytest.raises(ValueError):  # int64 images
        aug.apply(torch.zeros(1, 1, 32, 32, dtype=torch.int64), aug.sample(1, 32, 32))
    # scale > 8 on either axis
    x = torch.zeros(1, 1, 160, 160, dtype=torch.uint8)
    p = aug.sample(1, 160, 160)
    p.box = torch.tensor([[0, 0, 129, 16]], dtype=torch.int32)
    with pytest.raises(ValueError, match="scale"):
        aug.apply(x, p)
    p.box = torch.tensor([[0, 0, 16, 129]], dtype=torch.int32)
    with pytest.raises(ValueError, match="scale"):
        aug.apply(x, p)
    p.box = torch.tensor([[40, 0, 128, 128]], dtype=torch.int32)  # leaves the image
    with pytest.raises(ValueError, match="leaves"):
        aug.apply(x, p)
    with pytest.raises(ValueError):  # 160 -> 16 is scale 10
        aug.eval_transform(x)
    with pytest.raises(ValueError):
        aug.apply(x, aug.sample(2, 160, 160))  # parameters of another batch size
    # a legal call gets as far as the device check: no CPU fallback
    p.box = torch.tensor([[0, 0, 128, 128]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug.apply(x, p)
    with pytest.raises(ValueError):
        dcv.DeviceAugment(tps_prob=1.5)
    assert math.isclose(hip.CROP_MAX_SCALE, 8)
