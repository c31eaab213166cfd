"""dcv_tps_warp and dcv_crop_resize_flip on the GPU (csrc/augment.hip) against the fixture recorded from the real reference
(tests/golden/tps_warp.npz), the float64 restatements of tests/augment_ref.py and torch's CPU interpolate; then DeviceAugment end to end.

Bounds (augment_ref.tps_bound / crop_bound), every element compared:
  warp:   2 G W 2^-21 + 4 2^-24 max|x|, G the largest adjacent-pixel difference — an fp32 coordinate error of about W 2^-21 pixel times the
          bilinear slope on both axes, plus the rounding of the fp32 blend.  A wrong tap, fold or upsampling rule is off by whole grey levels.
  resize: 18 max(h, w) 2^-24 max|x| — fp32 centres, 9 weight-ulps per axis."""
import numpy as np
import pytest
import torch

import augment_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _warp(dev, x, dst, src, flags, sentinel=-7.0):
    """x [B, C, W, W] host tensor, dst [B, 9, 2] / src [9, 2] float64 -> (out [B, C, W, W] on the host, the device tensors used)."""
    from diverse_channel_vit_amd import augment as A, hip
    B, W = x.shape[0], x.shape[-1]
    P = A.tps_control_points(torch.as_tensor(dst), W).to(dev)
    coef = A.tps_coefficients(torch.as_tensor(dst), torch.as_tensor(src), W).to(dev)
    apply = torch.tensor(flags, dtype=torch.int32, device=dev)
    out = torch.full((B,) + tuple(x.shape[1:]), sentinel, dtype=torch.float32, device=dev)
    xd = x.to(dev)
    hip.tps_warp(xd, P, coef, apply, out)
    return out.cpu(), (xd, P, coef, apply)


def _close(got, want, bound, what):
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    print(f"{what}: max |out - ref| = {err:.3e}, bound {bound:.3e} ({err / bound:.3f} of it)")
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_tps_warp_matches_the_reference_fixture(gpu_device, dtype):
    """Every fixture case (W 31, 64, 160, 224; C 1, 3, 5; zero displacement; coordinates that fold twice) against the real reference's output."""
    meta, z = load_golden("tps_warp")
    for c in meta["cases"]:
        n, W = c["name"], c["W"]
        img = z[n + "_img"]
        x = torch.from_numpy(img)[None].to(dtype)
        out, _ = _warp(gpu_device, x, z[n + "_dst"][None], z[n + "_src"], [1])
        _close(out[0].numpy(), z[n + "_out"].astype(np.float64), R.tps_bound(img, W), f"{n} {dtype}")


@pytest.mark.parametrize("W,C", [(21, 1), (31, 3), (64, 5), (160, 3)])
def test_tps_warp_batch_with_mixed_flags(gpu_device, W, C):
    """B = 5 with flags 1 0 1 1 0 against the restatement; unflagged samples keep the sentinel; a second call agrees bit for bit; uint8 and
    float32 input give the same bits for the same pixel values."""
    from diverse_channel_vit_amd import augment as A, hip
    rs = np.random.RandomState(W)
    flags = [1, 0, 1, 1, 0]
    img = rs.randint(0, 256, (5, C, W, W)).astype(np.uint8)
    src = A.regular_grid(W)
    dst = src + torch.from_numpy(rs.uniform(-0.1 * W, 0.1 * W, (5, 9, 2)))
    out, (xd, P, coef, apply) = _warp(gpu_device, torch.from_numpy(img), dst, src, flags)
    for b, f in enumerate(flags):
        if f:
            _close(out[b].numpy(), R.tps_warp_ref(img[b], dst[b].numpy(), src.numpy()), R.tps_bound(img[b], W), f"W{W} C{C} sample {b}")
        else:
            assert bool((out[b] == -7.0).all()), "an unflagged sample's workspace was written"
    again = torch.full_like(out, -7.0).to(gpu_device)
    hip.tps_warp(xd, P, coef, apply, again)
    assert torch.equal(again.cpu(), out)
    outf, _ = _warp(gpu_device, torch.from_numpy(img).float(), dst, src, flags)
    assert torch.equal(outf, out)


def test_tps_warp_far_coordinates_and_float_images(gpu_device):
    """An affine 'spline' (kernel weights 0) that maps the image to coordinates from -1.6 W to 2.7 W: every fold count up to two on both sides, on
    float images with negative values and fractions; K = 32 control points, the most the kernel takes."""
    from diverse_channel_vit_amd import hip
    W, C, K = 43, 2, 32
    rs = np.random.RandomState(1)
    img = rs.uniform(-300, 500, (1, C, W, W)).astype(np.float32)
    P = rs.uniform(0, W, (1, K, 2))
    coef = np.zeros((1, 2, K + 3))
    coef[0, 0, K:] = [-1.6 * W, 4.3, 0.4]
    coef[0, 1, K:] = [2.7 * W - 0.25, -0.3, -4.1]
    coef[0, :, :K] = rs.uniform(-1e-3, 1e-3, (2, K)) / W
    co = R.tps_coords(P[0], coef[0], W)
    assert co.min() < -1.5 * W and co.max() > 2.5 * W
    out = torch.full((1, C, W, W), -7.0, device=gpu_device)
    hip.tps_warp(torch.from_numpy(img).to(gpu_device), torch.from_numpy(P).to(gpu_device), torch.from_numpy(coef).to(gpu_device),
                 torch.ones(1, dtype=torch.int32, device=gpu_device), out)
    # the coordinate error grows with the coordinate's size: 2.7 W instead of W
    _close(out[0].cpu().numpy(), R.sample_reflect(img[0], co), 3 * R.tps_bound(img[0], W), "affine far")


def _crop(dev, x, box, flip, S, warped=None, use=None, guard=8):
    from diverse_channel_vit_amd import hip
    B, C = x.shape[:2]
    buf = torch.full((guard + B * C * S * S + guard,), 1234.5, dtype=torch.float32, device=dev)
    out = buf[guard:guard + B * C * S * S].view(B, C, S, S)
    xd = x.to(dev)
    hip.crop_resize_flip(xd, None if warped is None else warped.to(dev), None if use is None else torch.tensor(use, dtype=torch.int32, device=dev),
                         torch.tensor(box, dtype=torch.int32, device=dev), torch.tensor(flip, dtype=torch.int32, device=dev), out)
    buf = buf.cpu()
    assert bool((buf[:guard] == 1234.5).all()) and bool((buf[-guard:] == 1234.5).all()), "guard floats around the output were written"
    return buf[guard:-guard].view(B, C, S, S)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_crop_identity_box_is_a_copy_or_a_mirror(gpu_device, dtype):
    S = 37
    rs = np.random.RandomState(2)
    x = torch.from_numpy(rs.randint(0, 256, (2, 3, 50, 61)).astype(np.uint8)).to(dtype)
    out = _crop(gpu_device, x, [[5, 7, S, S], [13, 24, S, S]], [0, 1], S)
    assert torch.equal(out[0], x[0, :, 5:5 + S, 7:7 + S].float())
    assert torch.equal(out[1], x[1, :, 13:13 + S, 24:24 + S].float().flip(-1))


def test_crop_half_scale_closed_form(gpu_device):
    """A 2S x 2S box: weights 1/8 3/8 3/8 1/8 per axis for the interior outputs, exact on small integers; the two border outputs per axis see
    three taps with weights 3/7 3/7 1/7 and go by tolerance."""
    S = 24
    rs = np.random.RandomState(3)
    x = torch.from_numpy(rs.randint(0, 32, (1, 2, 2 * S + 3, 2 * S + 2)).astype(np.uint8))
    out = _crop(gpu_device, x, [[3, 1, 2 * S, 2 * S]], [0], S)[0].double()
    c = x[0, :, 3:, 1:1 + 2 * S].double()
    k = torch.tensor([1, 3, 3, 1], dtype=torch.float64) / 8
    rows = sum(k[t] * c[:, 1 + t:1 + t + 2 * S - 4:2, :] for t in range(4))        # output rows 1 .. S - 2
    want = sum(k[t] * rows[:, :, 1 + t:1 + t + 2 * S - 4:2] for t in range(4))
    assert torch.equal(out[:, 1:-1, 1:-1], want)
    full = R.crop_resize_flip_ref(x[0].numpy(), (3, 1, 2 * S, 2 * S), False, S)
    assert abs(R.aa_weights(2 * S, S)[0, :3] - np.array([3, 3, 1]) / 7).max() < 1e-15
    _close(out.numpy(), full, R.crop_bound(x[0].numpy(), 2 * S, 2 * S), "half scale, borders included")


GENERAL = [  # (H, W, S, box, what)
    (40, 44, 56, (3, 5, 30, 33), "upscale"),
    (130, 140, 56, (1, 6, 128, 128), "downscale 2.29"),
    (215, 90, 56, (0, 10, 215, 61), "non-square, 3.84 by 1.09"),
    (70, 80, 32, (0, 0, 50, 60), "top left corner"),
    (70, 80, 32, (20, 20, 50, 60), "bottom right corner"),
    (70, 80, 32, (0, 0, 70, 80), "whole image"),
    (70, 80, 32, (9, 37, 55, 1), "w = 1"),
    (70, 80, 32, (33, 2, 1, 77), "h = 1"),
    (300, 270, 33, (10, 3, 264, 263), "downscale 8 with an odd size"),
]


def test_crop_general_boxes(gpu_device):
    """Each box as a batch of two images, the second flipped, from uint8 and from float32 input, against the float64 restatement and against
    torch's CPU interpolate(antialias=True) of the cropped box."""
    for H, W, S, box, what in GENERAL:
        rs = np.random.RandomState(H + W)
        img = rs.randint(0, 256, (2, 2, H, W)).astype(np.uint8)
        i, j, h, w = box
        bound = R.crop_bound(img, h, w)
        for dtype in (torch.uint8, torch.float32):
            out = _crop(gpu_device, torch.from_numpy(img).to(dtype), [box, box], [0, 1], S)
            for b, flip in enumerate((False, True)):
                _close(out[b].numpy(), R.crop_resize_flip_ref(img[b], box, flip, S), bound, f"{what} {dtype} flip {flip} vs restatement")
                t = torch.nn.functional.interpolate(torch.from_numpy(img[b:b + 1, :, i:i + h, j:j + w]).float().contiguous(), size=(S, S), mode="bilinear",
                                                    align_corners=False, antialias=True)[0]
                _close(out[b].numpy(), (t.flip(-1) if flip else t).double().numpy(), bound, f"{what} {dtype} flip {flip} vs torch")


def test_crop_reads_both_sources_in_one_batch(gpu_device):
    S = 20
    rs = np.random.RandomState(4)
    x = torch.from_numpy(rs.randint(0, 256, (4, 3, 31, 31)).astype(np.uint8))
    warped = torch.from_numpy(rs.uniform(0, 255, (4, 3, 31, 31)).astype(np.float32))
    use, flip = [0, 1, 1, 0], [1, 1, 0, 0]
    box = [[0, 0, 31, 31], [2, 3, 25, 27], [5, 5, 20, 20], [1, 0, 30, 29]]
    out = _crop(gpu_device, x, box, flip, S, warped=warped, use=use)
    for b in range(4):
        src = (warped if use[b] else x.float())[b].numpy()
        _close(out[b].numpy(), R.crop_resize_flip_ref(src, box[b], flip[b], S), R.crop_bound(src, box[b][2], box[b][3]), f"sample {b} source {use[b]}")
    assert torch.equal(out[2], warped[2, :, 5:25, 5:25])  # the identity box of the warped source, bit for bit


def _params(aug, B, W, tps, flip):
    p = aug.sample(B, W, W)
    p.tps, p.flip = torch.tensor(tps, dtype=torch.bool), torch.tensor(flip, dtype=torch.bool)
    return p


def _pipeline_ref(img, p, S):
    """stage 2 o stage 1 of the restatement, and the sum of the two bounds per sample."""
    outs, bounds = [], []
    for b in range(img.shape[0]):
        W = img.shape[-1]
        mid = R.tps_warp_ref(img[b], p.dst[b].numpy(), p.src.numpy()) if bool(p.tps[b]) else img[b].astype(np.float64)
        box = p.box[b].tolist()
        outs.append(R.crop_resize_flip_ref(mid, box, bool(p.flip[b]), S))
        bounds.append((R.tps_bound(img[b], W) if bool(p.tps[b]) else 0.0) + R.crop_bound(img[b], box[2], box[3]))
    return np.stack(outs), bounds


def test_pipeline_matches_the_composed_restatement(gpu_device):
    import diverse_channel_vit_amd as dcv
    B, C, W, S = 5, 3, 64, 48
    rs = np.random.RandomState(6)
    img = rs.randint(0, 256, (B, C, W, W)).astype(np.uint8)
    aug = dcv.DeviceAugment(size=S, generator=torch.Generator().manual_seed(11))
    p = _params(aug, B, W, [1, 0, 1, 0, 1], [0, 1, 1, 0, 0])
    want, bounds = _pipeline_ref(img, p, S)
    x = torch.from_numpy(img).to(gpu_device)
    out = aug.apply(x, p)
    assert out.shape == (B, C, S, S) and out.dtype == torch.float32
    for b in range(B):
        _close(out[b].cpu().numpy(), want[b], bounds[b], f"pipeline sample {b} tps {int(p.tps[b])} flip {int(p.flip[b])}")
    ws = aug._ws
    assert torch.equal(aug.apply(x, p), out) and aug._ws is ws  # bit for bit, and the workspace is reused
    assert torch.equal(aug.apply(x.float(), p), out)
    assert aug(x).shape == (B, C, S, S)
    # the eval transform: the whole image resized, no warp, no flip
    ev = dcv.DeviceAugment(size=S).eval_transform(x)
    for b in range(B):
        _close(ev[b].cpu().numpy(), R.crop_resize_flip_ref(img[b], (0, 0, W, W), False, S), R.crop_bound(img[b], W, W), f"eval sample {b}")


def test_augmented_batch_feeds_the_model(gpu_device):
    """The smoke() architecture with set_input_normalisation on the device-augmented raw batch against the same weights without input
    normalisation on the CPU-restated, CPU-normalised batch, at test_fused_input_normalisation's tolerance."""
    import diverse_channel_vit_amd as dcv
    from oracle import dichavit_oracle as orc

    class Cfg(dict):
        __getattr__ = dict.get

    base = dict(name="dichavit", pretrained_model_name="small", patch_size=8, temperature=0.07, learnable_temp=False, enable_sample=False,
                use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False, block_type="block",
                hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.001, ortho_loss_v1_lambda=0.1, drop_path_rate=0.0, gamma_s=0.5,
                gamma_d=4.0, reverse_pos_pairs=True, use_square=False)
    C, S, K, B, W = 6, 32, 7, 4, 40
    st = orc.make_state(orc.state_shapes(base, C, S, K), 3)
    rs = np.random.RandomState(9)
    mean, std = rs.uniform(0.02, 0.3, C).astype(np.float32), rs.uniform(0.05, 0.2, C).astype(np.float32)
    img = rs.randint(0, 256, (B, C, W, W)).astype(np.uint8)
    aug = dcv.DeviceAugment(size=S, generator=torch.Generator().manual_seed(5))
    p = _params(aug, B, W, [1, 0, 0, 1], [1, 0, 1, 0])
    raw = aug.apply(torch.from_numpy(img).to(gpu_device), p)
    want, _ = _pipeline_ref(img, p, S)
    ref_in = torch.from_numpy(((want / 255.0 - mean[None, :, None, None]) / std[None, :, None, None]).astype(np.float32))
    feats = []
    for fused in (False, True):
        model = dcv.dichavit(Cfg(base, in_channel_names=list(range(C)), img_size=[S], num_classes=K), mapper={"train": list(range(C))})
        model.load_state_dict({**st, "adaptive_interface.0": st["proxies"]})
        model = model.to(gpu_device).train()
        model.stochastic_weight_rounding = False
        if fused:
            model.set_input_normalisation(mean, std, 255.0)
        out, extra = model(raw if fused else ref_in.to(gpu_device), "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        feats.append((out.detach().clone(), extra.item()))
    (f0, e0), (f1, e1) = feats
    assert (f0 - f1).abs().max().item() <= 2e-2 * f0.abs().max().item()
    assert abs(e0 - e1) <= 1e-3 * abs(e0) + 1e-6
