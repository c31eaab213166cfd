"""Times input-image gradients at the headline shape (DiChaViT-S, 8 channels, 224 x 224, patch 16, bs 64), in one process, with events after
warm-up (median of --iters):
  * dcv_patch_dgrad alone (M = 100 352 token rows, D 384): reads 77.1 MB of dY, writes 102.8 MB of dx — against the 180 MB / 6.29 TB/s copy-rate
    floor (28.7 us) and against a same-size device copy (dx.copy_(other)) measured here;
  * a saliency call — eval forward + torch.autograd.grad(logits[b, y_b].sum(), x) — with frozen weights (the data-only backward) and with the
    weights requiring grad (the full backward);
  * a training step's forward + backward (CE + extra) with and without x.requires_grad.

    python tools/input_grad_bench.py [--iters 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, C, IMG, P, D = 64, 8, 224, 16, 384
FLOOR_TBPS = 6.29


def _time(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]  # median, us


def kernel(res, iters):
    from diverse_channel_vit_amd import hip
    n = (IMG // P) ** 2
    M = B * C * n
    g = torch.Generator(device="cpu").manual_seed(0)
    dY = (torch.randn(M, D, generator=g) * 1e-3).to(torch.bfloat16).cuda()
    W = (torch.randn(D, P * P, generator=g) * 0.05).to(torch.bfloat16).cuda()
    ch = torch.arange(C, dtype=torch.int32, device="cuda")
    dx = torch.empty(B, C, IMG, IMG, device="cuda")
    nbytes = 2.0 * M * D + 4.0 * dx.numel()
    res.update(shape=f"M{M} D{D} P{P} B{B} C{C} {IMG}x{IMG}", bytes=nbytes, floor_us=round(nbytes / (FLOOR_TBPS * 1e12) * 1e6, 1))
    res["patch_dgrad_us"] = _time(lambda: hip.patch_dgrad(dY, W, ch, dx, B, C, C, IMG, IMG, P), iters)
    src = torch.empty(int(nbytes // 8), dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)  # a device copy that reads and writes 90 MB each: 180 MB moved
    res["copy_same_bytes_us"] = _time(lambda: dst.copy_(src), iters)
    res["patch_dgrad_TBps"] = round(nbytes / (res["patch_dgrad_us"] * 1e-6) / 1e12, 3)
    res["patch_dgrad_vs_floor"] = round(res["patch_dgrad_us"] / res["floor_us"], 2)


def model_times(res, iters):
    import diverse_channel_vit_amd as dcv

    class Cfg(dict):
        __getattr__ = dict.get

    cfg = Cfg(name="dichavit", pretrained_model_name="small", patch_size=P, temperature=0.07, learnable_temp=False, enable_sample=False,
              use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False, block_type="block",
              hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.001, ortho_loss_v1_lambda=0.1, drop_path_rate=0.0, gamma_s=0.5,
              gamma_d=4.0, reverse_pos_pairs=True, use_square=False, in_channel_names=list(range(C)), img_size=[IMG], num_classes=161)
    model = dcv.dichavit(cfg, mapper={"train": list(range(C))}).cuda()
    x = torch.randn(B, C, IMG, IMG, device="cuda")
    y = torch.randint(0, 161, (B,), device="cuda")

    def saliency():
        xg = x.detach().requires_grad_(True)
        out = model(xg, "train", None)
        return torch.autograd.grad(out.gather(1, y[:, None]).sum(), xg)[0]

    model.eval()
    it = max(iters // 2, 5)
    res["saliency_full_bwd_ms"] = round(_time(saliency, it) / 1e3, 3)
    for p in model.parameters():
        p.requires_grad_(False)
    res["saliency_data_only_ms"] = round(_time(saliency, it) / 1e3, 3)
    for p in model.parameters():
        p.requires_grad_(True)
    with torch.no_grad():
        res["eval_forward_ms"] = round(_time(lambda: model(x, "train", None), it) / 1e3, 3)
    model.train()

    def step(xin):
        model.zero_grad(set_to_none=True)
        out, extra = model(xin, "train", None)
        (torch.nn.functional.cross_entropy(out, y) + extra).backward()

    res["train_fwd_bwd_ms"] = round(_time(lambda: step(x), it) / 1e3, 3)
    res["train_fwd_bwd_x_grad_ms"] = round(_time(lambda: step(x.detach().requires_grad_(True)), it) / 1e3, 3)
    res["train_fwd_bwd_again_ms"] = round(_time(lambda: step(x), it) / 1e3, 3)  # the first measurement repeated: the spread of the pair


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    res = {}
    kernel(res, a.iters)
    model_times(res, a.iters)
    for k, v in res.items():
        print(f"{k:32s} {v:.3f}" if isinstance(v, float) else f"{k:32s} {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
