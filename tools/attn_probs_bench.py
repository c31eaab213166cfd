"""Times the attention-probabilities kernel (dcv_attn_probs_rows / _ps) at the headline shape and what surrounds it, in one process, with events
after warm-up:
  * the kernel at B 64, H 6, N 1569 (3.78 GB written), both q forms;
  * torch.empty(same shape).fill_(0): the plain write rate of this box, the yardstick;
  * get_last_selfattention(layer_idx=11) against one eval forward of DiChaViT-S at the headline config (8 channels, 224 x 224, patch 16, bs 64).
With --nt it also times a variant build with non-temporal stores (-DDCV_PROBS_NT=1, libdcv_hip_probs_nt.so) in a child process.

    python tools/attn_probs_bench.py [--nt] [--iters 20]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, H, N = 64, 6, 1569


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


def kernel_times(iters):
    from diverse_channel_vit_amd import hip
    D = H * 64
    g = torch.Generator(device="cpu").manual_seed(0)
    qkv = (torch.randn(B, N, 3 * D, generator=g) * 1.2).to(torch.bfloat16).cuda()
    o = torch.empty(B, N, D, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, N, device="cuda")
    P = torch.empty(B, H, N, N, device="cuda")
    out = {}
    for ps in (False, True):
        hip.attn_fwd(qkv, o, lse, B, N, H, 64, 64 ** -0.5, prescaled=ps)
        out["ps" if ps else "plain"] = _time(lambda: hip.attn_probs(qkv, lse, P, B, N, H, 64, 64 ** -0.5, prescaled=ps), iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--nt", action="store_true", help="also time the non-temporal-store variant build")
    ap.add_argument("--kernel-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernel_only:
        print(json.dumps(kernel_times(a.iters)))
        return
    nbytes = 4.0 * B * H * N * N
    tb = lambda us: nbytes / (us * 1e-6) / 1e12  # noqa: E731
    res = {"shape": f"B{B} H{H} N{N}", "bytes": nbytes}
    fill = torch.empty(B, H, N, N, device="cuda")
    res["fill_us"] = _time(lambda: fill.fill_(0), a.iters)
    del fill
    for k, us in kernel_times(a.iters).items():
        res[f"kernel_{k}_us"] = us
    if a.nt:
        from diverse_channel_vit_amd import _build
        lib = os.path.join(ROOT, "diverse_channel_vit_amd", "libdcv_hip_probs_nt.so")
        src = os.path.join(ROOT, "diverse_channel_vit_amd", "csrc", "attn_probs.hip")
        if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
            _build.build_variant("probs_nt", ["DCV_PROBS_NT=1"])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-only", "--iters", str(a.iters)], env={**os.environ, "DCV_LIB": lib},
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        for k, us in json.loads(r.stdout.strip().splitlines()[-1]).items():
            res[f"kernel_{k}_nt_us"] = us
    # the model method against one eval forward, DiChaViT-S at the headline config
    import diverse_channel_vit_amd as dcv

    class Cfg(dict):
        __getattr__ = dict.get

    cfg = Cfg(name="dichavit", pretrained_model_name="small", patch_size=16, temperature=0.07, learnable_temp=False, enable_sample=False,
              use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False, block_type="block",
              hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.001, ortho_loss_v1_lambda=0.1, drop_path_rate=0.0, gamma_s=0.5,
              gamma_d=4.0, reverse_pos_pairs=True, use_square=False, in_channel_names=list(range(8)), img_size=[224], num_classes=161)
    model = dcv.dichavit(cfg, mapper={"train": list(range(8))}).cuda().eval()
    x = torch.randn(B, 8, 224, 224, device="cuda")
    with torch.no_grad():
        res["eval_forward_us"] = _time(lambda: model(x, "train", None), max(a.iters // 2, 5))
        res["get_last_selfattention_us"] = _time(lambda: model.feature_extractor.get_last_selfattention(x, chunk="train", layer_idx=11),
                                                 max(a.iters // 2, 5))
    for k in list(res):
        if k.startswith("kernel_") or k == "fill_us":
            res[k.replace("_us", "_TBps")] = round(tb(res[k]), 3)
    for k in list(res):
        if k.startswith("kernel_") and k.endswith("_us"):
            res[k.replace("_us", "_vs_fill")] = round(res["fill_us"] / res[k], 3)
    for k, v in res.items():
        print(f"{k:32s} {v:.1f}" if isinstance(v, float) else f"{k:32s} {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
