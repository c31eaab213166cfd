"""Times the LayerNorm channel-pool kernel (dcv_ln_pool_channels) and what surrounds it, in one process, with events after warm-up, the
candidates alternating inside every round (median of --iters rounds), at B 64, n_p 196, D 384 with C 8 (the headline shape) and C 3
(CHAMMI-sized):
  (a) the kernel: reads the residual stream once (B N D 4 bytes), writes B (1 + C) D floats;
  (b) what it replaces, from kernels that exist without it: dcv_ln_fwd with fp32 output, then torch.mean over the reshaped patch rows into a
      preallocated output (the CLS rows are not even copied: (b) does slightly less than (a));
  (c) the floor: a device-to-device copy that moves the same number of bytes in total as the kernel must read (a copy of X bytes moves 2 X,
      so half as many are copied).
(a) must be faster than (b) — it moves a third of the bytes: the tool prints a line starting with DEFECT and exits with status 1 otherwise.
Then get_intermediate_layers(n=4, pool="channel") and (n=4, pool=None) against one eval forward of DiChaViT-S at the headline config (8 channels,
224 x 224, patch 16, bs 64).
With --variants it also times a variant build of the kernel's launch plan (-DDCV_LP_TARGET_WGS=512: one workgroup per segment at the headline
shape, no workspace, no second launch) in a child process.

    python tools/intermediate_layers_bench.py [--iters 50] [--variants]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, N_P, D = 64, 196, 384
VARIANTS = {"lp_wg512": ["DCV_LP_TARGET_WGS=512"]}


def variant_lib(name):
    return os.path.join(ROOT, "diverse_channel_vit_amd", f"libdcv_hip_{name}.so")


def build_variants():
    from diverse_channel_vit_amd import _build
    src = os.path.join(ROOT, "diverse_channel_vit_amd", "csrc", "ln_pool.hip")
    for name, defines in VARIANTS.items():
        lib = variant_lib(name)
        if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
            _build.build_variant(name, defines)


def _time_alternating(fns, iters, warmup=5):
    """{name: fn} -> {name: median us}; one launch of each per round, so drift in clocks or neighbours hits every candidate alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ts[k].append(s.elapsed_time(e) * 1e3)
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


def kernel(res, C, iters):
    from diverse_channel_vit_amd import hip
    N = 1 + C * N_P
    g = torch.Generator(device="cuda").manual_seed(C)
    x = torch.randn(B, N, D, device="cuda", generator=g) * 3.0 + 5.0
    gamma, beta = 1 + 0.1 * torch.randn(D, device="cuda", generator=g), 0.1 * torch.randn(D, device="cuda", generator=g)
    out = torch.empty(B, 1 + C, D, device="cuda")
    normed = torch.empty(B, N, D, device="cuda")
    means = torch.empty(B, C, D, device="cuda")
    nbytes = 4.0 * B * N * D
    src = torch.empty(int(nbytes // 8), dtype=torch.float32, device="cuda")  # reads and writes nbytes / 2 each
    dst = torch.empty_like(src)

    def replaced():
        hip.ln_fwd(x, gamma, beta, normed, None, None, B * N, D, 1e-6)
        torch.mean(normed[:, 1:].view(B, C, N_P, D), dim=2, out=means)

    t = _time_alternating({"pool": lambda: hip.ln_pool_channels(x, gamma, beta, out, B, C, N_P, D, 1e-6), "ln_fwd_then_mean": replaced,
                           "copy_same_bytes": lambda: dst.copy_(src)}, iters)
    replaced()
    tag = f"C{C}"
    res[f"{tag}_shape"] = f"B{B} C{C} n_p{N_P} D{D}"
    res[f"{tag}_read_bytes"] = nbytes
    res[f"{tag}_ws_floats"] = int(hip.load().dcv_ln_pool_channels_ws_floats(B, C, N_P, D))
    res[f"{tag}_pool_us"] = t["pool"]
    res[f"{tag}_ln_fwd_then_mean_us"] = t["ln_fwd_then_mean"]
    res[f"{tag}_copy_same_bytes_us"] = t["copy_same_bytes"]
    res[f"{tag}_pool_TBps"] = round(nbytes / (t["pool"] * 1e-6) / 1e12, 3)
    res[f"{tag}_pool_vs_replaced"] = round(t["pool"] / t["ln_fwd_then_mean"], 3)
    res[f"{tag}_pool_vs_copy_floor"] = round(t["pool"] / t["copy_same_bytes"], 3)
    res[f"{tag}_max_abs_diff_to_replaced"] = max((out[:, 1:] - means).abs().max().item(), (out[:, 0] - normed[:, 0]).abs().max().item())


def model_times(res, iters):
    import diverse_channel_vit_amd as dcv

    class Cfg(dict):
        __getattr__ = dict.get

    C = 8
    cfg = Cfg(name="dichavit", pretrained_model_name="small", patch_size=16, temperature=0.07, learnable_temp=False, enable_sample=False,
              use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False, block_type="block",
              hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.001, ortho_loss_v1_lambda=0.1, drop_path_rate=0.0, gamma_s=0.5,
              gamma_d=4.0, reverse_pos_pairs=True, use_square=False, in_channel_names=list(range(C)), img_size=[224], num_classes=161)
    model = dcv.dichavit(cfg, mapper={"train": list(range(C))}).cuda().eval()
    fe = model.feature_extractor
    x = torch.randn(B, C, 224, 224, device="cuda")
    with torch.no_grad():
        t = _time_alternating({"eval_forward": lambda: model(x, "train", None),
                               "n4_channel": lambda: fe.get_intermediate_layers(x, n=4, chunk="train", pool="channel"),
                               "n4_tokens": lambda: fe.get_intermediate_layers(x, n=4, chunk="train")}, max(iters // 5, 5), warmup=2)
    res["eval_forward_ms"] = round(t["eval_forward"] / 1e3, 3)
    res["get_intermediate_layers_n4_channel_ms"] = round(t["n4_channel"] / 1e3, 3)
    res["get_intermediate_layers_n4_tokens_ms"] = round(t["n4_tokens"] / 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--variants", action="store_true", help="also time the variant builds of the launch plan (built on demand)")
    ap.add_argument("--build-variants", action="store_true", help="build the variant libraries and exit (needs hipcc, no GPU)")
    ap.add_argument("--kernel-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.build_variants:
        build_variants()
        return
    if not torch.cuda.is_available():
        raise SystemExit("intermediate_layers_bench needs the GPU: a CPU run gives no time")
    res = {}
    for C in (8, 3):
        kernel(res, C, a.iters)
    if a.kernel_only:
        print(json.dumps(res))
        return
    if a.variants:
        if not all(os.path.exists(variant_lib(name)) for name in VARIANTS):  # --build-variants beforehand keeps hipcc out of the timed session
            build_variants()
        for name in VARIANTS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-only", "--iters", str(a.iters)],
                               env={**os.environ, "DCV_LIB": variant_lib(name)}, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(r.stderr)
            for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                if k.endswith(("_pool_us", "_ws_floats", "_ln_fwd_then_mean_us", "_copy_same_bytes_us")):
                    res[f"{name}_{k}"] = v
    model_times(res, a.iters)
    for k, v in res.items():
        print(f"{k:44s} {v:.3f}" if isinstance(v, float) else f"{k:44s} {v}")
    print(json.dumps(res))
    slow = [c for c in (8, 3) if res[f"C{c}_pool_us"] >= res[f"C{c}_ln_fwd_then_mean_us"]]
    if slow:
        print(f"DEFECT: dcv_ln_pool_channels is not faster than dcv_ln_fwd + torch.mean at C = {slow}")
        raise SystemExit(1)


if __name__ == "__main__":
    main()
