"""Times the relevance-step attention kernel (dcv_attn_relevance_step_ps) and the call built on it, in one process, with device events after
warm-up, the candidates alternating inside every round (median of --iters rounds), at the headline shape B 64, H 6, C 8, n_p 196 (N 1569),
pre-scaled q:
  (a) the kernel, per block: one relevance step (all query rows, and the CLS row alone as in the last block) against one rollout step on the
      same qkv — it issues twice the MFMA work — and against a device copy that moves the same bytes (qkv and dO read once: 8 B N D bytes);
  (b) what it replaces, on B_SMALL images (the [B,H,N,N] arrays of 64 do not fit beside each other): dcv_attn_probs_rows_ps into a [B,H,N,N]
      buffer, dO V^T as a torch matmul into a second one, relu, product, head mean and the vector-matrix product in torch — against the
      kernel on the same B_SMALL images;
  (c) whole calls on DiChaViT-S at the headline config (8 channels, 224 x 224, patch 16, bs 64): get_attention_relevance() against the
      saliency call it extends (eval forward + the data-only backward of one logit per image to the input) and against one eval forward.
The kernel must beat (b) by more than (b)'s own spread over the run; everything else is recorded, not required.  The tool prints a line starting
with DEFECT and exits with status 1 otherwise.

    python tools/attention_relevance_bench.py [--iters 30] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from attention_rollout_bench import _median, _time_alternating  # noqa: E402

B, H, C, N_P = 64, 6, 8, 196
N = 1 + C * N_P
D = H * 64
SCALE = 64 ** -0.5
B_SMALL = 4


def kernel(res, iters):
    from diverse_channel_vit_amd import hip
    g = torch.Generator(device="cuda").manual_seed(8)
    qkv = torch.randn(B, N, 3 * D, device="cuda", generator=g) * 1.5
    qkv[..., :D] *= SCALE * math.log2(math.e)  # the pre-scaled q the model's operand copies deliver
    qkv = qkv.to(torch.bfloat16)
    dO = (torch.randn(B, N, D, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    o = torch.empty(B, N, D, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, N, device="cuda")
    hip.attn_fwd(qkv, o, lse, B, N, H, 64, SCALE, prescaled=True)
    w = torch.rand(B, N, device="cuda", generator=g)
    e0 = torch.zeros(B, N, device="cuda")
    e0[:, 0] = 1.0
    out, out0, out1, outs = (torch.empty(B, N, device="cuda") for _ in range(4))
    nbytes = 2 * B * N * 4 * D  # qkv and dO, read once
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    P = torch.empty(B_SMALL, H, N, N, device="cuda")
    got = {}

    def replaced():
        hip.attn_probs(qkv, lse, P, B_SMALL, N, H, 64, SCALE, prescaled=True)
        v = qkv[:B_SMALL].view(B_SMALL, N, 3, H, 64)[:, :, 2].transpose(1, 2).float()
        G = dO[:B_SMALL].view(B_SMALL, N, H, 64).transpose(1, 2).float() @ v.transpose(-1, -2)
        got["r"] = w[:B_SMALL] + torch.einsum("bq,bqk->bk", w[:B_SMALL], (G.clamp_(min=0) * P).mean(1))

    t = _time_alternating({
        "relevance_step": lambda: hip.attn_relevance_step(qkv, lse, dO, w, out, B, N, H, 64, SCALE, prescaled=True),
        "rollout_step": lambda: hip.attn_rollout_step(qkv, lse, w, out1, B, N, H, 64, SCALE, 0.5, prescaled=True),
        "relevance_step_cls_row": lambda: hip.attn_relevance_step(qkv, lse, dO, e0, out0, B, N, H, 64, SCALE, nq=1, prescaled=True),
        "same_bytes_copy": lambda: dst.copy_(src),
        "relevance_step_b_small": lambda: hip.attn_relevance_step(qkv, lse, dO, w, outs, B_SMALL, N, H, 64, SCALE, prescaled=True),
        "probs_dOVt_relu_mean_einsum_b_small": replaced}, iters)
    replaced()
    torch.cuda.synchronize()
    res["shape"] = f"B{B} H{H} C{C} n_p{N_P} N{N} pre-scaled q"
    res["rounds"] = iters
    res["mfma_gflop"] = round(4.0 * B * H * N * N * 64 / 1e9, 1)
    res["hbm_bytes"] = nbytes + 4 * B * N * (H + 2)
    res["workgroups"] = B * ((N + 127) // 128)
    for k, v in t.items():
        res[f"{k}_us"] = round(_median(v), 1)
        res[f"{k}_min_max_us"] = f"{v[0]:.1f} .. {v[-1]:.1f}"
    res["relevance_step_vs_rollout_step"] = round(_median(t["relevance_step"]) / _median(t["rollout_step"]), 3)
    res["relevance_step_vs_same_bytes_copy"] = round(_median(t["relevance_step"]) / _median(t["same_bytes_copy"]), 2)
    res["relevance_step_TFLOPs"] = round(4.0 * B * H * N * N * 64 / (_median(t["relevance_step"]) * 1e-6) / 1e12, 1)
    res["b_small"] = B_SMALL
    res["replaced_arrays_bytes_b_small"] = 2 * 4 * B_SMALL * H * N * N
    res["relevance_step_vs_replaced_b_small"] = round(_median(t["relevance_step_b_small"]) / _median(t["probs_dOVt_relu_mean_einsum_b_small"]), 4)
    mag = got["r"].abs()
    res["max_rel_diff_to_replaced_b_small"] = ((outs[:B_SMALL] - got["r"]).abs() / mag).max().item()
    slow = t["probs_dOVt_relu_mean_einsum_b_small"]
    return _median(slow) - _median(t["relevance_step_b_small"]), slow[-1] - slow[0]


def model_times(res, iters):
    import diverse_channel_vit_amd as dcv

    class Cfg(dict):
        __getattr__ = dict.get

    cfg = Cfg(name="dichavit", pretrained_model_name="small", patch_size=16, temperature=0.07, learnable_temp=False, enable_sample=False,
              use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False, block_type="block",
              hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.001, ortho_loss_v1_lambda=0.1, drop_path_rate=0.0, gamma_s=0.5,
              gamma_d=4.0, reverse_pos_pairs=True, use_square=False, in_channel_names=list(range(C)), img_size=[224], num_classes=161)
    model = dcv.dichavit(cfg, mapper={"train": list(range(C))}).cuda().eval()
    for p in model.parameters():
        p.requires_grad_(False)  # the saliency call: nothing but x needs a gradient (the data-only backward)
    x = torch.randn(B, C, 224, 224, device="cuda")
    target = torch.arange(B, device="cuda") % 161
    got = {}

    def relevance():
        got["relevance"] = model.get_attention_relevance(x, target, chunk="train")

    def relevance_last4():
        got["last4"] = model.get_attention_relevance(x, target, chunk="train", start_layer=8)

    def saliency():
        xg = x.detach().requires_grad_(True)
        model(xg, "train", None).gather(1, target.view(-1, 1)).sum().backward()
        got["saliency"] = xg.grad

    def forward():
        with torch.no_grad():
            model(x, "train", None)

    t = _time_alternating({"eval_forward": forward, "saliency": saliency, "relevance": relevance, "relevance_start_layer_8": relevance_last4},
                          max(iters // 3, 5), warmup=2)
    for k in t:
        res[f"{k}_ms"] = round(_median(t[k]) / 1e3, 3)
        res[f"{k}_min_max_ms"] = f"{t[k][0] / 1e3:.3f} .. {t[k][-1] / 1e3:.3f}"
    res["relevance_minus_saliency_ms"] = round((_median(t["relevance"]) - _median(t["saliency"])) / 1e3, 3)
    res["relevance_vs_saliency"] = round(_median(t["relevance"]) / _median(t["saliency"]), 3)
    r = got["relevance"]
    res["relevance_cls_min_max"] = f"{r[:, 0].min().item():.6f} .. {r[:, 0].max().item():.6f}"
    res["relevance_patch_sum_min_max"] = f"{r[:, 1:].sum(-1).min().item():.3e} .. {r[:, 1:].sum(-1).max().item():.3e}"
    res["relevance_finite_and_nonnegative"] = bool(torch.isfinite(r).all() and (r >= 0).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_relevance_bench needs the GPU: a CPU run gives no time")
    res = {}
    gain, spread = kernel(res, a.iters)
    model_times(res, a.iters)
    lines = [f"{k:46s} {v}" for k, v in res.items()] + [json.dumps(res)]
    if gain <= spread:
        lines.append(f"DEFECT: dcv_attn_relevance_step_ps is not faster than dcv_attn_probs_rows_ps + dO V^T and the reduction in torch by more than "
                     f"the latter's spread (gain {gain:.1f} us, spread {spread:.1f} us)")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if gain <= spread:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
