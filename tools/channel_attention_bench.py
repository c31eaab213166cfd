"""Times the channel-mass attention kernel (dcv_attn_channel_mass_ps) and what surrounds it, in one process, with device events after warm-up,
the candidates alternating inside every round (median of --iters rounds), at the headline shape B 64, H 6, C 8, n_p 196 (N 1569), pre-scaled q:
  (a) the kernel: the token masses alone (tok [B,H,N,1+C]), the channel matrix alone (ch [B,H,1+C,1+C], token masses through the workspace),
      and both together;
  (b) what it replaces, from kernels that exist without it: dcv_attn_probs_rows_ps into a [B,H,N,N] buffer (3.78 GB), then the torch reduction
      of that map to the channel matrix (key segments summed, query segments averaged) into preallocated outputs;
  (c) the yardstick: dcv_attn_fwd_rows_ps on the same qkv — the forward shares the Q K^T half and the exp2 per score and adds P V.
(a) must be faster than (b) by more than (b)'s own spread over the run (max - min of its rounds): the tool prints a line starting with DEFECT
and exits with status 1 otherwise.  No absolute time is required.  Then whole calls on DiChaViT-S at the headline config (8 channels, 224 x 224,
patch 16, bs 64): get_channel_attention(n=12), both query forms, against one eval forward.

    python tools/channel_attention_bench.py [--iters 30] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, H, C, N_P = 64, 6, 8, 196
N, W = 1 + C * N_P, 1 + C
SCALE = 64 ** -0.5


def _time_alternating(fns, iters, warmup=3):
    """{name: fn} -> {name: sorted us per round}; one call of each per round, so drift in clocks or neighbours hits every candidate alike."""
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
    return {k: sorted(v) for k, v in ts.items()}


def _median(v):
    return v[len(v) // 2]


def kernel(res, iters):
    from diverse_channel_vit_amd import hip
    D = H * 64
    g = torch.Generator(device="cuda").manual_seed(8)
    qkv = torch.randn(B, N, 3 * D, device="cuda", generator=g) * 1.5
    qkv[..., :D] *= SCALE * math.log2(math.e)  # the pre-scaled q the model's operand copies deliver
    qkv = qkv.to(torch.bfloat16)
    o = torch.empty(B, N, D, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, N, device="cuda")
    hip.attn_fwd(qkv, o, lse, B, N, H, 64, SCALE, prescaled=True)
    tok, ch = torch.empty(B, H, N, W, device="cuda"), torch.empty(B, H, W, W, device="cuda")
    tok1, ch1 = torch.empty_like(tok), torch.empty_like(ch)
    P = torch.empty(B, H, N, N, device="cuda")
    Tt, At = torch.empty(B, H, N, W, device="cuda"), torch.empty(B, H, W, W, device="cuda")
    o2, lse2 = torch.empty_like(o), torch.empty_like(lse)

    def replaced():
        hip.attn_probs(qkv, lse, P, B, N, H, 64, SCALE, prescaled=True)
        Tt[..., 0] = P[..., 0]
        torch.sum(P[..., 1:].unflatten(-1, (C, N_P)), dim=-1, out=Tt[..., 1:])
        At[:, :, 0] = Tt[:, :, 0]
        torch.mean(Tt[:, :, 1:].unflatten(2, (C, N_P)), dim=3, out=At[:, :, 1:])

    t = _time_alternating({
        "both": lambda: hip.attn_channel_mass(qkv, lse, B, N, H, 64, SCALE, C, N_P, tok=tok, ch=ch, prescaled=True),
        "tok_alone": lambda: hip.attn_channel_mass(qkv, lse, B, N, H, 64, SCALE, C, N_P, tok=tok1, prescaled=True),
        "ch_alone": lambda: hip.attn_channel_mass(qkv, lse, B, N, H, 64, SCALE, C, N_P, ch=ch1, prescaled=True),
        "probs_then_torch": replaced,
        "probs_alone": lambda: hip.attn_probs(qkv, lse, P, B, N, H, 64, SCALE, prescaled=True),
        "attn_fwd": lambda: hip.attn_fwd(qkv, o2, lse2, B, N, H, 64, SCALE, prescaled=True)}, iters)
    replaced()
    torch.cuda.synchronize()
    res["shape"] = f"B{B} H{H} C{C} n_p{N_P} N{N} pre-scaled q"
    res["rounds"] = iters
    res["qk_gflop"] = round(2.0 * B * H * N * N * 64 / 1e9, 1)
    res["probs_map_bytes"] = 4 * B * H * N * N
    res["ws_floats"] = int(hip.load().dcv_attn_channel_mass_ws_floats(B, N, H, C))
    for k, v in t.items():
        res[f"{k}_us"] = round(_median(v), 1)
        res[f"{k}_min_max_us"] = f"{v[0]:.1f} .. {v[-1]:.1f}"
    spread = t["probs_then_torch"][-1] - t["probs_then_torch"][0]
    res["probs_then_torch_spread_us"] = round(spread, 1)
    res["both_vs_probs_then_torch"] = round(_median(t["both"]) / _median(t["probs_then_torch"]), 4)
    res["both_vs_attn_fwd"] = round(_median(t["both"]) / _median(t["attn_fwd"]), 3)
    res["tok_alone_vs_attn_fwd"] = round(_median(t["tok_alone"]) / _median(t["attn_fwd"]), 3)
    res["both_TFLOPs"] = round(2.0 * B * H * N * N * 64 / (_median(t["both"]) * 1e-6) / 1e12, 1)
    res["max_abs_diff_to_replaced_tok"] = (tok - Tt).abs().max().item()
    res["max_abs_diff_to_replaced_ch"] = (ch - At).abs().max().item()
    res["alone_equals_both_bitwise"] = bool(torch.equal(tok, tok1) and torch.equal(ch, ch1))
    slowest_a = max(_median(t[k]) for k in ("both", "tok_alone", "ch_alone"))
    return _median(t["probs_then_torch"]) - slowest_a, spread


def model_times(res, iters):
    import diverse_channel_vit_amd as dcv

    class Cfg(dict):
        __getattr__ = dict.get

    cfg = Cfg(name="dichavit", pretrained_model_name="small", patch_size=16, temperature=0.07, learnable_temp=False, enable_sample=False,
              use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False, block_type="block",
              hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.001, ortho_loss_v1_lambda=0.1, drop_path_rate=0.0, gamma_s=0.5,
              gamma_d=4.0, reverse_pos_pairs=True, use_square=False, in_channel_names=list(range(C)), img_size=[224], num_classes=161)
    model = dcv.dichavit(cfg, mapper={"train": list(range(C))}).cuda().eval()
    fe = model.feature_extractor
    x = torch.randn(B, C, 224, 224, device="cuda")
    with torch.no_grad():
        t = _time_alternating({"eval_forward": lambda: model(x, "train", None),
                               "n12_channel": lambda: fe.get_channel_attention(x, n=12, chunk="train"),
                               "n12_token": lambda: fe.get_channel_attention(x, n=12, chunk="train", queries="token")}, max(iters // 3, 5), warmup=2)
    res["eval_forward_ms"] = round(_median(t["eval_forward"]) / 1e3, 3)
    res["get_channel_attention_n12_channel_ms"] = round(_median(t["n12_channel"]) / 1e3, 3)
    res["get_channel_attention_n12_token_ms"] = round(_median(t["n12_token"]) / 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("channel_attention_bench needs the GPU: a CPU run gives no time")
    res = {}
    gain, spread = kernel(res, a.iters)
    model_times(res, a.iters)
    lines = [f"{k:44s} {v}" for k, v in res.items()] + [json.dumps(res)]
    ok = gain > spread
    if not ok:
        lines.append(f"DEFECT: dcv_attn_channel_mass_ps is not faster than dcv_attn_probs_rows_ps + the torch reduction by more than the latter's "
                     f"spread (gain {gain:.1f} us, spread {spread:.1f} us)")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
