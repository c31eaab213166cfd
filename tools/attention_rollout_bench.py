"""Times the rollout-step attention kernel (dcv_attn_rollout_step_ps) and what surrounds it, in one process, with device events after warm-up,
the candidates alternating inside every round (median of --iters rounds), at the headline shape B 64, H 6, C 8, n_p 196 (N 1569), pre-scaled q:
  (a) the kernel: one rollout step, out [B,N] from w [B,N];
  (b) what it replaces, from kernels that exist without it: dcv_attn_probs_rows_ps into a [B,H,N,N] buffer (3.78 GB), then the head mean and
      torch.einsum("bq,bqk->bk") of that map;
  (c) the yardstick: dcv_attn_channel_mass_ps, token masses alone, on the same qkv — the same Q K^T and exp2 work, reduced along the other axis.
(a) must be faster than (b) by more than (b)'s own spread over the run (max - min of its rounds).  How (a) stands against (c) is recorded, not
required.  Then whole calls on DiChaViT-S at the headline config (8 channels, 224 x 224, patch 16, bs 64): get_attention_rollout() against one
eval forward and against the route it replaces — twelve get_last_selfattention calls, the head mean and the vector-matrix product in torch, last
block first — which it must beat as well.  The tool prints a line starting with DEFECT and exits with status 1 otherwise.

    python tools/attention_rollout_bench.py [--iters 30] [--out FILE]
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
N = 1 + C * N_P
SCALE = 64 ** -0.5
ALPHA = 0.5
B_EVEN = 59


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
    w = torch.rand(B, N, device="cuda", generator=g)
    w /= w.sum(-1, keepdim=True)
    e0 = torch.zeros(B, N, device="cuda")
    e0[:, 0] = 1.0
    out, out0, out1 = (torch.empty(B, N, device="cuda") for _ in range(3))
    P = torch.empty(B, H, N, N, device="cuda")
    Pm = torch.empty(B, N, N, device="cuda")
    tok = torch.empty(B, H, N, 1 + C, device="cuda")
    got = {}

    def replaced():
        hip.attn_probs(qkv, lse, P, B, N, H, 64, SCALE, prescaled=True)
        torch.mean(P, dim=1, out=Pm)
        got["r"] = torch.einsum("bq,bqk->bk", w, Pm)

    t = _time_alternating({
        "rollout_step": lambda: hip.attn_rollout_step(qkv, lse, w, out, B, N, H, 64, SCALE, ALPHA, prescaled=True),
        "rollout_step_onehot": lambda: hip.attn_rollout_step(qkv, lse, e0, out0, B, N, H, 64, SCALE, ALPHA, prescaled=True),
        "probs_mean_einsum": replaced,
        "probs_alone": lambda: hip.attn_probs(qkv, lse, P, B, N, H, 64, SCALE, prescaled=True),
        "channel_mass_tok": lambda: hip.attn_channel_mass(qkv, lse, B, N, H, 64, SCALE, C, N_P, tok=tok, prescaled=True),
        # the first B_EVEN images alone: 13 B_EVEN = 767 workgroups of the rollout kernel, one short of three per CU, against 3.25 per CU at B 64
        "rollout_step_b_even": lambda: hip.attn_rollout_step(qkv, lse, w, out1, B_EVEN, N, H, 64, SCALE, ALPHA, prescaled=True),
        "channel_mass_tok_b_even": lambda: hip.attn_channel_mass(qkv, lse, B_EVEN, N, H, 64, SCALE, C, N_P, tok=tok, prescaled=True)}, iters)
    replaced()
    torch.cuda.synchronize()
    res["shape"] = f"B{B} H{H} C{C} n_p{N_P} N{N} pre-scaled q"
    res["rounds"] = iters
    res["qk_gflop"] = round(2.0 * B * H * N * N * 64 / 1e9, 1)
    res["probs_map_bytes"] = 4 * B * H * N * N
    res["workgroups"] = B * ((N + 127) // 128)
    for k, v in t.items():
        res[f"{k}_us"] = round(_median(v), 1)
        res[f"{k}_min_max_us"] = f"{v[0]:.1f} .. {v[-1]:.1f}"
    spread = t["probs_mean_einsum"][-1] - t["probs_mean_einsum"][0]
    res["probs_mean_einsum_spread_us"] = round(spread, 1)
    res["rollout_step_vs_probs_mean_einsum"] = round(_median(t["rollout_step"]) / _median(t["probs_mean_einsum"]), 4)
    res["rollout_step_vs_channel_mass_tok"] = round(_median(t["rollout_step"]) / _median(t["channel_mass_tok"]), 3)
    res["b_even"] = B_EVEN
    res["rollout_step_vs_channel_mass_tok_b_even"] = round(_median(t["rollout_step_b_even"]) / _median(t["channel_mass_tok_b_even"]), 3)
    res["rollout_step_TFLOPs"] = round(2.0 * B * H * N * N * 64 / (_median(t["rollout_step"]) * 1e-6) / 1e12, 1)
    ref = ALPHA * w + (1 - ALPHA) * got["r"]
    res["max_rel_diff_to_replaced"] = ((out - ref).abs() / ref).max().item()
    return _median(t["probs_mean_einsum"]) - _median(t["rollout_step"]), spread


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
    got = {}

    def rollout():
        got["rollout"] = fe.get_attention_rollout(x, chunk="train")

    def twelve_calls():
        r = torch.zeros(B, N, device="cuda")
        r[:, 0] = 1.0
        for li in range(11, -1, -1):  # the last block first
            A = fe.get_last_selfattention(x, chunk="train", layer_idx=li).mean(1)
            r = ALPHA * r + (1 - ALPHA) * torch.einsum("bq,bqk->bk", r, A)
            del A
        got["twelve"] = r

    with torch.no_grad():
        t = _time_alternating({"eval_forward": lambda: model(x, "train", None), "rollout": rollout, "twelve_calls": twelve_calls},
                              max(iters // 6, 5), warmup=2)
    res["eval_forward_ms"] = round(_median(t["eval_forward"]) / 1e3, 3)
    res["get_attention_rollout_ms"] = round(_median(t["rollout"]) / 1e3, 3)
    res["get_attention_rollout_min_max_ms"] = f"{t['rollout'][0] / 1e3:.3f} .. {t['rollout'][-1] / 1e3:.3f}"
    res["twelve_get_last_selfattention_plus_torch_ms"] = round(_median(t["twelve_calls"]) / 1e3, 3)
    res["twelve_calls_min_max_ms"] = f"{t['twelve_calls'][0] / 1e3:.3f} .. {t['twelve_calls'][-1] / 1e3:.3f}"
    res["rollout_vs_eval_forward"] = round(_median(t["rollout"]) / _median(t["eval_forward"]), 3)
    res["rollout_vs_twelve_calls"] = round(_median(t["rollout"]) / _median(t["twelve_calls"]), 4)
    res["rollout_row_sum_min_max"] = f"{got['rollout'].sum(-1).min().item():.7f} .. {got['rollout'].sum(-1).max().item():.7f}"
    res["max_rel_diff_rollout_to_twelve_calls"] = ((got["rollout"] - got["twelve"]).abs() / got["twelve"]).max().item()
    return _median(t["twelve_calls"]) - _median(t["rollout"]), t["twelve_calls"][-1] - t["twelve_calls"][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_rollout_bench needs the GPU: a CPU run gives no time")
    res = {}
    gain, spread = kernel(res, a.iters)
    mgain, mspread = model_times(res, a.iters)
    lines = [f"{k:46s} {v}" for k, v in res.items()] + [json.dumps(res)]
    if gain <= spread:
        lines.append(f"DEFECT: dcv_attn_rollout_step_ps is not faster than dcv_attn_probs_rows_ps + the torch reduction by more than the latter's "
                     f"spread (gain {gain:.1f} us, spread {spread:.1f} us)")
    if mgain <= mspread:
        lines.append(f"DEFECT: get_attention_rollout is not faster than twelve get_last_selfattention calls + torch by more than the latter's "
                     f"spread (gain {mgain / 1e3:.3f} ms, spread {mspread / 1e3:.3f} ms)")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if gain <= spread or mgain <= mspread:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
