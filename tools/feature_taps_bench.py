"""Times the channel-pool adjoint (dcv_ln_pool_channels_bwd) and the training step that uses it, in one process, with events after warm-up,
the candidates alternating inside every round (median of --iters rounds), at B 64, n_p 196, D 384 with C 8 (the headline shape) and C 3
(CHAMMI-sized):
  (a) the kernel (all its launches: the row pass and the two small dgamma / dbeta sums): reads x once, reads and writes dx once;
  (b) what it replaces, from what exists without it: the broadcast du [B, N, D] of dout / n_p materialised in fp32 by torch, dcv_ln_fwd for
      the row statistics, then dcv_ln_bwd (f32 du) accumulating into dx;
  (c) the floor: a device-to-device copy that moves 3 B N D 4 bytes in total (a copy of X bytes moves 2 X).
The three are timed --repeats times over; the spread of a candidate is the range of its medians.  (a) must be faster than (b) by more than
the larger of the two spreads: the tool prints a line starting with DEFECT and exits with status 1 otherwise.  The ratio to (c) is reported.
Then the eager bs-64 headline step of DiChaViT-S (8 channels, 224 x 224, patch 16: zero_grad, forward, loss, backward, HipAdamW) plain against
the same step through forward_with_features(layers=4, pool="channel") with a linear loss on the four taps.

    python tools/feature_taps_bench.py [--iters 50] [--repeats 3] [--out profiles/feature_taps_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, N_P, D = 64, 196, 384


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


def kernel(res, C, iters, repeats):
    from diverse_channel_vit_amd import hip
    N = 1 + C * N_P
    M = B * N
    g = torch.Generator(device="cuda").manual_seed(C)
    x = torch.randn(B, N, D, device="cuda", generator=g) * 2.0 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(D, device="cuda", generator=g), torch.zeros(D, device="cuda")
    dout = torch.randn(B, 1 + C, D, device="cuda", generator=g) * N_P
    dx_a, dx_b = torch.zeros(B, N, D, device="cuda"), torch.zeros(B, N, D, device="cuda")
    dg_a, db_a, dg_b, db_b = (torch.zeros(D, device="cuda") for _ in range(4))
    du = torch.empty(B, N, D, device="cuda")
    mean, rstd, scratch = torch.empty(M, device="cuda"), torch.empty(M, device="cuda"), torch.empty(M, D, dtype=torch.bfloat16, device="cuda")
    nbytes = 3 * 4.0 * B * N * D
    src = torch.empty(int(nbytes // 8), dtype=torch.float32, device="cuda")  # reads and writes nbytes / 2 each
    dst = torch.empty_like(src)

    def composite():
        du[:, 0] = dout[:, 0]
        du[:, 1:].view(B, C, N_P, D).copy_((dout[:, 1:] / N_P).unsqueeze(2).expand(B, C, N_P, D))
        hip.ln_fwd(x, gamma, beta, scratch, mean, rstd, M, D, 1e-6)
        hip.ln_bwd(du.view(M, D), x, mean, rstd, gamma, dx_b.view(M, D), dx_b.view(M, D), None, dg_b, db_b, M, D)

    fns = {"kernel": lambda: hip.ln_pool_channels_bwd(x, gamma, dout, dx_a, dg_a, db_a, B, C, N_P, D, 1e-6), "composite": composite,
           "copy_3BND4_bytes": lambda: dst.copy_(src)}
    runs = [_time_alternating(fns, iters) for _ in range(repeats)]
    # one call of each from equal starts: the two must agree
    for t in (dx_a, dx_b, dg_a, dg_b, db_a, db_b):
        t.zero_()
    fns["kernel"]()
    composite()
    tag = f"C{C}"
    med = {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in fns}
    spread = {k: max(r[k] for r in runs) - min(r[k] for r in runs) for k in fns}
    res[f"{tag}_shape"] = f"B{B} C{C} n_p{N_P} D{D}"
    res[f"{tag}_ws_floats"] = int(hip.load().dcv_ln_pool_channels_bwd_ws_floats(B, C, N_P, D))
    for k in fns:
        res[f"{tag}_{k}_us"] = round(med[k], 2)
        res[f"{tag}_{k}_us_runs"] = [round(r[k], 2) for r in runs]
        res[f"{tag}_{k}_spread_us"] = round(spread[k], 2)
    res[f"{tag}_kernel_TBps"] = round(nbytes / (med["kernel"] * 1e-6) / 1e12, 3)
    res[f"{tag}_kernel_vs_composite"] = round(med["kernel"] / med["composite"], 3)
    res[f"{tag}_kernel_vs_copy_floor"] = round(med["kernel"] / med["copy_3BND4_bytes"], 3)
    res[f"{tag}_gap_us"] = round(med["composite"] - med["kernel"], 2)
    res[f"{tag}_max_abs_diff_dx"] = (dx_a - dx_b).abs().max().item()
    res[f"{tag}_max_abs_diff_dgamma_over_max"] = ((dg_a - dg_b).abs().max() / dg_b.abs().max()).item()
    return med["composite"] - med["kernel"] > max(spread["kernel"], spread["composite"])


def step_times(res, iters):
    import diverse_channel_vit_amd as dcv

    class Cfg(dict):
        __getattr__ = dict.get

    C = 8
    cfg = Cfg(name="dichavit", pretrained_model_name="small", patch_size=16, temperature=0.07, learnable_temp=False, enable_sample=False,
              use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False, block_type="block",
              hcs_sampling="none", hcs_sampling_temp=0.1, proxy_loss_lambda=0.001, ortho_loss_v1_lambda=0.1, drop_path_rate=0.0, gamma_s=0.5,
              gamma_d=4.0, reverse_pos_pairs=True, use_square=False, in_channel_names=list(range(C)), img_size=[224], num_classes=161)
    torch.manual_seed(0)
    model = dcv.dichavit(cfg, mapper={"train": list(range(C))}).cuda().train()
    opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=4.9e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.04, model=model)
    x = torch.randn(B, C, 224, 224, device="cuda")
    y = torch.randint(0, 161, (B,), device="cuda")
    W = [torch.randn(B, 1 + C, D, device="cuda") * 1e-3 for _ in range(4)]
    ce = torch.nn.CrossEntropyLoss()

    def plain():
        opt.zero_grad()
        out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        (ce(out, y) + extra).backward()
        opt.step()

    def tapped():
        opt.zero_grad()
        (out, extra), feats = model.forward_with_features(x, "train", None, layers=4, pool="channel", cur_epoch=0)
        (ce(out, y) + extra + sum((w * f).sum() for w, f in zip(W, feats))).backward()
        opt.step()

    t = _time_alternating({"plain": plain, "tapped": tapped}, max(iters // 3, 5), warmup=3)
    res["step_plain_ms"] = round(t["plain"] / 1e3, 3)
    res["step_layers4_channel_taps_ms"] = round(t["tapped"] / 1e3, 3)
    res["step_taps_cost_ms"] = round((t["tapped"] - t["plain"]) / 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_taps_bench.txt"))
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_taps_bench needs the GPU: a CPU run gives no time")
    res, ok = {}, {}
    for C in (8, 3):
        ok[C] = kernel(res, C, a.iters, a.repeats)
    if not a.kernel_only:
        step_times(res, a.iters)
    lines = [f"{k:44s} {v}" for k, v in res.items()] + [json.dumps(res)]
    slow = [c for c in (8, 3) if not ok[c]]
    if slow:
        lines.append(f"DEFECT: dcv_ln_pool_channels_bwd is not faster than the composite by more than the spread at C = {slow}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(f"# tools/feature_taps_bench.py --iters {a.iters} --repeats {a.repeats}: medians of {a.iters} launches, candidates alternating, "
                f"{a.repeats} repeats (spread = range of a candidate's medians)\n" + text)
    if slow:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
