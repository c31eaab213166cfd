"""Times the fused iBOT patch loss (dcv_ibot_loss_fwd + dcv_ibot_loss_bwd) in one process, with events after warm-up, the candidates alternating
inside every round (median of --iters rounds), at (R, K) = (60000, 8192) — two global crops at bs 64 with 30 % of 8 x 196 tokens masked, 8192
prototypes — and (6000, 8192):
  (a) the kernel pair: the forward's three launches (streaming pass with tsum's first level, finish with tsum's second level, row sum) and the
      backward's one;
  (b) the plain fp32 torch restatement, forward and autograd backward: softmax of the centred teacher, log_softmax of the student, product, row
      sum, weighting, the centre's column sum;
  (c) the floor: a device-to-device copy that moves the bytes the plan moves — two reads of S and T, one write of dS: 20 R K bytes (a copy of
      X bytes moves 2 X).
The candidates are timed --repeats times over; the spread of a candidate is the range of its medians.  (a) must be faster than (b) by more than
the larger of the two spreads: the tool prints a line starting with DEFECT and exits with status 1 otherwise.  The ratio to (c) is reported, and
the forward and backward halves of (a) alone.  Peak extra device memory of (a) and (b) is one call's torch.cuda.max_memory_allocated above the
inputs.  Then the mask-token kernels (dcv_mask_tokens_fwd / _bwd) at B 128, C 8, n 196, D 384 with 30 % of the tokens masked.

    python tools/ibot_loss_bench.py [--iters 20] [--repeats 3] [--out profiles/ibot_loss_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dino_loss_bench import _peak_extra, _time_alternating  # noqa: E402

TS, TT = 0.1, 0.04
SHAPES = ((60000, 8192), (6000, 8192))


def shape(res, R, K, iters, repeats):
    from diverse_channel_vit_amd import hip
    g = torch.Generator(device="cuda").manual_seed(R)
    S = 3 * torch.randn(R, K, device="cuda", generator=g)
    T = 3 * torch.randn(R, K, device="cuda", generator=g)
    c = torch.randn(K, device="cuda", generator=g)
    w = (0.05 + torch.rand(R, device="cuda", generator=g)) / R
    one = torch.ones(1, device="cuda")
    hip.ibot_loss_fwd(S, T, c, w, TS, TT, torch.empty(1, device="cuda"), None, None, torch.empty(K, device="cuda"))  # grows the stream's workspace first
    nbytes = 20.0 * R * K
    src = torch.empty(int(nbytes // 8), dtype=torch.float32, device="cuda")  # reads and writes nbytes / 2 each
    dst = torch.empty_like(src)
    keep = {}

    def fwd():
        loss, tsum = torch.empty(1, device="cuda"), torch.empty(K, device="cuda")
        ss, tstat = torch.empty(R, 3, device="cuda"), torch.empty(R, 4, device="cuda")
        hip.ibot_loss_fwd(S, T, c, w, TS, TT, loss, ss, tstat, tsum)
        keep["k"] = (loss, tsum, ss, tstat)

    def bwd():
        dS = torch.empty_like(S)
        hip.ibot_loss_bwd(S, T, c, w, TS, TT, keep["k"][2], keep["k"][3], one, dS)
        keep["dS"] = dS

    def kernel():
        fwd()
        bwd()

    def restatement():
        s = S.detach().requires_grad_(True)
        q = torch.softmax((T - c) / TT, dim=-1)
        logp = torch.log_softmax(s / TS, dim=-1)
        loss = (w * torch.sum(-q * logp, dim=-1)).sum()
        loss.backward()
        keep["t"] = (loss.detach(), T.sum(0), s.grad)

    fwd()
    fns = {"kernel_pair": kernel, "kernel_fwd": fwd, "kernel_bwd": bwd, "torch_restatement": restatement, "copy_plan_bytes": lambda: dst.copy_(src)}
    runs = [_time_alternating(fns, iters) for _ in range(repeats)]
    kernel()
    restatement()
    torch.cuda.synchronize()
    tag = f"R{R}"
    med = {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in fns}
    spread = {k: max(r[k] for r in runs) - min(r[k] for r in runs) for k in fns}
    res[f"{tag}_shape"] = f"R{R} K{K}"
    res[f"{tag}_plan"] = hip.ibot_loss_plan(R, K)
    res[f"{tag}_ws_floats"] = hip.ibot_loss_ws_floats(R, K)
    res[f"{tag}_plan_bytes"] = int(nbytes)
    for k in fns:
        res[f"{tag}_{k}_us"] = round(med[k], 2)
        res[f"{tag}_{k}_us_runs"] = [round(r[k], 2) for r in runs]
        res[f"{tag}_{k}_spread_us"] = round(spread[k], 2)
    res[f"{tag}_kernel_pair_TBps"] = round(nbytes / (med["kernel_pair"] * 1e-6) / 1e12, 3)
    res[f"{tag}_kernel_vs_restatement"] = round(med["kernel_pair"] / med["torch_restatement"], 4)
    res[f"{tag}_kernel_vs_copy_floor"] = round(med["kernel_pair"] / med["copy_plan_bytes"], 3)
    res[f"{tag}_loss_kernel"] = keep["k"][0].item()
    res[f"{tag}_loss_restatement"] = keep["t"][0].item()
    res[f"{tag}_max_abs_diff_dS"] = (keep["dS"] - keep["t"][2]).abs().max().item()
    res[f"{tag}_max_abs_diff_tsum"] = (keep["k"][1] - keep["t"][1]).abs().max().item()
    keep.clear()
    res[f"{tag}_kernel_pair_peak_extra_MiB"] = round(_peak_extra(kernel) / 2 ** 20, 1)  # dS itself (R K floats) and the statistics; the workspace is the stream's
    keep.clear()
    res[f"{tag}_torch_restatement_peak_extra_MiB"] = round(_peak_extra(restatement) / 2 ** 20, 1)
    keep.clear()
    return med["torch_restatement"] - med["kernel_pair"] > max(spread["kernel_pair"], spread["torch_restatement"])


def mask_kernels(res, iters, repeats, B=128, C=8, n=196, D=384):
    from diverse_channel_vit_amd import hip
    g = torch.Generator(device="cuda").manual_seed(1)
    T = C * n
    xs = torch.randn(B, 1 + T, D, device="cuda", generator=g)
    dx = torch.randn(B, 1 + T, D, device="cuda", generator=g)
    mt, E, pos = torch.randn(D, device="cuda", generator=g), torch.randn(C, D, device="cuda", generator=g), torch.randn(1 + n, D, device="cuda", generator=g)
    mask = (torch.rand(B, T, device="cuda", generator=g) < 0.3).to(torch.uint8)
    dYl = torch.randn(B * T, D, device="cuda", generator=g)
    dYb = torch.empty(B * T, D, dtype=torch.bfloat16, device="cuda")
    dmt = torch.zeros(D, device="cuda")
    fns = {"mask_tokens_fwd": lambda: hip.mask_tokens_fwd(xs, mask, mt, E, pos, B, C, n, D),
           "mask_tokens_bwd": lambda: hip.mask_tokens_bwd(dx, mask, dYl, dYb, dmt, B, C, n, D),
           "mask_tokens_bwd_no_ortho": lambda: hip.mask_tokens_bwd(dx, mask, None, dYb, dmt, B, C, n, D)}
    runs = [_time_alternating(fns, iters) for _ in range(repeats)]
    res["mask_shape"] = f"B{B} C{C} n{n} D{D}, {int(mask.sum())} of {B * T} tokens masked"
    for k in fns:
        res[f"{k}_us"] = round(sorted(r[k] for r in runs)[len(runs) // 2], 2)
        res[f"{k}_us_runs"] = [round(r[k], 2) for r in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ibot_loss_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ibot_loss_bench needs the GPU: a CPU run gives no time")
    res, ok = {}, {}
    for R, K in SHAPES:
        ok[R] = shape(res, R, K, a.iters, a.repeats)
        torch.cuda.empty_cache()
    mask_kernels(res, a.iters, a.repeats)
    lines = [f"{k:44s} {v}" for k, v in res.items()] + [json.dumps(res)]
    slow = [v for v in ok if not ok[v]]
    if slow:
        lines.append(f"DEFECT: the iBOT loss kernel pair is not faster than the torch restatement by more than the spread at R = {slow}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(f"# tools/ibot_loss_bench.py --iters {a.iters} --repeats {a.repeats}: medians of {a.iters} launches, candidates alternating, "
                f"{a.repeats} repeats (spread = range of a candidate's medians)\n" + text)
    if slow:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
