"""Times the fused DINO loss (dcv_dino_loss_fwd + dcv_dino_loss_bwd) in one process, with events after warm-up, the candidates alternating inside
every round (median of --iters rounds), at (V, B, K) = (10, 64, 65536) — 65 536 prototypes, 2 global + 8 local crops, bs 64 — and (2, 64, 65536):
  (a) the kernel pair: the forward's three launches (streaming pass, finish with tsum, row sum) and the backward's one;
  (b) the plain fp32 torch restatement, forward and autograd backward: softmax of the centred teacher, log_softmax of the student, the loop over
      teacher view and student views, the centre's column sum;
  (c) the floor: a device-to-device copy that moves the bytes the plan moves — forward S, T twice (tsum re-reads it) and the centre, backward S, T,
      the centre and dS: 4 K (B (3 V + 6) + 2) bytes (a copy of X bytes moves 2 X).
The three are timed --repeats times over; the spread of a candidate is the range of its medians.  (a) must be faster than (b) by more than the
larger of the two spreads: the tool prints a line starting with DEFECT and exits with status 1 otherwise.  The ratio to (c) is reported, and the
forward and backward halves of (a) alone.  Peak extra device memory of (a) and (b) is one call's torch.cuda.max_memory_allocated above the inputs.

    python tools/dino_loss_bench.py [--iters 50] [--repeats 3] [--out profiles/dino_loss_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

TS, TT = 0.1, 0.04
SHAPES = ((10, 64, 65536), (2, 64, 65536))


def _time_alternating(fns, iters, warmup=3):
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


def _peak_extra(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def shape(res, V, B, K, iters, repeats):
    from diverse_channel_vit_amd import hip
    g = torch.Generator(device="cuda").manual_seed(V)
    S = 3 * torch.randn(V * B, K, device="cuda", generator=g)
    T = 3 * torch.randn(2 * B, K, device="cuda", generator=g)
    c = torch.randn(K, device="cuda", generator=g)
    one = torch.ones(1, device="cuda")
    hip.dino_loss_fwd(S, T, c, V, TS, TT, torch.empty(1, device="cuda"), None, None, None)  # grows the stream's workspace before anything is measured
    nbytes = 4.0 * K * (B * (3 * V + 6) + 2)
    src = torch.empty(int(nbytes // 8), dtype=torch.float32, device="cuda")  # reads and writes nbytes / 2 each
    dst = torch.empty_like(src)
    keep = {}

    def fwd():
        loss, tsum = torch.empty(1, device="cuda"), torch.empty(K, device="cuda")
        ss, tstat = torch.empty(V * B, 2, device="cuda"), torch.empty(2 * B, 3, device="cuda")
        hip.dino_loss_fwd(S, T, c, V, TS, TT, loss, ss, tstat, tsum)
        keep["k"] = (loss, tsum, ss, tstat)

    def bwd():
        dS = torch.empty_like(S)
        hip.dino_loss_bwd(S, T, c, V, TS, TT, keep["k"][2], keep["k"][3], one, dS)
        keep["dS"] = dS

    def kernel():
        fwd()
        bwd()

    def restatement():
        s = S.detach().requires_grad_(True)
        q = torch.softmax((T - c) / TT, dim=-1).view(2, B, K)
        logp = torch.log_softmax(s / TS, dim=-1).view(V, B, K)
        total, terms = 0, 0
        for iq in range(2):
            for v in range(V):
                if v != iq:
                    total = total + torch.sum(-q[iq] * logp[v], dim=-1).mean()
                    terms += 1
        loss = total / terms
        loss.backward()
        keep["t"] = (loss.detach(), T.sum(0), s.grad)

    fwd()
    fns = {"kernel_pair": kernel, "kernel_fwd": fwd, "kernel_bwd": bwd, "torch_restatement": restatement, "copy_plan_bytes": lambda: dst.copy_(src)}
    runs = [_time_alternating(fns, iters) for _ in range(repeats)]
    kernel()
    restatement()
    torch.cuda.synchronize()
    tag = f"V{V}"
    med = {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in fns}
    spread = {k: max(r[k] for r in runs) - min(r[k] for r in runs) for k in fns}
    res[f"{tag}_shape"] = f"V{V} B{B} K{K}"
    res[f"{tag}_plan"] = hip.dino_loss_plan(V, B, K)
    res[f"{tag}_ws_floats"] = hip.dino_loss_ws_floats(V, B, K)
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
    res[f"{tag}_kernel_pair_peak_extra_MiB"] = round(_peak_extra(kernel) / 2 ** 20, 1)  # dS itself (V B K floats) and the statistics
    keep.clear()
    res[f"{tag}_torch_restatement_peak_extra_MiB"] = round(_peak_extra(restatement) / 2 ** 20, 1)
    keep.clear()
    return med["torch_restatement"] - med["kernel_pair"] > max(spread["kernel_pair"], spread["torch_restatement"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dino_loss_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dino_loss_bench needs the GPU: a CPU run gives no time")
    res, ok = {}, {}
    for V, B, K in SHAPES:
        ok[V] = shape(res, V, B, K, a.iters, a.repeats)
        torch.cuda.empty_cache()
    lines = [f"{k:44s} {v}" for k, v in res.items()] + [json.dumps(res)]
    slow = [v for v in ok if not ok[v]]
    if slow:
        lines.append(f"DEFECT: the DINO loss kernel pair is not faster than the torch restatement by more than the spread at V = {slow}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(f"# tools/dino_loss_bench.py --iters {a.iters} --repeats {a.repeats}: medians of {a.iters} launches, candidates alternating, "
                f"{a.repeats} repeats (spread = range of a candidate's medians)\n" + text)
    if slow:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
