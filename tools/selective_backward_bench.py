"""Measurements of the selective backward on one MI355X, DiChaViT-S at the headline config (8 channels, 224 x 224, patch 16, bs 64).

Kernel: dcv_bias_grad at the workload's M = 100 416 token rows for P = 384, 1152 and 1536 against a device-to-device copy that moves the same
bytes (a copy of M P bytes reads M P and writes M P: the 2 M P bytes the kernel reads), in one process, candidates alternating inside every
round, medians of --iters rounds after warm-up.  Every candidate rotates over enough buffers that no launch finds its input in the Infinity
Cache (256 MB) from the launch before.

Step: forward + backward + HipAdamW.step under every set_trainable() preset, against the full step (twice per round: its spread is the
yardstick) and against the data-only call (every parameter frozen, x asks: forward + backward, no optimiser), configurations alternating
over --rounds rounds.  Every preset's step must be faster than the full step by more than the full step's spread: otherwise a line starting
with DEFECT is printed and the exit status is 1.

--ab PARENT: bench.py --steps 20 --warmup 5 --dump-outputs in PARENT (a built checkout of the parent commit) and in this tree, alternating,
two runs each; the dumps are compared byte for byte.

    python tools/selective_backward_bench.py [--iters 50] [--rounds 3] [--out profiles/selective_backward_bench.txt]
                                             [--ab PARENT --ab-out profiles/selective_backward_bench_ab.txt]
"""
import argparse
import filecmp
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, C, M_HEADLINE = 64, 8, 100416
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


class Cfg(dict):
    __getattr__ = dict.get


def make_model():
    import diverse_channel_vit_amd as dcv
    cfg = Cfg(name="dichavit", pretrained_model_name="small", patch_size=16, temperature=0.07, learnable_temp=False, enable_sample=False,
              use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none", freeze_channel_emb=False, block_type="block",
              hcs_sampling="none", hcs_sampling_temp=1000.0, proxy_loss_lambda=0.001, ortho_loss_v1_lambda=0.001, drop_path_rate=0.0, gamma_s=1.0,
              gamma_d=4.0, reverse_pos_pairs=True, use_square=False, new_channel_inits=["zero"], in_channel_names=[f"c{i}" for i in range(C)],
              img_size=[224], num_classes=161)
    torch.manual_seed(0)
    return dcv.dichavit(cfg, mapper={"train": list(range(C))}).cuda().train()


def time_alternating(fns, iters, warmup=5):
    """{name: fn} -> {name: median us}; one call of each per round, so drift in clocks or neighbours hits every candidate alike."""
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


def kernel_part(iters):
    from diverse_channel_vit_amd import hip
    hip.load()
    dev = "cuda"
    M = M_HEADLINE
    if os.environ.get("DCV_LIB"):
        say(f"library: {os.path.basename(os.environ['DCV_LIB'])} (a build_variant of the same sources)")
    say(f"kernel: dcv_bias_grad (the streaming launch and its det_reduce) at M = {M} rows against a device-to-device copy moving the same bytes; "
        f"medians of {iters} alternating launches, every candidate rotating over buffers of more than 256 MB in all")
    say(f"  {'P':>5s} {'MB read':>8s} {'bias_grad us':>13s} {'TB/s':>6s} {'copy us':>8s} {'TB/s':>6s} {'vs copy':>8s} {'plan: col chunks x row wgs, passes':>36s}")
    import ctypes as Ct
    for P in (384, 1152, 1536):
        nbytes = 2.0 * M * P
        nbuf = int(2 * (256 << 20) // nbytes) + 2
        Ys = [(torch.randn(M, P, device=dev)).to(torch.bfloat16) for _ in range(nbuf)]
        src = [torch.empty(M * P, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        dst = [torch.empty(M * P, dtype=torch.uint8, device=dev) for _ in range(2)]
        db = torch.zeros(P, device=dev)
        it = [0, 0]

        def bias():
            it[0] += 1
            hip.bias_grad(Ys[it[0] % nbuf], db)

        def copy():
            it[1] += 1
            dst[it[1] % 2].copy_(src[it[1] % nbuf])

        t = time_alternating({"bias_grad": bias, "copy": copy}, iters)
        got = [Ct.c_int() for _ in range(5)]
        hip.load().dcv_bias_grad_plan(M, P, *[Ct.byref(g) for g in got])
        plan = f"{got[0].value} x {got[3].value}, {got[4].value}"
        say(f"  {P:5d} {nbytes / 1e6:8.1f} {t['bias_grad']:13.1f} {nbytes / (t['bias_grad'] * 1e-6) / 1e12:6.2f} {t['copy']:8.1f} "
            f"{nbytes / (t['copy'] * 1e-6) / 1e12:6.2f} {t['bias_grad'] / t['copy']:8.2f} {plan:>36s}")
        del Ys, src, dst


PRESETS = (("bias",), ("norm",), ("channel_embed",), ("tokeniser",), ("head",), ("head", "norm"))


def step_part(model, rounds, steps=10):
    import diverse_channel_vit_amd as dcv
    x = torch.randn(B, C, 224, 224, device="cuda")
    xg = x.clone().requires_grad_(True)
    y = torch.randint(0, 161, (B,), device="cuda")
    ce = torch.nn.CrossEntropyLoss()
    configs = [("full a", ("all",)), ("full b", ("all",))] + [("+".join(s), s) for s in PRESETS] + [("data-only call", None)]
    opts = {}

    def setup(name, specs):
        if specs is None:
            for p in model.parameters():
                p.requires_grad_(False)
            return None
        model.set_trainable(*specs)
        if name not in opts:
            opts[name] = dcv.HipAdamW(dcv.param_groups(model, 4.9e-5, 0.04), model=model)
        return opts[name]

    def one(opt):
        model.zero_grad(set_to_none=True)  # not opt.zero_grad(): a parameter frozen now may hold a gradient of the configuration before
        xin = x
        if opt is None:
            xin, xg.grad = xg, None
        out, extra = model(xin, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        (ce(out, y) + extra).backward()
        if opt is not None:
            opt.step()

    def timed(opt):
        for _ in range(3):
            one(opt)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ts = []
        for _ in range(steps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            one(opt)
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e))
        return sorted(ts)[len(ts) // 2], torch.cuda.max_memory_allocated() / 2 ** 30

    res = {name: [] for name, _ in configs}
    mem, launches = {}, {}
    for _ in range(rounds):
        for name, specs in configs:
            ms, gb = timed(setup(name, specs))
            res[name].append(ms)
            mem[name] = gb
    # what each configuration launches for the weight gradients, from the profiler's records of one step
    from diverse_channel_vit_amd import hip
    for name, specs in configs:
        opt = setup(name, specs)
        hip.set_profiler(True)
        one(opt)
        torch.cuda.synchronize()
        rec = hip.set_profiler(False)
        cnt = {"tn": 0, "group": 0, "bias": 0}
        for (sym, _), r in rec.items():
            key = "group" if sym == "gemm_tn384_group_kernel" else "tn" if sym.startswith("gemm_tn") else "bias" if sym == "bias_grad_kernel" else None
            if key:
                cnt[key] += len(r["ev"])
        launches[name] = f"{cnt['group']:3d} grouped {cnt['tn']:3d} single {cnt['bias']:3d} bias sums"
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    full = res["full a"] + res["full b"]
    spread = max(full) - min(full)
    base = sorted(full)[len(full) // 2]
    say()
    say(f"step: forward + backward + HipAdamW.step (the data-only call: forward + backward) at bs {B}, {C} channels, 224 x 224, eager; median of {steps} "
        f"steps per run, {rounds} alternating rounds")
    say(f"  {'trainable':16s} {'ms per round':28s} {'median':>8s} {'saved ms':>9s} {'peak GiB':>9s}   weight-gradient launches per step")
    for name, _ in configs:
        say(f"  {name:16s} {' '.join(f'{v:7.2f}' for v in res[name]):28s} {med[name]:8.2f} {base - med[name]:9.2f} {mem[name]:9.2f}   {launches[name]}")
    say(f"  the full step: median of both {base:.2f} ms, spread (max - min over {len(full)} runs) {spread:.2f} ms")
    ok = True
    for name, specs in configs[2:]:
        if not base - med[name] > spread:
            say(f"DEFECT: the step under {name} is not faster than the full step beyond its spread")
            ok = False
    return ok


def ab_part(parent, out_path, steps=20, warmup=5):
    rows, dumps = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in (1, 2):
            for tag, root in (("parent", parent), ("new", ROOT)):
                d = os.path.join(tmp, f"{tag}{rnd}")
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", d],
                                   cwd=root, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise RuntimeError(f"bench.py failed in {root}:\n{r.stderr[-2000:]}")
                line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                rows.append((f"{tag} {rnd}", line))
                dumps.append((f"{tag} {rnd}", d))
                print(f"{tag} {rnd}: {json.dumps(line)[:300]}", flush=True)
        first = dumps[0]
        names = sorted(os.listdir(first[1]))
        cmp_lines = []
        same_all = True
        for tag, d in dumps[1:]:
            same = sorted(os.listdir(d)) == names and all(filecmp.cmp(os.path.join(first[1], f), os.path.join(d, f), shallow=False) for f in names)
            same_all = same_all and same
            cmp_lines.append(f"{first[0]} vs {tag}: {'bit-identical' if same else 'DIFFERENT'}")
    txt = [f"bench.py --gpus 1 --steps {steps} --warmup {warmup} --dump-outputs, parent commit and this tree alternating in one session on one MI355X",
           "(every parameter trainable: the gradient plan asks for everything, the grouped weight-gradient launches go out as before and dcv_bias_grad is "
           "not launched)", "",
           f"{'run':9s} {'images/sec':>11s} {'ms/step':>9s} {'median ms/step':>15s}"]
    for tag, line in rows:
        txt.append(f"{tag:9s} {line['value']:11.2f} {line['ms_per_step']:9.3f} {line['median_ms_per_step']:15.3f}")
    txt += ["", f"--dump-outputs ({', '.join(names)}), compared byte for byte:", "    ".join(cmp_lines)]
    with open(out_path, "w") as f:
        f.write("\n".join(txt) + "\n")
    print("\n".join(txt), flush=True)
    return same_all


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selective_backward_bench.txt"))
    ap.add_argument("--ab", metavar="PARENT", default=None, help="a built checkout of the parent commit: run the bench.py A/B instead")
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "selective_backward_bench_ab.txt"))
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("selective_backward_bench needs the GPU: a CPU run gives no time")
    if a.ab:
        raise SystemExit(0 if ab_part(os.path.abspath(a.ab), a.ab_out) else 1)
    kernel_part(a.iters)
    ok = True
    if not a.kernel_only:
        ok = step_part(make_model(), a.rounds)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
