"""Measurements of the fine-tuning path on one MI355X, DiChaViT-S at the headline config (8 channels, 224 x 224, patch 16, bs 64).

Kernel: dcv_adamw_groups over the model's real arena with the table of param_groups(layer_decay=0.75) (LLRD + no-decay split) against
dcv_adamw_dyn over the same range (what a single group costs; timed twice, as two candidates, for the baseline's own spread), against one
dcv_adamw_dyn per tensor (what the same groups cost without the kernel), and against a device-to-device copy that moves the same 28 bytes
per parameter.  One process, candidates alternating inside every round, medians of --iters rounds after warm-up.  The grouped kernel must
not be slower than the FASTER of the two dcv_adamw_dyn medians by more than that spread: otherwise a line starting with DEFECT is printed and the exit status is 1.

Step: forward + backward + optimizer step and the peak memory, for k frozen blocks (model.freeze_prefix(k)) in {0, 6, 8, 11}; k = 0 both
with a single group and with the LLRD groups.  The configurations alternate over --rounds rounds (k = 0 single-group once per round: its
spread is the yardstick).  Also the eval forward and the optimizer step alone, for the expected saving k / 12 x (step - eval forward -
optimizer).  The step time must fall strictly with k beyond the k = 0 spread, and LLRD at k = 0 must be within it (DEFECT otherwise).

--ab PARENT: bench.py --steps 20 --warmup 5 --dump-outputs in PARENT (a built checkout of the parent commit) and in this tree, alternating,
two runs each; the dumps are compared byte for byte.

    python tools/finetune_bench.py [--iters 50] [--rounds 3] [--out profiles/finetune_bench.txt] [--ab PARENT --ab-out profiles/finetune_bench_ab.txt]
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

B, C = 64, 8
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


def kernel_part(model, iters):
    import diverse_channel_vit_amd as dcv
    from diverse_channel_vit_amd import hip
    from diverse_channel_vit_amd.optim import build_segments
    model._ensure_arena(torch.device("cuda"))
    groups = dcv.param_groups(model, lr=1e-4, weight_decay=0.04, layer_decay=0.75)
    gid = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
    rows = [gid[id(p)] for p in model._enc_params]
    ends4, grps = build_segments(model._enc_off, model._enc_size, rows)
    n = model._enc_size
    dev = "cuda"
    p = model._arena[:n].clone()
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    hyper = torch.zeros(8 * len(groups), device=dev)
    hip.adamw_set_hyper_groups(hyper, [(gr["lr"], 0.9, 0.999, 1e-8, gr["weight_decay"]) for gr in groups], [10] * len(groups), 1.0)
    e_dev, g_dev = torch.tensor(ends4, dtype=torch.int32, device=dev), torch.tensor(grps, dtype=torch.int32, device=dev)
    slots = [(o, (model._enc_off[i + 1] if i + 1 < len(rows) else n) - o, rows[i]) for i, o in enumerate(model._enc_off)]
    src = torch.empty(n * 7 // 2, device=dev)  # a copy of X bytes moves 2 X: 14 bytes per parameter copied = 28 moved
    dst = torch.empty_like(src)

    def per_tensor():
        for o, ln, r in slots:
            hip.adamw_dyn(p[o:o + ln], g[o:o + ln], m[o:o + ln], v[o:o + ln], ln, hyper[8 * r:8 * r + 8])

    dyn = lambda: hip.adamw_dyn(p, g, m, v, n, hyper)  # noqa: E731
    t = time_alternating({"dyn_a": dyn, "groups": lambda: hip.adamw_groups(p, g, m, v, n, e_dev, g_dev, len(ends4), hyper, len(groups)),
                          "dyn_b": dyn, "per_tensor": per_tensor, "copy": lambda: dst.copy_(src)}, iters)
    nbytes = 28.0 * n
    spread = abs(t["dyn_a"] - t["dyn_b"])
    if os.environ.get("DCV_LIB"):
        say(f"library: {os.path.basename(os.environ['DCV_LIB'])} (a build_variant of the same sources)")
    say(f"kernel: DiChaViT-S encoder arena, {n} floats ({len(rows)} tensors), param_groups(layer_decay=0.75): {len(groups)} groups, "
        f"{len(ends4)} runs in the table; {nbytes / 1e6:.1f} MB moved per launch (28 B per parameter); medians of {iters} alternating launches")
    say(f"  {'candidate':46s} {'us':>9s} {'TB/s':>7s} {'vs copy':>8s}")
    for key, label in (("groups", "dcv_adamw_groups (one launch, the table)"), ("dyn_a", "dcv_adamw_dyn, whole range (single group), 1st"),
                       ("dyn_b", "dcv_adamw_dyn, whole range (single group), 2nd"), ("per_tensor", f"dcv_adamw_dyn per tensor ({len(slots)} launches)"),
                       ("copy", "device-to-device copy of the same bytes")):
        say(f"  {label:46s} {t[key]:9.1f} {nbytes / (t[key] * 1e-6) / 1e12:7.3f} {t[key] / t['copy']:8.3f}")
    base = min(t["dyn_a"], t["dyn_b"])
    say(f"  baseline spread |1st - 2nd| = {spread:.1f} us; grouped - faster baseline = {t['groups'] - base:+.1f} us")
    ok = t["groups"] <= base + spread
    if not ok:
        say("DEFECT: dcv_adamw_groups is slower than dcv_adamw_dyn over the same range by more than the baseline's spread")
    return ok


def step_part(model, rounds, steps=10):
    import diverse_channel_vit_amd as dcv
    x = torch.randn(B, C, 224, 224, device="cuda")
    y = torch.randint(0, 161, (B,), device="cuda")
    ce = torch.nn.CrossEntropyLoss()
    configs = [("k0 single", 0, False), ("k0 llrd", 0, True), ("k6", 6, False), ("k8", 8, False), ("k11", 11, False)]
    opts = {}

    def setup(name, k, llrd):
        if k:
            model.freeze_prefix(k)
        else:
            model.freeze_prefix(0, tokeniser=False)
        if name not in opts:
            params = dcv.param_groups(model, 4.9e-5, 0.04, layer_decay=0.75) if llrd else [p for p in model.parameters() if p.requires_grad]
            opts[name] = dcv.HipAdamW(params, lr=4.9e-5, weight_decay=0.04, model=model)
        return opts[name]

    def one(opt):
        model.zero_grad(set_to_none=True)  # not opt.zero_grad(): a parameter frozen now may hold a gradient of the configuration before
        out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        (ce(out, y) + extra).backward()
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

    res = {name: [] for name, _, _ in configs}
    mem = {}
    for _ in range(rounds):
        for name, k, llrd in configs:
            ms, gb = timed(setup(name, k, llrd))
            res[name].append(ms)
            mem[name] = gb
    # the two terms of the expected saving
    opt = setup("k0 single", 0, False)
    one(opt)
    t_opt = time_alternating({"opt": opt.step}, 20, warmup=2)["opt"] / 1e3
    model.eval()
    with torch.no_grad():
        t_eval = time_alternating({"eval": lambda: model(x, "train", None)}, 10, warmup=2)["eval"] / 1e3
    model.train()
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    spread = max(res["k0 single"]) - min(res["k0 single"])
    say()
    say(f"step: forward + backward + HipAdamW.step at bs {B}, {C} channels, 224 x 224; median of {steps} steps per run, {rounds} alternating rounds; "
        f"eval forward {t_eval:.2f} ms, optimizer step alone {t_opt:.3f} ms")
    say(f"  {'configuration':12s} {'ms per round':32s} {'median':>8s} {'peak GiB':>9s} {'saved ms':>9s} {'k/12 x (step - eval - opt)':>27s}")
    backward_side = med["k0 single"] - t_eval - t_opt
    for name, k, _ in configs:
        exp = f"{k / 12 * backward_side:27.2f}" if k else f"{'':27s}"
        say(f"  {name:12s} {' '.join(f'{v:7.2f}' for v in res[name]):32s} {med[name]:8.2f} {mem[name]:9.2f} {med['k0 single'] - med[name]:9.2f} {exp}")
    say(f"  spread of the k0 single runs (max - min): {spread:.2f} ms")
    ok = True
    order = ["k0 single", "k6", "k8", "k11"]
    for a, b in zip(order, order[1:]):
        if not med[a] - med[b] > spread:
            say(f"DEFECT: the step at {b} is not faster than at {a} beyond the spread")
            ok = False
    if abs(med["k0 llrd"] - med["k0 single"]) > spread:
        say("DEFECT: the LLRD groups at k = 0 are outside the spread of the single-group step")
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
           "(single group, every parameter trainable: HipAdamW takes dcv_adamw as before, no frozen prefix, the table kernel is not launched)", "",
           f"{'run':9s} {'images/sec':>11s} {'ms/step':>9s} {'median ms/step':>15s}"]
    for tag, line in rows:
        val = line["value"]
        ms, med = line["ms_per_step"], line["median_ms_per_step"]
        txt.append(f"{tag:9s} {val:11.2f} {ms:9.3f} {med:15.3f}")
    txt += ["", f"--dump-outputs ({', '.join(names)}), compared byte for byte:", "    ".join(cmp_lines)]
    with open(out_path, "w") as f:
        f.write("\n".join(txt) + "\n")
    print("\n".join(txt), flush=True)
    return same_all


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_bench.txt"))
    ap.add_argument("--ab", metavar="PARENT", default=None, help="a built checkout of the parent commit: run the bench.py A/B instead")
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "finetune_bench_ab.txt"))
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_bench needs the GPU: a CPU run gives no time")
    if a.ab:
        raise SystemExit(0 if ab_part(os.path.abspath(a.ab), a.ab_out) else 1)
    model = make_model()
    ok = kernel_part(model, a.iters)
    if not a.kernel_only:
        ok = step_part(model, a.rounds) and ok
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
