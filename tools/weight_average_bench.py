"""Measurements of weight averaging on one MI355X, DiChaViT-S at the headline config (8 channels, 224 x 224, patch 16, bs 64).

Kernel: dcv_avg_update over the model's real FULL arena (model._arena -> the averaged copy's arena, count > 0 read from a device word)
against what it replaces — torch.optim.swa_utils.AveragedModel.update_parameters on a deep copy of the same model, at a count > 0, timed
twice as two candidates for the baseline's own spread — and against a device-to-device copy that moves the same 12 bytes per element (a
copy_ of 1.5 n floats).  Also every launch shape that was tried: grid caps through the grid_cap argument, and the number of float4 in
flight per lane through stand-alone builds of csrc/avg.hip with -DDCV_AVG_ILP=k (--build-variants makes them, where hipcc is; they are
loaded next to the product library, same entry point).  One process, candidates alternating inside every round, medians of --iters
launches after warm-up.  The kernel must be faster than the FASTER torch median by more than the spread of the two: otherwise a line
starting with DEFECT is printed and the exit status is 1.  The ratio to the copy is reported without a bar.

Step: forward + backward + HipAdamW.step at bs 64, eager and captured (GraphedTrainStep), each with and without update_parameters after
every step (the SWAD case); the four configurations alternate over --rounds rounds, median of 10 steps per run.

--ab PARENT: bench.py --steps 20 --warmup 5 --dump-outputs in PARENT (a built checkout of the parent commit) and in this tree, alternating,
two runs each; the dumps are compared byte for byte.

    python tools/weight_average_bench.py --build-variants
    python tools/weight_average_bench.py [--iters 60] [--rounds 3] [--out profiles/weight_average_bench.txt]
    python tools/weight_average_bench.py --ab PARENT [--ab-out profiles/weight_average_bench_ab.txt]
"""
import argparse
import ctypes
import filecmp
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "diverse_channel_vit_amd")

B, C = 64, 8
ILP_VARIANTS = (1, 2, 8)  # the product is 4
GRID_CAPS = (256, 512, 1024, 1792, 4096, 1 << 20)  # the product is 2048; 1 << 20: no walking at all
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def variant_path(k):
    return os.path.join(PKG, f"libdcv_avg_ilp{k}.so")


def build_variants():
    from diverse_channel_vit_amd import _build
    for k in ILP_VARIANTS:
        cmd = [_build.HIPCC] + _build.FLAGS + [f"-DDCV_AVG_ILP={k}", "-shared", os.path.join(_build.CSRC, "avg.hip"), "-o", variant_path(k)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"hipcc failed for ILP {k}:\n{r.stderr}")
        print("built", variant_path(k))


class Cfg(dict):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return self.get(k)


def make_model():
    import torch
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
    import torch
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
    import torch
    from torch.optim import swa_utils
    import diverse_channel_vit_amd as dcv
    from diverse_channel_vit_amd import hip
    dev = torch.device("cuda")
    model._ensure_arena(dev)
    ours = dcv.AveragedModel(model)
    ours.update_parameters(model)  # count 1 from here on; the copy's arena exists
    theirs = swa_utils.AveragedModel(model)  # what the trainer builds: a deep copy, n_averaged on the host
    theirs.update_parameters(model)
    src, dst, n = model._arena, ours.module._arena, model._arena.numel()
    word = torch.full((1,), 10, dtype=torch.int64, device=dev)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    a_ptr, p_ptr, w_ptr = ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(word.data_ptr())
    sig = hip._SIGS["dcv_avg_update"]

    fns = {"ours_a": lambda: hip.avg_update(dst, src, n, hip.AVG_SWA, n_averaged_dev=word),
           "torch_a": lambda: theirs.update_parameters(model)}
    labels = {"ours_a": "dcv_avg_update (one launch; ILP 4, cap 2048), 1st", "torch_a": "torch AveragedModel.update_parameters, 1st"}
    for cap in GRID_CAPS:
        fns[f"cap{cap}"] = lambda cap=cap: hip.avg_update(dst, src, n, hip.AVG_SWA, n_averaged_dev=word, grid_cap=cap)
        labels[f"cap{cap}"] = f"  grid_cap {cap}" + (" (no walking)" if cap == 1 << 20 else "")
    for k in ILP_VARIANTS:
        if not os.path.exists(variant_path(k)):
            say(f"(ILP {k}: {os.path.basename(variant_path(k))} not built: run --build-variants first; not measured)")
            continue
        fn = ctypes.CDLL(variant_path(k)).dcv_avg_update
        fn.argtypes, fn.restype = sig
        for cap in (0, 1 << 20):
            fns[f"ilp{k}_{cap}"] = lambda fn=fn, cap=cap: fn(a_ptr, p_ptr, n, 0, 0.0, 0, w_ptr, cap, stream())
            labels[f"ilp{k}_{cap}"] = f"  {k} float4 in flight per operand, " + ("cap 2048" if cap == 0 else "no walking")
    half = torch.empty(n * 3 // 2, device=dev)  # a copy of X bytes moves 2 X: 6 bytes per element copied = 12 moved
    half2 = torch.empty_like(half)
    fns["copy"] = lambda: half2.copy_(half)
    labels["copy"] = "device-to-device copy of the same bytes"
    fns["ours_b"] = fns["ours_a"]
    labels["ours_b"] = "dcv_avg_update, 2nd"
    fns["torch_b"] = fns["torch_a"]
    labels["torch_b"] = "torch AveragedModel.update_parameters, 2nd"
    t = time_alternating(fns, iters)
    nbytes = 12.0 * n
    say(f"kernel: DiChaViT-S full arena, {n} floats ({len(model._all_params)} tensors), SWA at a count > 0 read from a device word; "
        f"{nbytes / 1e6:.1f} MB moved per update (12 B per element); medians of {iters} alternating launches, device events around each call")
    say(f"  {'candidate':58s} {'us':>9s} {'TB/s':>7s} {'vs copy':>8s}")
    for key in fns:
        say(f"  {labels[key]:58s} {t[key]:9.1f} {nbytes / (t[key] * 1e-6) / 1e12:7.3f} {t[key] / t['copy']:8.3f}")
    spread_t, spread_o = abs(t["torch_a"] - t["torch_b"]), abs(t["ours_a"] - t["ours_b"])
    base, mine = min(t["torch_a"], t["torch_b"]), max(t["ours_a"], t["ours_b"])
    say(f"  spread |1st - 2nd|: torch {spread_t:.1f} us, dcv_avg_update {spread_o:.1f} us; faster torch median - slower dcv_avg_update median = "
        f"{base - mine:+.1f} us ({base / mine:.2f}x); dcv_avg_update / copy = {mine / t['copy']:.3f}")
    ok = mine < base - spread_t
    if not ok:
        say("DEFECT: dcv_avg_update is not faster than torch's update_parameters by more than the baseline's spread")
    return ok


def step_part(rounds, steps=10):
    import torch
    import diverse_channel_vit_amd as dcv
    x = torch.randn(B, C, 224, 224, device="cuda")
    y = torch.randint(0, 161, (B,), device="cuda")
    ce = torch.nn.CrossEntropyLoss()

    def eager(with_avg):
        model = make_model()
        opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=4.9e-5, weight_decay=0.04, model=model)
        avg = dcv.AveragedModel(model) if with_avg else None

        def one():
            opt.zero_grad(set_to_none=True)
            out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
            (ce(out, y) + extra).backward()
            opt.step()
            if avg is not None:
                avg.update_parameters(model)
        return one

    def captured(with_avg):
        model = make_model()
        opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=4.9e-5, weight_decay=0.04, model=model, capturable=True)
        gs = dcv.GraphedTrainStep(model, opt, "train", None, ce, 1.0, warmup=2, averager=dcv.AveragedModel(model) if with_avg else None)
        return lambda: gs(x, y)

    configs = {"eager": eager(False), "eager + update": eager(True), "captured": captured(False), "captured + update": captured(True)}

    def timed(one):
        for _ in range(3):
            one()
        torch.cuda.synchronize()
        ts = []
        for _ in range(steps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            one()
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e))
        return sorted(ts)[len(ts) // 2]

    res = {k: [] for k in configs}
    for _ in range(rounds):
        for k, one in configs.items():
            res[k].append(timed(one))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    say()
    say(f"step: forward + backward + HipAdamW.step at bs {B}, {C} channels, 224 x 224, with and without AveragedModel.update_parameters after "
        f"every step (SWAD); median of {steps} steps per run, {rounds} alternating rounds")
    say(f"  {'configuration':18s} {'ms per round':32s} {'median':>8s} {'max - min':>10s} {'update costs':>13s}")
    for k in configs:
        base = k.replace(" + update", "")
        cost = f"{(med[k] - med[base]) * 1e3:+10.0f} us" if k != base else ""
        say(f"  {k:18s} {' '.join(f'{v:7.2f}' for v in res[k]):32s} {med[k]:8.2f} {max(res[k]) - min(res[k]):10.2f} {cost:>13s}")
    return True


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
           "(no averager: GraphedTrainStep, save_checkpoint and load_checkpoint at their defaults, dcv_avg_update is not launched)", "",
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
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_average_bench.txt"))
    ap.add_argument("--build-variants", action="store_true", help="build the ILP variants of csrc/avg.hip (needs hipcc, no GPU) and exit")
    ap.add_argument("--ab", metavar="PARENT", default=None, help="a built checkout of the parent commit: run the bench.py A/B instead")
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "weight_average_bench_ab.txt"))
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    if a.build_variants:
        build_variants()
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("weight_average_bench needs the GPU: a CPU run gives no time")
    if a.ab:
        raise SystemExit(0 if ab_part(os.path.abspath(a.ab), a.ab_out) else 1)
    ok = kernel_part(make_model(), a.iters)
    if not a.kernel_only:
        ok = step_part(a.rounds) and ok
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
