"""Measurements of the device augmentation on one MI355X: dcv_tps_warp + dcv_crop_resize_flip (DeviceAugment.apply's two launches).

Kernels: three shapes at B = 64 — 8 channels 224 -> 224 (the headline shape), 5 channels 160 -> 224 (CHAMMI CP), 4 channels 512 -> 224 — uint8
input, boxes and control points from DeviceAugment.sample, each with every sample warped and with p = 0.2.  Candidates, alternating inside every
round in one process, device events around each call, medians of --iters calls after warm-up:
  ours   the two launches with the parameter tables already on the device (timed twice: 1st / 2nd);
  copy   a device-to-device copy that moves the bytes the two launches move at the least (every byte of the boxes and of the warped samples
         read once, every output byte written once) — the floor; the ratio is reported, no bar is set;
  torch  the same work composed from torch ops on the device (timed twice, for the baseline's own spread): the coarse grid, the reference's
         upsampling rule and the sampling field built with tensor ops, F.grid_sample(bilinear, reflection) on the warped samples, then per sample
         crop, F.interpolate(bilinear, antialias=True) and flip.
The two launches must be faster than the FASTER torch median by more than the spread of the two torch medians: otherwise a line starting with
DEFECT is printed and the exit status is 1.

Rows: dcv_tps_warp alone at its product setting (2 image rows per workgroup) against stand-alone builds of csrc/augment.hip with
-DDCV_TPS_ROWS=1 / 4 / 8 (--build-variants makes them, where hipcc is; same entry point), and a launch with no sample flagged, which is what
the events around one call cost by themselves.

Host: DeviceAugment.sample plus tps_coefficients for the warped samples, per batch of 64 (wall clock, median).
Step: forward + backward + HipAdamW.step at bs 64, 8 channels, 224 x 224 on a fixed float batch, against the same step with DeviceAugment (fresh
parameters every step, uint8 batch) in front of it; the two alternate over --rounds rounds, median of 10 steps per run.

--ab PARENT: bench.py --steps 20 --warmup 5 --dump-outputs in PARENT (a built checkout of the parent commit) and in this tree, alternating, two
runs each; the dumps are compared byte for byte.

    python tools/device_augment_bench.py --build-variants
    python tools/device_augment_bench.py [--iters 40] [--rounds 3] [--out profiles/device_augment_bench.txt]
    python tools/device_augment_bench.py --ab PARENT [--ab-out profiles/device_augment_bench_ab.txt]
"""
import argparse
import ctypes
import filecmp
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 64
SHAPES = ((8, 224), (5, 160), (4, 512))  # (channels, W); every one -> 224
S = 224
ROWS_VARIANTS = (1, 4, 8)  # the product is 2
PKG = os.path.join(ROOT, "diverse_channel_vit_amd")
LINES = []


def variant_path(r):
    return os.path.join(PKG, f"libdcv_aug_rows{r}.so")


def build_variants():
    from diverse_channel_vit_amd import _build
    for r in ROWS_VARIANTS:
        cmd = [_build.HIPCC] + _build.FLAGS + [f"-DDCV_TPS_ROWS={r}", "-shared", os.path.join(_build.CSRC, "augment.hip"), "-o", variant_path(r)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise SystemExit(f"hipcc failed for {r} rows:\n{res.stderr}")
        print("built", variant_path(r))


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def time_alternating(fns, iters, warmup=3):
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


def torch_composition(x, P, coef, tps_idx, boxes, flips, out):
    """The work of the two launches from torch ops: x uint8 [B, C, W, W]; P [B, K, 2], coef [B, 2, K + 3] float64 on the device; tps_idx the
    warped samples (device int64); boxes / flips host lists."""
    import torch
    import torch.nn.functional as F
    W = x.shape[-1]
    xf = x.float()
    if tps_idx.numel():
        steps = (W - 1) / 10
        n = int(steps)
        K = P.shape[1]
        Pm, cm = P[tps_idx], coef[tps_idx]
        g = torch.arange(n, dtype=torch.float64, device=x.device) * ((W - 1) / (n - 1))
        gx, gy = g[:, None].expand(n, n), g[None, :].expand(n, n)
        r2 = (Pm[:, :, 0, None, None] - gx) ** 2 + (Pm[:, :, 1, None, None] - gy) ** 2          # [m, K, n, n]
        u = torch.where(r2 < 1e-200, torch.zeros_like(r2), r2 * 0.5 * torch.log(r2.clamp(min=1e-300)))
        coarse = (cm[:, :, :K, None, None] * u[:, None]).sum(2) + cm[:, :, K, None, None] + cm[:, :, K + 1, None, None] * gx + cm[:, :, K + 2, None, None] * gy
        coarse = coarse.float()                                                                    # [m, 2, n, n]
        pos = (steps - 1) * torch.arange(W, dtype=torch.float64, device=x.device) / float(W - 1)
        idx = pos.long()
        fr = (pos - idx).float()
        up = (idx + 1).clamp(max=int(steps - 1))
        t0, t1 = coarse[:, :, idx], coarse[:, :, up]                                               # rows
        rows = t0 * (1 - fr)[:, None] + t1 * fr[:, None]
        field = rows[..., idx] * (1 - fr) + rows[..., up] * fr                                     # [m, 2, W, W]: (axis 0, axis 1)
        grid = torch.stack([(2 * field[:, 1] + 1) / W - 1, (2 * field[:, 0] + 1) / W - 1], dim=-1)
        xf[tps_idx] = F.grid_sample(xf[tps_idx], grid, mode="bilinear", padding_mode="reflection", align_corners=False)
    for b, ((i, j, h, w), flip) in enumerate(zip(boxes, flips)):
        o = F.interpolate(xf[b:b + 1, :, i:i + h, j:j + w], size=(S, S), mode="bilinear", align_corners=False, antialias=True)
        out[b] = o[0].flip(-1) if flip else o[0]
    return out


def kernel_part(iters):
    import torch
    import diverse_channel_vit_amd as dcv
    from diverse_channel_vit_amd import augment as A, hip
    dev = torch.device("cuda")
    ok = True
    say(f"kernels: B {B}, uint8 input, output {S} x {S} float32; medians of {iters} alternating calls, device events around each call")
    say(f"  {'shape':22s} {'warped':>7s} {'MB moved':>9s} {'ours 1st':>9s} {'ours 2nd':>9s} {'copy':>8s} {'ours/copy':>10s} {'torch 1st':>10s} {'torch 2nd':>10s} "
        f"{'spread':>7s} {'torch/ours':>11s}   (us)")
    for C, W in SHAPES:
        x = torch.randint(0, 256, (B, C, W, W), dtype=torch.uint8, device=dev)
        for label, prob in (("all", 1.0), ("p 0.2", 0.2)):
            aug = dcv.DeviceAugment(size=S, tps_prob=prob, generator=torch.Generator().manual_seed(C * W))
            p = aug.sample(B, W, W)
            P = A.tps_control_points(p.dst, W).to(dev)
            coef = A.tps_coefficients(p.dst, p.src, W).to(dev)
            flag, flip, box = p.tps.to(torch.int32).to(dev), p.flip.to(torch.int32).to(dev), p.box.to(dev)
            ws = torch.empty(B, C, W, W, dtype=torch.float32, device=dev)
            out = torch.empty(B, C, S, S, dtype=torch.float32, device=dev)
            out_t = torch.empty_like(out)
            tps_idx = torch.nonzero(p.tps).flatten().to(dev)
            boxes, flips = p.box.tolist(), p.flip.tolist()
            m = int(p.tps.sum())
            nbytes = m * C * W * W * (1 + 4) + B * C * S * S * 4 + sum(C * h * w * (4 if t else 1) for (_, _, h, w), t in zip(boxes, p.tps.tolist()))
            src_c = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst_c = torch.empty_like(src_c)

            def ours():
                if m:
                    hip.tps_warp(x, P, coef, flag, ws)
                hip.crop_resize_flip(x, ws, flag, box, flip, out)

            def composed():
                torch_composition(x, P, coef, tps_idx, boxes, flips, out_t)

            t = time_alternating({"ours_a": ours, "torch_a": composed, "copy": lambda: dst_c.copy_(src_c), "ours_b": ours, "torch_b": composed}, iters)
            diff = (out - out_t).abs().max().item()
            spread = abs(t["torch_a"] - t["torch_b"])
            mine, base = max(t["ours_a"], t["ours_b"]), min(t["torch_a"], t["torch_b"])
            say(f"  {f'C {C}, {W} -> {S}':22s} {f'{m}/{B}':>7s} {nbytes / 1e6:9.1f} {t['ours_a']:9.1f} {t['ours_b']:9.1f} {t['copy']:8.1f} {mine / t['copy']:10.2f} "
                f"{t['torch_a']:10.1f} {t['torch_b']:10.1f} {spread:7.1f} {base / mine:11.1f}   max |ours - torch| {diff:.3f}")
            if not mine < base - spread:
                ok = False
                say(f"DEFECT: the two launches are not faster than the torch composition by more than its spread at C {C}, W {W}, {label}")
    return ok


def rows_part(iters):
    import torch
    import diverse_channel_vit_amd as dcv
    from diverse_channel_vit_amd import augment as A, hip
    dev = torch.device("cuda")
    fns_v = {}
    for r in ROWS_VARIANTS:
        if not os.path.exists(variant_path(r)):
            say(f"({r} rows: {os.path.basename(variant_path(r))} not built: run --build-variants first; not measured)")
            continue
        fn = ctypes.CDLL(variant_path(r)).dcv_tps_warp
        fn.argtypes, fn.restype = hip._SIGS["dcv_tps_warp"]
        fns_v[r] = fn
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    say()
    say(f"rows: dcv_tps_warp alone, B {B}, uint8 input, image rows per workgroup (product: 2); 'none' = no sample flagged: the cost of the events around one call; us, medians of {iters}")
    for C, W in SHAPES:
        x = torch.randint(0, 256, (B, C, W, W), dtype=torch.uint8, device=dev)
        for prob in (1.0, 0.2):
            p = dcv.DeviceAugment(size=S, tps_prob=prob, generator=torch.Generator().manual_seed(C * W)).sample(B, W, W)
            P, coef = A.tps_control_points(p.dst, W).to(dev), A.tps_coefficients(p.dst, p.src, W).to(dev)
            flag = p.tps.to(torch.int32).to(dev)
            none = torch.zeros_like(flag)
            ws = torch.empty(B, C, W, W, dtype=torch.float32, device=dev)
            fns = {"2 rows": lambda: hip.tps_warp(x, P, coef, flag, ws), "none": lambda: hip.tps_warp(x, P, coef, none, ws)}
            for r, fn in fns_v.items():
                fns[f"{r} rows"] = lambda fn=fn: fn(vp(x), 1, vp(P), vp(coef), vp(flag), vp(ws), B, C, W, P.shape[1], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            t = time_alternating(fns, iters)
            say(f"  C {C}, W {W:3d}, warped {int(p.tps.sum()):2d}/{B}: " + "   ".join(f"{k} {v:6.1f}" for k, v in sorted(t.items())))


def host_part(reps=30):
    import torch
    import diverse_channel_vit_amd as dcv
    say()
    say(f"host: DeviceAugment.sample + tps_coefficients for the warped samples, batch of {B}, wall clock, median of {reps} ({torch.get_num_threads()} torch threads)")
    for W in (224, 160, 512):
        for prob in (0.2, 1.0):
            aug = dcv.DeviceAugment(size=S, tps_prob=prob, generator=torch.Generator().manual_seed(1))
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                p = aug.sample(B, W, W)
                t1 = time.perf_counter()
                if bool(p.tps.any()):
                    dcv.tps_coefficients(p.dst[p.tps], p.src, W)
                ts.append((t1 - t0, time.perf_counter() - t1))
            med = lambda k: sorted(v[k] for v in ts)[len(ts) // 2] * 1e6  # noqa: E731
            say(f"  W {W:4d}  tps_prob {prob:.1f}: sample {med(0):7.0f} us   tps_coefficients {med(1):7.0f} us")


def step_part(rounds, steps=10):
    import torch
    import diverse_channel_vit_amd as dcv
    from weight_average_bench import make_model
    C, W = 8, 224
    raw = torch.randint(0, 256, (B, C, W, W), dtype=torch.uint8, device="cuda")
    fixed = raw.float()
    y = torch.randint(0, 161, (B,), device="cuda")
    ce = torch.nn.CrossEntropyLoss()
    mean, std = [0.1] * C, [0.2] * C

    def make(with_aug):
        model = make_model()
        model.set_input_normalisation(mean, std, 255.0)
        opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=4.9e-5, weight_decay=0.04, model=model)
        aug = dcv.DeviceAugment(size=S, generator=torch.Generator().manual_seed(0))

        def one():
            x = aug(raw) if with_aug else fixed
            opt.zero_grad(set_to_none=True)
            out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
            (ce(out, y) + extra).backward()
            opt.step()
        return one

    configs = {"step": make(False), "DeviceAugment + step": make(True)}

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
    say(f"step: eager forward + backward + HipAdamW.step at bs {B}, {C} channels, {W} x {W}, raw input with set_input_normalisation; with DeviceAugment "
        f"(tps_prob 0.2, new parameters every step, drawn and solved on the host inside the timed region) in front; median of {steps} steps per run, {rounds} alternating rounds")
    say(f"  {'configuration':22s} {'ms per round':32s} {'median':>8s} {'max - min':>10s} {'augment costs':>14s}")
    for k in configs:
        cost = f"{(med[k] - med['step']) * 1e3:+10.0f} us" if k != "step" else ""
        say(f"  {k:22s} {' '.join(f'{v:7.2f}' for v in res[k]):32s} {med[k]:8.2f} {max(res[k]) - min(res[k]):10.2f} {cost:>14s}")


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
           "(the benchmark feeds the model directly: DeviceAugment is not constructed and its two kernels are not launched)", "",
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
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_augment_bench.txt"))
    ap.add_argument("--build-variants", action="store_true", help="build the rows-per-workgroup variants of csrc/augment.hip (needs hipcc, no GPU) and exit")
    ap.add_argument("--ab", metavar="PARENT", default=None, help="a built checkout of the parent commit: run the bench.py A/B instead")
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "device_augment_bench_ab.txt"))
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    if a.build_variants:
        build_variants()
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("device_augment_bench needs the GPU: a CPU run gives no time")
    if a.ab:
        raise SystemExit(0 if ab_part(os.path.abspath(a.ab), a.ab_out) else 1)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    ok = kernel_part(a.iters)
    rows_part(a.iters)
    host_part()
    if not a.kernel_only:
        step_part(a.rounds)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
