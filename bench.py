#!/usr/bin/env python
"""Headline benchmark: train images/sec, DiChaViT-S, 8-ch 224x224, bs=64 per GPU (BASELINE.json).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
           bench.py --gpus N --steps K --warmup W

One step = one pass of the hot path over one synthetic batch already resident in HBM:
zero_grad -> forward (tokeniser, 12 blocks, regularisers) -> CE + extra -> backward (+ RCCL gradient
all-reduce overlapped with backward when N > 1) -> fused AdamW.  The reference's three per-step
``.item()`` logging syncs (trainer.py:1021-1027) are NOT included (the loss stays on the device).

Prints ONE JSON line on rank 0 (contract in the task statement):
  * value / ms_per_step : wall clock over EXACTLY K steps between barrier + synchronize pairs, max over ranks;
    median_ms_per_step  : median of the K per-step event intervals (value_median = the rate it gives).
A plain run does only that: set-up, W warm-up steps, the K timed steps, the line.  With --full it also profiles warm-up steps,
re-times the dominant kernel inside the timed region and times the CPU baseline, and the line carries:
  * roofline            : the dominant kernel SYMBOL (largest share of a step, found in the profiled warm-up steps), its
    launches bracketed by HIP events on the launch stream INSIDE the timed region, achieved = algorithmic FLOPs (or bytes) of
    that launch / mean event interval; `executed_*` = the FLOPs the kernel really performs (S recomputed in the attention
    backward); `algorithmic_bytes` and `traffic` (HBM bytes per launch from the committed rocprofv3 --pmc passes of the
    newest profiles/rNN_vM_pmc_traffic.json, FETCH_SIZE x2 + WRITE_SIZE per the gfx950 correction);
  * kernel_table        : one row per kernel symbol and problem shape from the profiled warm-up steps (every C-ABI launch
    bracketed by events): launches/step, mean us, FLOPs and algorithmic bytes per launch, achieved rate and fraction of the
    MFMA / HBM peak, share of the step — so the worst kernel is named;
  * cpu_baseline        : the oracle (CPU restatement of the reference, "port") timed on this box's host cores.

--dump-outputs DIR writes what the last timed step handed its caller as DIR/<name>.npy (see dump_outputs); the inputs, the
initial weights and the rounding seeds are fixed, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import glob
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16 = 2.5e15  # dense MFMA bf16, MI355X_MICROARCH.md
PEAK_HBM = 8.0e12   # HBM3E spec (6.29 TB/s measured with a float4 copy), MI355X_MICROARCH.md
RIDGE = PEAK_BF16 / PEAK_HBM  # 312.5 FLOP per HBM byte: below it a kernel is HBM-bound on paper
TRAIN_GFLOP_PER_IMG = 336.94  # BASELINE.md §3 (matmul-only, train = 3 x fwd)
DEAD_GFLOP_PER_IMG = 23.82    # rows of the last block that never reach the output


class Cfg(dict):
    __getattr__ = dict.get


def model_cfg(arch="small", channels=8, img=224, patch=16, classes=161):
    # JUMP-CP script hyper-parameters (train_scripts.sh:5) with enable_sample=False (SURVEY §8d headline run)
    return Cfg(name="dichavit", pretrained_model_name=arch, patch_size=patch, temperature=0.07, learnable_temp=False,
               enable_sample=False, use_channelvit_channels=True, orthogonal_channel_emb_init=True, dropout_tokens_hcs="none",
               freeze_channel_emb=False, block_type="block", hcs_sampling="none", hcs_sampling_temp=1000.0,
               proxy_loss_lambda=0.001, ortho_loss_v1_lambda=0.001, drop_path_rate=0.0, gamma_s=1.0, gamma_d=4.0,
               reverse_pos_pairs=True, use_square=False, new_channel_inits=["zero"],
               in_channel_names=[f"c{i}" for i in range(channels)], img_size=[img], num_classes=classes)


def cpu_baseline(cfg, channels, img, classes, sample_bs=8, steps=3):
    """The oracle (CPU restatement of the reference's path, fp32) timed on this host: baseline only (BASELINE.md §4:
    1 warm-up + >= 3 timed steps at batch 8, the rate scales linearly with the batch)."""
    from oracle import dichavit_oracle as orc
    # the box's CPU share, not the host's core count (an oversubscribed pool is many times slower)
    try:
        ncpu = len(os.sched_getaffinity(0))
    except AttributeError:
        ncpu = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(ncpu, 16)))
    shapes = orc.state_shapes(cfg, channels, img, classes)
    sd = orc.make_state(shapes, 0)
    names = [k for k in sd if k != "proxies"]
    for k in names:
        sd[k].requires_grad_(True)
    m = {k: torch.zeros_like(sd[k]) for k in names}
    v = {k: torch.zeros_like(sd[k]) for k in names}
    x, y = orc.make_batch(1234, sample_bs, channels, img, classes)
    ch = list(range(channels))
    times = []
    for s in range(steps + 1):
        t0 = time.time()
        for k in names:
            sd[k].grad = None
        loss, _, _, _ = orc.train_loss(sd, x, y, cfg, ch, ch)
        loss.backward()
        with torch.no_grad():
            for k in names:
                orc.adamw_step(sd[k], sd[k].grad, m[k], v[k], s + 1, 4.9e-5, 0.9, 0.999, 1e-8, 0.04)
        if s > 0:
            times.append(time.time() - t0)
    dt = float(np.median(times))
    return {"value": round(sample_bs / dt, 4), "unit": "images/sec", "cores": torch.get_num_threads(), "kind": "port",
            # the reference cannot travel to the GPU box; its own rate was measured in the build container
            "reference_itself": {"value": 0.63, "unit": "images/sec", "cores": 8, "where": "the real reference (fp32, CPU, same model and batch shape) "
                                 "in the build container, BASELINE.md section 2 — not timed on this box"},
            "sample": f"median of {steps} timed fp32 train steps (after 1 warm-up) of the same model at batch {sample_bs} on the host CPU "
                      f"({dt:.1f} s per step)"}


DUMP_SAMPLE = 1 << 22  # elements kept of each flat parameter / gradient vector: 16 MB of fp32 each
DUMP_SEED = 20261016


def dump_outputs(path, loss, out_name, out, model):
    """What the last timed step hands its caller, as float32 / float64 .npy files under `path`:
      loss.npy              the step's loss (float64 scalar);
      logits.npy            the model output of that step (features.npy for --chammi: the proxy-loss features of its last chunk);
      params.npy, grads.npy every parameter after the optimiser step and its gradient, flattened and concatenated in
                            named_parameters() order (a missing gradient counts as zeros); above DUMP_SAMPLE elements, the same
                            fixed sample of positions for both (sorted, drawn from RandomState(DUMP_SEED))."""
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "loss.npy"), np.asarray(loss.item(), dtype=np.float64))
    np.save(os.path.join(path, out_name + ".npy"), out.float().cpu().numpy())
    params = [p for _, p in model.named_parameters()]
    flat_p = torch.cat([p.detach().reshape(-1).float() for p in params])
    flat_g = torch.cat([(p.grad.detach() if p.grad is not None else torch.zeros_like(p)).reshape(-1).float() for p in params])
    if flat_p.numel() > DUMP_SAMPLE:
        idx = np.unique(np.random.RandomState(DUMP_SEED).randint(0, flat_p.numel(), DUMP_SAMPLE))
        idx = torch.from_numpy(idx).to(flat_p.device)
        flat_p, flat_g = flat_p[idx], flat_g[idx]
    np.save(os.path.join(path, "params.npy"), flat_p.cpu().numpy())
    np.save(os.path.join(path, "grads.npy"), flat_g.cpu().numpy())


def newest_pmc_file():
    """profiles/rNN_vM_pmc_traffic.json with the highest (round, version) — numeric, not lexicographic."""
    best, best_key = None, None
    for f in glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic.json")):
        m = re.match(r"r(\d+)_v(\d+)_pmc_traffic\.json$", os.path.basename(f))
        key = (int(m.group(1)), int(m.group(2))) if m else (-1, -1)
        if best_key is None or key > best_key or (key == best_key and os.path.getmtime(f) > os.path.getmtime(best)):
            best, best_key = f, key
    return best


def table_from(prof, n_steps, step_ms):
    """rows per (symbol, shape) from hip.set_profiler records taken over n_steps eager steps"""
    rows = []
    for (sym, shape), r in prof.items():
        ts = [s.elapsed_time(e) for s, e in r["ev"]]
        if not ts:
            continue
        avg = float(np.mean(ts))
        row = {"symbol": sym, "shape": shape, "launches_per_step": round(len(ts) / n_steps, 2), "avg_us": round(avg * 1e3, 1),
               "ms_per_step": round(sum(ts) / n_steps, 3), "share_of_step": round(sum(ts) / n_steps / step_ms, 4)}
        if r["flops"] > 0:
            # which roofline binds THIS launch: its arithmetic intensity (executed FLOPs per algorithmic HBM byte) against the ridge
            # PEAK_BF16 / PEAK_HBM = 312.5 FLOP/B.  Every D = 384 GEMM of the encoder sits below it (170-290 FLOP/B): HBM-bound on paper.
            ai = r["flops_exec"] / r["bytes"] if r["bytes"] > 0 else float("inf")
            row.update(bound="mfma" if ai >= RIDGE else "hbm", flop_per_byte=round(ai, 1) if ai != float("inf") else None, gflop=round(r["flops"] / 1e9, 2), gflop_executed=round(r["flops_exec"] / 1e9, 2),
                       achieved_tflops=round(r["flops"] / (avg * 1e-3) / 1e12, 1), frac=round(r["flops"] / (avg * 1e-3) / PEAK_BF16, 4),
                       frac_executed=round(r["flops_exec"] / (avg * 1e-3) / PEAK_BF16, 4))
        if r["bytes"] > 0:
            row.update(algorithmic_mbytes=round(r["bytes"] / 1e6, 1), achieved_gbps=round(r["bytes"] / (avg * 1e-3) / 1e9, 0),
                       hbm_frac=round(r["bytes"] / (avg * 1e-3) / PEAK_HBM, 4))
            if r["flops"] <= 0:
                row["bound"] = "hbm"
        rows.append(row)
    rows.sort(key=lambda r: -r["ms_per_step"])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="images per GPU")
    ap.add_argument("--arch", default="small")
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--classes", type=int, default=161)
    ap.add_argument("--full", action="store_true", help="also the profiled warm-up steps (kernel_table), the dominant kernel re-timed in the timed "
                                                      "region (roofline, step_roofline) and the CPU baseline; a plain run times the steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the loss, the model output and (a fixed sample of) the updated "
                                                                         "parameters and their gradients after the last timed step as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--atomic-reductions", action="store_true", help="cross-workgroup sums with fp32 atomics (set_deterministic(False)) instead of the default "
                    "deterministic forms (partials through workspaces, fixed-order second pass; bit-reproducible gradients, +0.7 %% step time)")
    ap.add_argument("--kernel-table", action="store_true", help="also print the per-symbol table to stderr (implies --full)")
    ap.add_argument("--graph", action="store_true", help="N=1: replay a HIP-graph capture of the step (about 1 %% faster than eager launches); the "
                                                         "dominant kernel's events then come from the profiled warm-up steps, not from the timed region")
    ap.add_argument("--no-graph", action="store_true", help="(default since round 2; kept for old command lines)")
    ap.add_argument("--force-dp", action="store_true", help="exercise the N>1 code path on one GPU: RCCL group of world size 1, collectives forced")
    ap.add_argument("--grad-dtype", default="float32", choices=["float32", "bfloat16"], help="N>1: dtype the gradient buckets travel in")
    ap.add_argument("--overlap", action="store_true", help="N>1: per-layer buckets all-reduced beside the backward (which then stays on the 256 x 128 GEMM tiles and "
                                                           "leaves 8 CUs to RCCL) instead of ONE all-reduce of the arena after it — the default since round 3: on one "
                                                           "GPU with collectives forced the overlapped mode costs 0.8 ms per step, the single all-reduce 0.5 ms")
    ap.add_argument("--no-overlap", action="store_true", help="(accepted for round-2 command lines: the default now)")
    ap.add_argument("--wgrad-stream", type=int, default=None, choices=[0, 1], help="weight-gradient GEMMs on a second HIP stream (default: the model's default)")
    ap.add_argument("--hcs", action="store_true", help="secondary run (SURVEY §8d): enable_sample=True, hcs_sampling=lowest_cosine_prob, temp 1000 "
                                                     "(variable sequence length; the sampled subset stays on the device: no host sync per step)")
    ap.add_argument("--chammi", action="store_true", help="secondary run (SURVEY §8d, BASELINE config 3): the CHAMMI step of trainer.py:846-935 — a 12-channel "
                                                        "model, the batch split into Allen / HPA / CP sub-batches of 3 / 4 / 5 channels, proxy main loss on the "
                                                        "features, three forward/backward passes accumulate into one optimiser step")
    ap.add_argument("--h2d", action="store_true", help="PCIe-inclusive variant (never the headline value): every step's batch comes from pinned "
                                                     "host memory through a copy stream, double-buffered against the previous step")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    full = args.full or args.kernel_table

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print(f"warning: WORLD_SIZE={world} but --gpus {args.gpus}; using WORLD_SIZE", file=sys.stderr)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback in the product path)")
    # rehearsal hook (never used by the driver): DCV_BENCH_REHEARSAL=gloo runs the N > 1 code path with every rank on cuda:0 over gloo (RCCL refuses
    # two ranks on one device) — a one-GPU box can then execute the multi-rank branches of this file (both exchange modes, watchdog, max over ranks)
    rehearsal = os.environ.get("DCV_BENCH_REHEARSAL") == "gloo"
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist
    use_dp = world > 1 or args.force_dp
    rccl_log = None
    if use_dp:
        # RCCL's INIT log goes to a file (ONE JSON line on stdout): rank 0 parses the channel count actually set up from it
        rccl_log = f"/tmp/dcv_rccl_{os.getpid()}.log"
        os.environ["NCCL_DEBUG"] = os.environ.get("DCV_NCCL_DEBUG", "INFO")  # DCV_NCCL_DEBUG=WARN switches the channel report off
        os.environ.setdefault("NCCL_DEBUG_SUBSYS", "INIT,GRAPH")
        os.environ["NCCL_DEBUG_FILE"] = rccl_log
        if "MASTER_ADDR" not in os.environ:
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", "29655"
        from diverse_channel_vit_amd.dp import DataParallel as _DP
        _DP.limit_rccl_channels(_DP.reserved_cus)  # before the communicator exists; see dp.py
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    import diverse_channel_vit_amd as dcv
    from diverse_channel_vit_amd import hip
    hip.load()
    if args.atomic_reductions:
        hip.set_deterministic(False)

    if args.chammi:
        args.channels, args.classes = 12, 14
    cfg = model_cfg(args.arch, args.channels, args.img, 16, args.classes)
    if args.hcs:
        cfg.update(enable_sample=True, hcs_sampling="lowest_cosine_prob", hcs_sampling_temp=1000.0)
        import random
        random.seed(33978 + 21022023)  # same seed on every rank (dataset_utils.py:589): ranks draw the same subset
        torch.manual_seed(33978 + 21022023)
    torch.manual_seed(0)
    chammi_map = {"Allen": [0, 1, 2], "HPA": [3, 4, 5, 6], "CP": [7, 8, 9, 10, 11]}  # trainer.py:130-131
    model = dcv.dichavit(cfg, mapper=chammi_map if args.chammi else {"train": list(range(args.channels))}).to(dev)
    if args.wgrad_stream is not None:
        model.wgrad_stream = bool(args.wgrad_stream)
    model.train()
    dp = None
    if use_dp:  # INTEGRATION.md's call order: wrap, equalise, hook — all before the first forward
        dp = dcv.DataParallel(model, force_collectives=args.force_dp, grad_dtype=getattr(torch, args.grad_dtype), overlap=bool(args.overlap))
        dp.broadcast_parameters(0)
        dp.hook_misc_params()
    use_graph = args.graph and (world == 1) and not use_dp and not args.hcs and not args.chammi
    opt = dcv.HipAdamW([p for p in model.parameters() if p.requires_grad], lr=4.9e-5, betas=(0.9, 0.999), eps=1e-8,
                       weight_decay=0.04, model=model, capturable=use_graph)
    rs = np.random.RandomState(1234 + rank)
    x = torch.from_numpy(rs.standard_normal((args.batch, args.channels, args.img, args.img)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rs.randint(0, args.classes, args.batch)).to(dev)
    ce = torch.nn.CrossEntropyLoss()

    chunks = []
    if args.chammi:  # sub-batches of the three chunks (b/3 each, the remainder to the last), their own channel counts
        sizes = [args.batch // 3, args.batch // 3, args.batch - 2 * (args.batch // 3)]
        for (name, ids), bsz in zip(chammi_map.items(), sizes):
            chunks.append((name, torch.from_numpy(rs.standard_normal((bsz, len(ids), args.img, args.img)).astype(np.float32)).to(dev),
                           torch.from_numpy(rs.randint(0, args.classes, bsz)).to(dev)))

    last_out = {}  # the model output of the latest step, for --dump-outputs

    def chammi_step():
        opt.zero_grad()
        for name, xc, yc in chunks:  # trainer.py:846-935: one backward per chunk, gradients accumulate, one optimiser step
            feat, extra = model(xc, name, None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
            loss = dcv.proxy_loss(model.proxies, feat, yc, model.scale) + extra * 1.0
            loss.backward()
        opt.step()
        last_out["features"] = feat.detach()  # of the last chunk (detached: holds no autograd graph)
        return loss

    def eager_step():
        if args.chammi:
            return chammi_step()
        if use_graph:
            opt.advance()
        opt.zero_grad()
        out, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
        loss = ce(out, y) + extra * 1.0
        loss.backward()
        opt.step()
        last_out["logits"] = out.detach()
        return loss

    graphed = dcv.GraphedTrainStep(model, opt, "train", None, ce, 1.0) if use_graph else None
    step = eager_step

    def sync():
        torch.cuda.synchronize()
        if use_dp:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- warm-up: plain steps, then (--full) 1-2 fully profiled eager steps (every C-ABI launch bracketed by events) ----
    n_prof = (2 if args.warmup >= 3 else 1) if full else 0
    n_back = 1 if args.warmup > n_prof else 0  # the last warm-up step: after the profiled ones, in the timed region's configuration
    for _ in range(max(args.warmup - n_prof - n_back, 0)):
        step()
    two_streams = bool(model.wgrad_stream)
    if full:
        torch.cuda.synchronize()
        # the profiled steps run on ONE stream, so every launch's duration is its own (with the weight-gradient GEMMs on the second
        # stream the kernels of the two streams share the chip and their durations overlap: the table would add up to more than the step)
        model.wgrad_stream = False
        hip.set_profiler(True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_prof):
            step()
        e1.record()
        torch.cuda.synchronize()
        prof = hip.set_profiler(False)
        model.wgrad_stream = two_streams
    # A full (generation-2) pass of Python's cyclic collector over everything torch has imported and built by now takes ~110 ms on this
    # host and used to fire inside the timed region (always at the 7th timed step): one 120 ms step at batch 16, absorbed by the launch
    # queue at batch 64.  Collect now and park the survivors in the permanent generation: the collector stays ON, later passes only
    # look at objects created from here on.  Done BEFORE the last warm-up step so that the GPU is not idle right before the timed region.
    import gc
    gc.collect()
    gc.freeze()
    if n_back:
        step()  # the timed region's configuration (two streams again), counted in --warmup
    if full:
        prof_step_ms = e0.elapsed_time(e1) / n_prof
        table = table_from(prof, n_prof, prof_step_ms)
        by_symbol = {}
        for r in table:
            by_symbol[r["symbol"]] = by_symbol.get(r["symbol"], 0.0) + r["ms_per_step"]
        dominant = max(by_symbol, key=by_symbol.get)
        if args.kernel_table and rank == 0:
            for r in table:
                print(f"  {r['symbol']:28s} {r['shape']:26s} x{r['launches_per_step']:5.1f} {r['avg_us']:8.1f} us  {r['ms_per_step']:7.3f} ms/step "
                      f"{100 * r['share_of_step']:5.1f} %  " + (f"{r.get('achieved_tflops', 0):7.1f} TF/s ({100 * r.get('frac', 0):4.1f} % alg / "
                      f"{100 * r.get('frac_executed', 0):4.1f} % exec, {r.get('flop_per_byte')} FLOP/B -> {r.get('bound')})" if r.get("gflop") else f"{r.get('achieved_gbps', 0):7.0f} GB/s"), file=sys.stderr)

    # ---- timed region: EXACTLY K steps; (--full) events only around the dominant symbol's launches (eager) ----
    if use_graph:
        graphed(x, y)  # capture (plus its own eager warm-up steps)
        step = lambda: graphed(x, y)  # noqa: E731
        step()
    if args.h2d:
        xh, yh = x.cpu().pin_memory(), y.cpu().pin_memory()
        bufs = [(torch.empty_like(x), torch.empty_like(y)) for _ in range(2)]
        copy_stream = torch.cuda.Stream()
        landed = [torch.cuda.Event() for _ in range(2)]
        consumed = [torch.cuda.Event() for _ in range(2)]
        state = {"i": 0}

        def prefetch(slot):
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(consumed[slot])  # the step that last read this buffer is done with it
                bufs[slot][0].copy_(xh, non_blocking=True)
                bufs[slot][1].copy_(yh, non_blocking=True)
                landed[slot].record(copy_stream)

        for ev in consumed:
            ev.record()
        prefetch(0)
        inner = graphed if use_graph else None

        def step():  # noqa: F811
            nonlocal x, y
            i = state["i"]; state["i"] += 1
            slot = i % 2
            prefetch(1 - slot)
            torch.cuda.current_stream().wait_event(landed[slot])
            x, y = bufs[slot]
            loss = inner(x, y) if inner is not None else eager_step()
            consumed[slot].record()
            return loss
    picks0 = syncs0 = 0

    def timed_region():
        """EXACTLY K steps between barrier + synchronize pairs; returns (seconds, median step ms, per-launch records of the dominant symbol)."""
        nonlocal picks0, syncs0
        syncs0 = model.host_syncs
        picks0 = sum(model.feature_extractor.patch_embed.counter.values()) if args.hcs else 0  # channel draws so far (HCS histogram)
        if full and not use_graph:
            hip.set_profiler(True, only=[dominant])
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        sync()
        t0 = time.perf_counter()
        marks[0].record()
        loss_ = None
        for i in range(args.steps):
            loss_ = step()
            marks[i + 1].record()
        sync()
        dt_ = time.perf_counter() - t0
        live_ = hip.set_profiler(False) if full and not use_graph else None
        step_ms_ = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
        med_ = float(np.median(step_ms_))
        if os.environ.get("DCV_BENCH_STEP_TIMES") and rank == 0:
            print("step ms:", " ".join(f"{v:.1f}" for v in step_ms_), file=sys.stderr)
        if use_dp:
            t = torch.tensor([dt_, med_], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt_, med_ = t[0].item(), t[1].item()
        return dt_, med_, live_, loss_

    # N > 1: BOTH exchange modes are timed in this one invocation, same process group, K steps each — the overlapped
    # per-layer buckets first (north_star's mode and the library default), then one all-reduce after the backward; `value` is the better of
    # the two and `dp.modes` carries both.  --overlap / --no-overlap restrict the run to one mode.
    dp_modes = {}
    if dp is not None and not (args.overlap or args.no_overlap):
        order = [True, False]
    else:
        order = [bool(args.overlap) if dp is not None and (args.overlap or args.no_overlap) else (dp.overlap if dp is not None else None)]
    def full_fields(dt, live, headline):
        """--full: the roofline of the dominant symbol, the step's roofline and the per-symbol table."""
        # ---- roofline of the dominant symbol ----
        src = live if live is not None else prof
        recs = [(k, r) for k, r in src.items() if k[0] == dominant and r["ev"]]
        ev_ms = [s.elapsed_time(e) for _, r in recs for s, e in r["ev"]]
        n_l = len(ev_ms)
        avg_ms = float(np.mean(ev_ms))
        flops = sum(r["flops"] * len(r["ev"]) for _, r in recs) / n_l
        flops_exec = sum(r["flops_exec"] * len(r["ev"]) for _, r in recs) / n_l
        alg_bytes = sum(r["bytes"] * len(r["ev"]) for _, r in recs) / n_l
        where = ("HIP events around every launch of this symbol inside the timed region" if live is not None else
                 f"HIP events in the {n_prof} profiled eager warm-up step(s): the timed region replays a captured HIP graph")
        if flops > 0:
            ach = flops / (avg_ms * 1e-3)
            roof = {"bound": "mfma", "kernel": dominant, "achieved": round(ach / 1e12, 2), "peak": PEAK_BF16 / 1e12, "unit": "TFLOP/s",
                    "frac": round(ach / PEAK_BF16, 4), "executed_achieved": round(flops_exec / (avg_ms * 1e-3) / 1e12, 2),
                    "executed_frac": round(flops_exec / (avg_ms * 1e-3) / PEAK_BF16, 4),
                    "algorithmic_gflop_per_launch": round(flops / 1e9, 2), "executed_gflop_per_launch": round(flops_exec / 1e9, 2)}
        else:
            ach = alg_bytes / (avg_ms * 1e-3)
            roof = {"bound": "hbm", "kernel": dominant, "achieved": round(ach / 1e9, 1), "peak": PEAK_HBM / 1e9, "unit": "GB/s",
                    "frac": round(ach / PEAK_HBM, 4)}
        roof.update(traffic=None, algorithmic_bytes=round(alg_bytes), avg_launch_ms=round(avg_ms, 4), launches_timed=n_l,
                    share_of_step=round(by_symbol[dominant] / prof_step_ms, 4), measured=where)
        if two_streams and live is not None:
            # in the timed region the weight-gradient GEMMs run on a second stream beside the main stream's kernels: a launch's
            # duration there includes the time it shares the chip.  The one-stream profiled warm-up steps give the kernel alone.
            ex = [(r, [s_.elapsed_time(e_) for s_, e_ in r["ev"]]) for k, r in prof.items() if k[0] == dominant and r["ev"]]
            ex_n = sum(len(v) for _, v in ex)
            ex_ms = sum(sum(v) for _, v in ex) / ex_n
            ex_work = sum((r["flops"] if flops > 0 else r["bytes"]) * len(v) for r, v in ex) / ex_n
            roof.update(concurrent="timed launches overlap kernels of the other HIP stream (weight gradients on a second stream); "
                                   "exclusive_* = the same symbol in the one-stream profiled warm-up steps",
                        exclusive_avg_launch_ms=round(ex_ms, 4),
                        exclusive_frac=round(ex_work / (ex_ms * 1e-3) / (PEAK_BF16 if flops > 0 else PEAK_HBM), 4))
        # HBM bytes per launch of that symbol: PMC counters cannot be read from inside this process, so the figure comes from
        # the committed rocprofv3 --pmc passes over this same command at the headline configuration (tools/pmc_traffic.sh)
        pmc_path = newest_pmc_file() if headline else None
        pmc = {}
        if pmc_path:
            with open(pmc_path) as f:
                pmc = json.load(f)
            dom_key = dominant if dominant in pmc else dominant.split("<")[0]  # profiles older than the templated attention kernels
            if dom_key in pmc and dom_key != "_meta":
                v = pmc[dom_key]
                roof["traffic"] = round(v["read_bytes_per_launch"] + v["written_bytes_per_launch"])
                roof["traffic_unit"] = "bytes/launch (HBM, PMC: 2 x FETCH_SIZE + WRITE_SIZE)"
                roof["traffic_source"] = "profiles/" + os.path.basename(pmc_path)
                if dominant == "attn_bwd_dkdv3p_kernel":
                    # one dcv_attn_bwd_dkdv_rows_ps call = the persistent kernel + the second form's launch for the key remainder (N = 1569: 33 keys); the events
                    # bracket the call, rocprofv3 lists the two symbols separately
                    tails = [v for k, v in pmc.items() if k.startswith("attn_bwd_dkdv2_kernel<true, true>")]
                    if tails:
                        roof["traffic"] += round(tails[0]["read_bytes_per_launch"] + tails[0]["written_bytes_per_launch"])
                    roof["launch_includes"] = "attn_bwd_dkdv3p_kernel + attn_bwd_dkdv2_kernel<true, true> (key remainder) of one C-ABI call; rocprofv3 reports them as two symbols"
        # ---- the roofline that binds the STEP: executed FLOPs at the dense bf16 peak against HBM bytes (PMC, whole step)
        # at the HBM peak.  The PMC passes cover `steps` whole steps of this command (tools/pmc_traffic.sh: 2 timed + 1 warm-up).
        step_roof = None
        if pmc and headline:
            pmc_steps = (pmc.get("_meta") or {}).get("steps", 3)
            tot = sum((v["read_bytes_per_launch"] + v["written_bytes_per_launch"]) * v["launches"] for k, v in pmc.items() if k != "_meta") / pmc_steps
            step_ms_now = dt / args.steps * 1e3
            exec_flop = (TRAIN_GFLOP_PER_IMG - (DEAD_GFLOP_PER_IMG if model.cls_only_tail else 0.0)) * 1e9 * args.batch
            mfma_ms, hbm_ms = exec_flop / PEAK_BF16 * 1e3, tot / PEAK_HBM * 1e3
            step_roof = {"step_hbm_gbytes": round(tot / 1e9, 2), "step_hbm_floor_ms": round(hbm_ms, 2), "step_hbm_frac": round(hbm_ms / step_ms_now, 4),
                         "step_executed_tflop": round(exec_flop / 1e12, 2), "step_mfma_floor_ms": round(mfma_ms, 2), "step_mfma_frac": round(mfma_ms / step_ms_now, 4),
                         "step_bound": "hbm" if hbm_ms >= mfma_ms else "mfma", "step_frac_of_binding_roofline": round(max(hbm_ms, mfma_ms) / step_ms_now, 4),
                         "step_hbm_achieved_gbps": round(tot / (step_ms_now * 1e-3) / 1e9, 0),
                         "source": "HBM bytes: 2 x FETCH_SIZE + WRITE_SIZE summed over every kernel of a step, profiles/" + os.path.basename(pmc_path)}
        for r in table:  # per-symbol PMC traffic next to the algorithmic bytes (mean over the symbol's shapes in the PMC run)
            key = r["symbol"] if r["symbol"] in pmc else r["symbol"].split("<")[0]
            if key in pmc and key != "_meta":
                v = pmc[key]
                r["pmc_mbytes_per_launch"] = round((v["read_bytes_per_launch"] + v["written_bytes_per_launch"]) / 1e6, 1)
        # matrix-pipe utilisation per (symbol, shape) from the committed SQ-counter passes (tools/pmc_gemm.sh at the headline shapes):
        # mfma_busy_frac = SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 1024 SIMDs), the share of wall cycles the MFMA pipes are busy
        sq_files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_sq_counters.json")),
                          key=lambda f: int(re.match(r"r(\d+)_", os.path.basename(f)).group(1)))
        if headline and sq_files:
            with open(sq_files[-1]) as f:
                sq = json.load(f)
            for r in table:
                v = sq.get(f"{r['symbol']}|{r['shape']}")
                if v:
                    r["mfma_busy_frac"] = v["mfma_busy_frac"]
                    r["valu_mfma_coexec_frac"] = v["valu_mfma_coexec_frac"]
                    r["lds_bank_conflict_frac"] = round((v.get("lds_bank_conflict_cycles") or 0.0) / max(v.get("lds_active_cycles") or 1.0, 1.0), 4)
                    r["sq_counter_source"] = "profiles/" + os.path.basename(sq_files[-1])
        return {"roofline": roof, "step_roofline": step_roof,
                "kernel_table_mode": "per-launch durations from the profiled warm-up steps, run on one stream (exclusive); "
                                     "ms_per_step and share_of_step refer to that one-stream step",
                "kernel_table": table[:24]}

    def build_line(dt, med_ms, live, final_loss, chosen_mode):
        """The JSON line from one timed region (rank 0 only; None elsewhere)."""
        if rank != 0:
            return None
        B, C, H = args.batch, args.channels, {"tiny": 3, "small": 6, "base": 12, "distill": 6}[args.arch]
        headline = (args.arch, C, args.img, args.batch, args.classes) == ("small", 8, 224, 64, 161) and not args.hcs and not args.chammi
        n = (args.img // 16) ** 2
        N = C * n + 1
        exec_gf = TRAIN_GFLOP_PER_IMG - (DEAD_GFLOP_PER_IMG if model.cls_only_tail else 0.0)
        imgs = args.batch * world * args.steps / dt
        imgs_med = args.batch * world / (med_ms * 1e-3)
        small8 = (args.arch, C, args.img) == ("small", 8, 224)
        line = {
            "metric": ("train images/sec, DiChaViT-S 8ch 224^2 bs=64/GPU" if (args.arch, C, args.img, args.batch) == ("small", 8, 224, 64) and not args.chammi
                       else f"train images/sec, DiChaViT-{args.arch} CHAMMI 3/4/5ch {args.img}^2 bs={args.batch}/GPU" if args.chammi
                       else f"train images/sec, DiChaViT-{args.arch} {C}ch {args.img}^2 bs={args.batch}/GPU"),
            "value": round(imgs, 2), "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
            "median_ms_per_step": round(med_ms, 3), "value_median": round(imgs_med, 2),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": f"DiChaViT-{args.arch} {C}ch {args.img}x{args.img} P16 {args.classes} classes, train step "
                                   f"(fwd + CE + ortho/proxy regularisers + bwd + fused AdamW), bs {args.batch}/GPU, N={N} tokens",
                       "global_batch": args.batch * world, "seq_len": N, "parallelism": f"dp{world}",
                       # the reference's 336.94 GFLOP/img include the rows of the LAST block that never reach the output (everything
                       # after its attention on the non-CLS tokens, and all but the CLS query of that attention): 3 * (18 N D^2 +
                       # 4 N^2 D) (N-1)/N = 23.82 GFLOP/img that this path does not execute.  The fraction is quoted on EXECUTED FLOPs.
                       "step_roofline_frac": round(imgs / world * exec_gf * 1e9 / PEAK_BF16, 4) if small8 else None,
                       "executed_gflop_per_img": round(exec_gf, 2) if small8 else None,
                       "dead_rows": ("last block: token-wise ops after the attention on the CLS rows only, attention for the CLS query only "
                                     "(the encoder returns norm(x)[:, 0]; same outputs and gradients, DCV_CLS_TAIL=0 computes every row)"
                                     if model.cls_only_tail else "none skipped"),
                       "final_loss": round(final_loss, 5),
                       "input": ("pinned host memory -> HBM every step (copy stream, double-buffered)" if args.h2d else "resident in HBM"),
                       # synchronisations the model's own code causes per step (the reference's HCS branch moves the sampled subset to the host
                       # every step, dichavit.py:178/184/200; here it stays on the device unless DCV_HCS_ON_DEVICE=0)
                       "host_syncs_per_step": round((model.host_syncs - syncs0) / max(args.steps * len(order), 1), 3),
                       "launch": "hip-graph replay of the captured step" if use_graph else "eager",
                       "wgrad_stream": bool(model.wgrad_stream),
                       "wgrad_group": bool(model.wgrad_group and model.wgrad_private_scratch),  # a block's four weight gradients in one launch
                       "reductions": ("deterministic: partial sums through workspaces, fixed-order second pass (bit-reproducible gradients)"
                                      if hip.is_deterministic() else "fp32 atomics (order-dependent in the last bits; --atomic-reductions)"),
                       **({"hcs": "enable_sample lowest_cosine_prob temp 1000 (E[C] = 4.5 of 8 channels; img/s counts whole images)",
                           # the secondary run reports tokens/s too.  Tokens of a step = batch * (1 + C_step * n); the sum of
                           # C_step over the timed steps is the growth of the model's channel histogram (patch_embed.counter)
                           "channels_per_step": round((sum(model.feature_extractor.patch_embed.counter.values()) - picks0) / args.steps, 2),
                           "tokens_per_sec": round(args.batch * world * (args.steps + n * (sum(model.feature_extractor.patch_embed.counter.values()) - picks0)) / dt, 1)}
                          if args.hcs else {}),
                       **({"chammi": "12-channel model, sub-batches Allen 3ch / HPA 4ch / CP 5ch (N = 589 / 785 / 981 tokens), proxy main loss, "
                                     "3 forward/backward passes + 1 optimiser step per step; img/s counts the images of all three"} if args.chammi else {})},
        }
        if full:
            line.update(full_fields(dt, live, headline))
        if dp is not None:
            steps_run = args.warmup + args.steps
            line["dp"] = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "buckets_launched": dp.buckets_launched,
                          "buckets_per_step": round(dp.buckets_launched / max(steps_run, 1), 2),
                          "mbytes_reduced_per_step": round(dp.bytes_reduced / max(steps_run, 1) / 1e6, 2), "grad_dtype": args.grad_dtype,
                          "overlap": bool(chosen_mode), "modes": dp_modes,
                          "mode_choice": ("both exchange modes timed in this invocation (K steps each, same process group); value / ms_per_step are "
                                          "the faster one's" if len(dp_modes) > 1 else "one mode timed (--overlap / --no-overlap)"),
                          "rccl_channels_requested": os.environ.get("NCCL_MAX_NCHANNELS"),
                          "rccl_channels_in_use": None,  # filled in below, once the communicator is gone and its log complete
                          "reserved_cus": dp.reserved_cus}
        if full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(cfg, args.channels, args.img, args.classes)
        return line

    # N > 1: the single all-reduce after the backward is timed FIRST (the simple mode: nothing runs beside the backward), the overlapped
    # per-layer buckets second, under a watchdog: that mode has never met real asynchronous collectives on two devices (no such box in four
    # rounds) — if it does not finish, every rank prints / exits with the first mode's line instead of hanging the scaling run.
    if len(order) == 2:
        order = [False, True]
    best = None
    fallback = None
    for mi, mode in enumerate(order):
        if dp is not None:
            dp.overlap = bool(mode)
        watchdog = None
        wd_env = os.environ.get("DCV_BENCH_WATCHDOG_S")  # test hook: arms the watchdog at any world size with this limit
        if dp is not None and mi > 0 and (world > 1 or wd_env):
            import threading
            limit = float(wd_env) if wd_env else max(180.0, 30.0 * best[1][0])

            def bail(limit=limit):
                # a firing watchdog is a FINDING, not a success: the line carries a top-level status and what the reducer was waiting for
                # (ADVICE r4); the exit code stays 0 so that the driver still records the valid single-all-reduce measurement
                pending = None
                try:
                    pending = dp.pending_state()
                except Exception as e:  # the reducer may be mid-update in the main thread
                    pending = f"unavailable: {e!r}"
                if rank == 0 and fallback is not None:
                    fallback["status"] = "overlap_hang"
                    fallback["dp"]["modes"]["overlap"] = {"status": f"did not finish within {limit:.0f} s: the line reports the single all-reduce mode",
                                                          "pending": pending}
                    fallback["dp"]["rccl_channels_in_use"] = dcv.DataParallel.rccl_channels_from_log(rccl_log) if rccl_log else None
                    print(json.dumps(fallback), flush=True)
                os._exit(0)

            watchdog = threading.Timer(limit, bail)
            watchdog.daemon = True
            watchdog.start()
        if dp is not None and mi > 0:
            for _ in range(2):  # untimed: the first steps in a mode allocate its buffers
                step()
        r = timed_region()
        if watchdog is not None:
            watchdog.cancel()
        if dp is not None:
            dp_modes["overlap" if mode else "single_allreduce_after_backward"] = {
                "images_per_sec": round(args.batch * world * args.steps / r[0], 2), "ms_per_step": round(r[0] / args.steps * 1e3, 3),
                "median_ms_per_step": round(r[1], 3)}
        if best is None or r[0] < best[1][0]:
            best = (mode, r)
        if dp is not None and mi == 0 and len(order) > 1 and (world > 1 or wd_env):
            fallback = build_line(r[0], r[1], r[2], r[3].item(), mode)
    chosen_mode, (dt, med_ms, live, loss) = best
    final_loss = loss.item()
    line = build_line(dt, med_ms, live, final_loss, chosen_mode)  # None on every rank but 0
    if line is not None:
        line["status"] = "ok"
    if args.dump_outputs and rank == 0:
        out_name, out = ("logits", graphed.static_out) if use_graph else next(iter(last_out.items()))
        dump_outputs(args.dump_outputs, loss, out_name, out, model)
    if use_dp:
        dist.barrier()
        dist.destroy_process_group()
        if rank == 0 and rccl_log:
            line["dp"]["rccl_channels_in_use"] = dcv.DataParallel.rccl_channels_from_log(rccl_log)
        if rccl_log:
            try:
                os.remove(rccl_log)
            except OSError:
                pass
    if rank == 0:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
