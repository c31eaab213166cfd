"""A/B of the 256 x 384 NT GEMM's balanced tile plan (192-row tiles in the last round, dcv_gemm_nt384_plan) against the -DDCV_N3_BALANCE=0 build of
the same sources (256-row tiles only), at the headline step's M = 100 416.  One process, the two libraries alternating; per entry the median
microseconds of both builds, the spread of the baseline between its alternations, and the tile-time ratio the pair implies: the old plan is
two rounds of 256-row tiles, the new one a 256-row round and a 192-row round, so t192 / t256 = 2 T_new / T_old - 1.
  python tools/gemm_balance_bench.py --build     (no GPU needed: builds libdcv_hip_n3_balance0.so)
  python tools/gemm_balance_bench.py             (on the GPU)"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diverse_channel_vit_amd import _build, hip  # noqa: E402

VARIANT = "n3_balance0"
ap = argparse.ArgumentParser()
ap.add_argument("--build", action="store_true", help="build the baseline variant and exit")
ap.add_argument("--rounds", type=int, default=14, help="alternations per entry (the first two are warm-up)")
ap.add_argument("--launches", type=int, default=5, help="launches per alternation and build")
args = ap.parse_args()
base_path = os.path.join(os.path.dirname(hip.LIB_PATH), f"libdcv_hip_{VARIANT}.so")
if args.build:
    _build.build_variant(VARIANT, ["DCV_N3_BALANCE=0"])
    sys.exit(0)

import torch  # noqa: E402


def load(path):
    lib = C.CDLL(path)
    for name, (a, r) in hip._SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = a, r
    return lib


libs = {"base": load(base_path), "new": hip.load()}
M, D = 64 * 1569, 384
for name, lib in libs.items():
    a, b = C.c_int(), C.c_int()
    lib.dcv_gemm_nt384_plan(M, D, 256, C.byref(a), C.byref(b))
    print(f"{name}: plan(M {M}, N 384, grid 256) = ({a.value} x 256, {b.value} x 192)")
bf = torch.bfloat16
torch.manual_seed(0)
acts = {K: torch.randn(M, K, device="cuda").to(bf) for K in (D, 3 * D, 4 * D)}
bias, gamma, beta = torch.zeros(D, device="cuda"), torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
resid = torch.randn(M, D, device="cuda")
x_out, u = torch.empty(M, D, device="cuda"), torch.empty(M, D, dtype=bf, device="cuda")
mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
out = torch.empty(M, D, dtype=bf, device="cuda")
p, st = hip._p, hip._stream


def ln_entry(K):
    W = (torch.randn(D, K, device="cuda") * 0.05).to(bf)
    A = acts[K]
    return lambda lib: lib.dcv_gemm_nt_resid_ln(p(A), K, p(W), K, M, D, K, p(bias), p(resid), D, None, 0, p(x_out), D, p(gamma), p(beta), 1e-6,
                                                p(u), D, p(mean), p(rstd), 0, st())


def plain_entry(K, tile):
    W = (torch.randn(D, K, device="cuda") * 0.05).to(bf)
    A = acts[K]
    return lambda lib: lib.dcv_gemm_nt_ex(p(A), K, p(W), K, M, D, K, hip.EPI_PLAIN_BF16, None, p(out), D, None, 0, None, 0, None, 0, 0, 0, tile, st())


entries = [("proj + resid + LN   N384 K384  wide", ln_entry(D)), ("fc2 + resid + LN    N384 K1536 wide", ln_entry(4 * D)),
           ("dgrad fc1T plain    N384 K1536 wide", plain_entry(4 * D, hip.TILE_WIDE)),
           ("dgrad qkvT plain    N384 K1152 wide (forced; AUTO stays narrow)", plain_entry(3 * D, hip.TILE_WIDE)),
           ("dgrad qkvT plain    N384 K1152 narrow (same kernel in both builds)", plain_entry(3 * D, hip.TILE_NARROW))]
for name, call in entries:
    res = {k: [] for k in libs}
    for rnd in range(args.rounds):
        for k, lib in libs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.launches):
                rc = call(lib)
            e.record()
            torch.cuda.synchronize()
            assert rc == 0, (name, k, rc)
            if rnd >= 2:
                res[k].append(s.elapsed_time(e) * 1e3 / args.launches)
    tb, tn = float(np.median(res["base"])), float(np.median(res["new"]))
    spread = max(res["base"]) - min(res["base"])
    print(f"{name:70s} base {tb:7.1f} us (alternations {min(res['base']):.1f} .. {max(res['base']):.1f}, spread {spread:.1f})   new {tn:7.1f} us "
          f"({min(res['new']):.1f} .. {max(res['new']):.1f})   gain {tb - tn:+6.1f} us = {100 * (tb - tn) / tb:+5.1f} %   "
          f"t192/t256 = {2 * tn / tb - 1:.3f}   {'improved' if tb - tn > spread else 'within the baseline spread'}", flush=True)
