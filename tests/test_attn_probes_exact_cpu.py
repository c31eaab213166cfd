"""The attention probe kernels (csrc/attn_probs.hip, attn_channel_mass.hip, attn_rollout.hip) on operands for which the ideal softmax is exactly 1, 1/2, 1/4
or 0: the operand builder, the closed-form expectations, the comparison rules of tests/test_attn_probes_exact_gpu.py, pure-Python restatements of the kernels'
walks with the regimes the case tables reach, and the proof, without a GPU and without the library, that the rules flag structural defects.

Operands.  The "group" operands of tests/test_attn_exact_cpu.py (structure(): keys in groups of 1, 2 or 4, k[:, :12] the +-1 code of the key's group, q[:, :12]
BETA = 512 times the code of the row's target group, scale 1/8): the keys of the target group tie, every other key lies at least 185 log2 units below and its
exp2 is exactly zero in fp32.  v and dO play no part.  The payloads that make a head mix-up visible in the forward tests do not reach P, so here EVERY (batch,
head) has its own structure (the seed argument): any two pairs of a case differ in the target group of at least half of their rows (asserted below for N >= 8;
with fewer keys there are too few partitions: N = 1 has one), so another head's K, Q or LSE is visible.  Rows >= Nq of q are zero and their LSE is 0: a row the
kernel must not write would be written as exp2(0) = 1, finite, into NaN.
LSE is an INPUT of these kernels: the tests give them the float32 rounding of the closed form SCALE qamp 12 + ln g (qamp: BETA; pre-scaled form bf16(BETA C) / C,
C = scale log2 e), so the result does not depend on the forward kernel; one small test per kernel takes LSE from hip.attn_fwd instead (the model's chain).

Expectations (float64, gathers and index_add over the groups; g = size of the row's target group):
  P[b,h,q,k] = 1 / g for k in the target group of row q, else 0
  T[b,h,q,j] = (keys of that group in segment S_j) / g;  A[b,h,i,j] = mean of T over the rows of S_i
  out[b,k]   = alpha w_k + (1 - alpha) / H sum_h (1 / g) sum of w_q over the rows q whose target group in head h holds k
The rollout weights are drawn from {0, 1/4, 1/2, 1, 2} (log2f exact); the "sparse" draw has at least a quarter of its rows zero and, for N > 128, the whole
second 64-query tile (the -inf row constant for a whole tile); w[N - 1] > 0 for N >= 2, so a clamped query row past N that leaked would show.  A "dense" draw
without zeros runs beside it (the sparse draw of N = 1 is w = 0).  alpha in {0, 0.5, 0.75}.

Rules (rule()).  Expectation zero: |got| <= DUST = 2^-30.  Elsewhere |got - ref| <= (2^-10 + n 2^-24) ref, n the number of summed terms: 0 for P, 4 for T, n_p
for A, the number of contributing (weight > 0) rows for out.  NaN always fails.  Where 2^-10 comes from, in log2 units of the exponent of exp2, which is formed
at magnitude about 1110 where an fp32 ulp is 2^-13:
  * the float32 LSE given to the kernel: half an ulp of 768 nats = 2^-15 nats = 4.4e-5 log2 units;
  * rowc = fl(-lse LOG2E) (attn_probs.hip:63, attn_channel_mass.hip:69, attn_keysweep_kernel's sC row constant): half an ulp of 1108 = 2^-14 = 6.1e-5;
  * the fp32 constants LOG2E and c = scale LOG2E (attn_probs.hip:105): each at most 2^-24 relative of about 1108, 1.3e-4 between them;
  * the rollout's c_q = fl(log2f(w) - lse LOG2E) (attn_keysweep_kernel's sC row constant): where the product is not contracted into the subtraction, half an ulp more, 6.1e-5;
  * plain form, exp2(fma(s, c, rowc)) (attn_probs.hip:89, attn_channel_mass.hip:103, attn_keysweep_kernel's exp2(fma(...)) line): one rounding of a difference of magnitude <= 2, nothing;
    in all 3.1e-4 log2 units = 2.1e-4 relative on p;
  * pre-scaled form, the accumulator starts at rowc = -1110 - log2 g and takes up to twelve products of +-92.5 (the MFMA's order of accumulation is not
    specified): each partial sum has magnitude <= 1112 and rounds by at most 2^-14: 12 x 6.1e-5 = 7.3e-4 on top of the first three terms less the constant c,
    at most 9e-4 log2 units = 6.3e-4 relative on p.
v_exp_f32 itself is good to one ulp (1.2e-7).  2^-10 = 9.8e-4 covers both forms.  The plain form's part is repeated below as a float32 emulation and asserted
inside the bound.  The sums add n 2^-24: a chain of n fp32 adds of non-negative terms; the handful of further roundings (fl((1 - alpha) / H), the half-wave
add, the final fma, 1 / n_p) are 6e-8 each against the 3.5e-4 the exponent budget leaves unused.  The smallest structural change — one key or one row of a
group of four — is a quarter of a term: 250 times the bound.
With LSE from hip.attn_fwd the bound is 2^-10 + LSE_ULPS 2^-14: the forward's LSE is held to LSE_ULPS fp32 ulps of 768 nats (2^-14 each), and p moves by
that many nats, relatively.
A against T: |A - mean64(T)| <= n_p 2^-24 max(T) at every shape (mean64: the float64 segment mean of the kernel's own T, max(T) the largest element of that
T: the n_p - 1 adds of the row chain, the slot adds of zeros being exact, and fl(1 / n_p) and the product, each 2^-24 of a partial sum <= n_p max(T), over
n_p); A[:, :, 0] equals T[:, :, 0] bit for bit (len 1: 0 + x and x * 1.0f).
Buffers: every output lies in a NaN-prefilled buffer with 4096 guard floats before and after; afterwards the interior is finite, the guards are NaN.

Regimes (the walks restated below; asserted in test_the_tables_reach_every_regime).
  channel-mass sweep, C in {1, 2, 3, 5, 8} x n_p in 1..130 (650 shapes, N <= 1041): a segment boundary on every residue mod 32; blocks inside the running
    segment (whole), whole blocks whose segment ends with them (whole + flush, attn_channel_mass.hip:106-109) at 33 shapes, among them (1,63), (1,95), (1,127),
    (2,63), (3,53); crossing blocks with 1 .. 9 flushes; segments that go on into the next block; last blocks with keys past N.  The seven shapes of
    tests/test_channel_attention_gpu.py reach no whole + flush: the gap this module closes.
  channel-mass table: (8,196) at B 2, H 6; (15,49) and (7,169) on the whole + flush path; (64,1), (12,4) with 32 and 8 flushes per block; (255,1), (256,1),
    (300,1), (257,2): 1 + C = 256, 257, 301, 258 columns, the mean kernel's second column pass with 1, 45 and 2 columns and R = 1; (1,1).
  mean kernel: R = 256 / min(W, 256) row slots from 128 (W 2) to 1; segments shorter than R, equal and longer (several rows per slot); one and two passes.
  probabilities: every N to 330 (nt 1 .. 6, every N mod 32 and mod 64, idle waves, the skipped second key block), partial query tiles Nq in {2, 31, 33, 127,
    129, 130} against whole ones {32, 128, 160}, Nq = 1 at N = 1569, B 3 x H 5 workgroups.
  rollout: every N to 400 at H = 3 (1 .. 4 key workgroups, clamped query rows in the last tile, the skipped second query block), zero tiles from N = 129 on,
    H = 6 and 12, N = 1569.

A finding of the restatement: dropping the flush of the whole path is NOT what shifts every later segment — the crossing loop of the next block (its first
pass adds nothing, the segment has ended, it flushes) repairs it; only when the block is the last one of the sweep does the segment stay unwritten
((1,63), (1,95), (1,127): NaN in the prefilled buffer).  A flush placed before the adds does move the block's mass into the next channel.  Both are injected below.

Measured on the MI355X: see the docstring of tests/test_attn_probes_exact_gpu.py."""
import math
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_attn_exact_cpu import BETA, C as QC, DUST, LOG2E, LSE_ULPS, SCALE, structure  # noqa: E402

REL = 2.0 ** -10
ADD = 2.0 ** -24
REL_FWD = REL + LSE_ULPS * 2.0 ** -14  # LSE from hip.attn_fwd: see the module docstring
GUARD = 4096
QAMP_PS = float(torch.tensor(BETA * QC).to(torch.bfloat16)) / QC  # what the pre-scaled kernels see, unscaled: 92.5 / C
ALPHAS = (0.0, 0.5, 0.75)
W_VALUES = (0.0, 0.25, 0.5, 1.0, 2.0)


def _chunks(xs, n):
    return [xs[i:i + n] for i in range(0, len(xs), n)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Case tables.
MASS_SWEEP = [(c, n_p) for c in (1, 2, 3, 5, 8) for n_p in range(1, 131)]
MASS_SWEEP_CHUNKS = _chunks(MASS_SWEEP, 82)
MASS_TABLE = [(2, 6, 8, 196), (2, 3, 15, 49), (1, 2, 7, 169), (1, 2, 64, 1), (2, 2, 12, 4), (1, 2, 255, 1), (1, 2, 256, 1), (1, 2, 300, 1), (1, 2, 257, 2),
              (2, 2, 1, 1)]  # (B, H, C, n_p)
MASS_FWD = [(1, 2, 15, 49), (1, 2, 1, 63), (1, 2, 257, 2), (2, 6, 8, 196)]
OLD_MASS_SHAPES = [(1, 1), (12, 4), (64, 1), (5, 16), (3, 36), (2, 64), (8, 196)]  # tests/test_channel_attention_gpu.py
NAMED_WHOLE_FLUSH = [(1, 63), (1, 95), (1, 127), (2, 63), (3, 53)]

PROBS_SWEEP = list(range(1, 331))
PROBS_SWEEP_CHUNKS = _chunks(PROBS_SWEEP, 83)
PROBS_TABLE = [(1, 2, N, Nq) for N, Nq in ((200, 2), (200, 31), (200, 32), (200, 33), (300, 127), (300, 128), (300, 129), (300, 160), (1569, 1), (1569, 130))]
PROBS_TABLE += [(3, 5, 300, None)]  # (B, H, N, Nq)
PROBS_FWD = [(1, 2, 200, 33), (1, 2, 300, 129), (3, 5, 300, None), (1, 2, 65, None)]

ROLLOUT_SWEEP = list(range(1, 401))
ROLLOUT_SWEEP_CHUNKS = _chunks(ROLLOUT_SWEEP, 80)
ROLLOUT_TABLE = [(3, 6, 257), (2, 12, 197), (1, 6, 1569)]  # (B, H, N)
ROLLOUT_FWD = [(3, 6, 257), (2, 12, 197), (1, 3, 129), (1, 3, 64)]

# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Operands: B * H structures, one per (batch, head).
ProbeOps = namedtuple("ProbeOps", "B H N Nq sts")
_ops = {}


def probe_ops(B, H, N, Nq=None):
    key = (B, H, N, Nq)
    if key not in _ops:
        _ops[key] = ProbeOps(B, H, N, N if Nq is None else Nq, [structure(N, Nq, seed=1 + n) for n in range(B * H)])
    return _ops[key]


def row_keys(st):
    """[Nq, 4]: the keys of each row's target group, ascending, padded with -1 — what "the target group of a row" is across structures."""
    G = len(st.gsize)
    keys = torch.full((G, 4), -1, dtype=torch.long)
    order = torch.argsort(st.gid, stable=True)  # keys by group, ascending inside a group
    first = torch.zeros(G, dtype=torch.long)
    first[1:] = st.gsize.cumsum(0)[:-1]
    sg = st.gid[order]
    keys[sg, torch.arange(st.N) - first[sg]] = order
    return keys[st.tgt]


def device_qkv(ops, prescaled):
    """qkv [B, N, 3 H 64] bf16 as the kernels read it: q rows >= Nq zero, k the group code and 0 / 1 payloads the scores do not see, v zero."""
    B, H, N, Nq = ops.B, ops.H, ops.N, ops.Nq
    t = torch.zeros(B, N, 3, H, 64)
    g = torch.Generator().manual_seed(977 * N + H)
    t[:, :, 1, :, 12:] = torch.randint(0, 2, (B, N, H, 52), generator=g).float()
    for n, st in enumerate(ops.sts):
        q = (BETA * st.code[st.tgt]).float()
        t[n // H, :Nq, 0, n % H, :12] = (q * QC).to(torch.bfloat16).float() if prescaled else q
        t[n // H, :, 1, n % H, :12] = st.code[st.gid].float()
    return t.reshape(B, N, 3 * H * 64).to(torch.bfloat16)


def closed_lse(ops, prescaled):
    """[B, H, N] float32: the rounding of SCALE qamp 12 + ln g; rows >= Nq hold 0 (see the module docstring)."""
    lse = torch.zeros(ops.B * ops.H, ops.N, dtype=torch.float64)
    for n, st in enumerate(ops.sts):
        lse[n, :ops.Nq] = SCALE * (QAMP_PS if prescaled else BETA) * 12 + st.gsize[st.tgt].double().log()
    return lse.float().reshape(ops.B, ops.H, ops.N)


def p_ref(ops):
    """[B, H, Nq, N] float64."""
    out = [(st.gid[None, :] == st.tgt[:, None]).double() / st.gsize[st.tgt].double()[:, None] for st in ops.sts]
    return torch.stack(out).reshape(ops.B, ops.H, ops.Nq, ops.N)


def segment_of(N, n_p):
    seg = (torch.arange(N) - 1).div(n_p, rounding_mode="floor") + 1
    seg[0] = 0
    return seg


def t_ref(ops, C_, n_p):
    """[B, H, N, 1 + C] float64."""
    N, W = ops.N, 1 + C_
    assert N == 1 + C_ * n_p and ops.Nq == N
    seg = segment_of(N, n_p)
    out = []
    for st in ops.sts:
        cnt = torch.zeros(len(st.gsize), W, dtype=torch.float64).index_put_((st.gid, seg), torch.ones(N, dtype=torch.float64), accumulate=True)
        out.append(cnt[st.tgt] / st.gsize[st.tgt].double()[:, None])
    return torch.stack(out).reshape(ops.B, ops.H, N, W)


def seg_mean64(T, C_, n_p):
    """The float64 segment mean over the query rows: [..., N, W] -> [..., 1 + C, W]."""
    T = T.double()
    return torch.cat([T[..., :1, :], T[..., 1:, :].reshape(*T.shape[:-2], C_, n_p, T.shape[-1]).mean(-2)], dim=-2)


def rollout_weights(B, N):
    """{"sparse", "dense"}: [B, N] float32 from W_VALUES; see the module docstring."""
    g = torch.Generator().manual_seed(31 * N + B)
    vals = torch.tensor(W_VALUES)
    dense = vals[torch.randint(1, 5, (B, N), generator=g)]
    sparse = vals[torch.randint(1, 5, (B, N), generator=g)]
    nz = -(-N // 4)
    for b in range(B):
        rows = torch.randperm(N - 1, generator=g)[:nz] if N > 1 else torch.zeros(1, dtype=torch.long)  # never row N - 1 (N >= 2)
        sparse[b, rows] = 0.0
    if N > 128:
        sparse[:, 64:128] = 0.0
    return dict(sparse=sparse, dense=dense)


def out_ref(ops, w, alpha):
    """out [B, N] float64 and the number of contributing rows per element [B, N]."""
    B, H, N = ops.B, ops.H, ops.N
    w = w.double()
    out, cnt = alpha * w, torch.zeros(B, N, dtype=torch.float64)
    for n, st in enumerate(ops.sts):
        b, G = n // H, len(st.gsize)
        gs = torch.zeros(G, dtype=torch.float64).index_add_(0, st.tgt, w[b])
        gc = torch.zeros(G, dtype=torch.float64).index_add_(0, st.tgt, (w[b] > 0).double())
        out[b] += (1 - alpha) / H * (gs / st.gsize.double())[st.gid]
        cnt[b] += gc[st.gid]
    return out, cnt


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The comparison rules.
def rule(got, ref, n=0, rel=REL):
    """(mask of failing elements, largest err / bound).  ref zero: |got| <= DUST; else |got - ref| <= (rel + n 2^-24) ref.  NaN fails.  n: a number or a tensor."""
    ref = ref.double()
    bound = torch.where(ref != 0, ref * (rel + ADD * torch.as_tensor(n, dtype=torch.float64)), torch.full_like(ref, DUST))
    ratio = (got.double() - ref).abs() / bound
    bad = ~(ratio <= 1)
    return bad, float(torch.nan_to_num(ratio, nan=math.inf).max()) if ratio.numel() else 0.0


def mean_rule(A, T, C_, n_p):
    """A against the float64 segment mean of the kernel's own T: (mask, largest err / bound, A[..., 0, :] is T[..., 0, :] bit for bit)."""
    bound = max(n_p * ADD * float(T.max()), 0.0)
    err = (A.double() - seg_mean64(T, C_, n_p)).abs()
    bad = ~(err <= bound)
    return bad, float(torch.nan_to_num(err, nan=math.inf).max()) / bound if bound else math.inf, torch.equal(A[..., 0, :], T[..., 0, :])


def guarded_nan(n, device=None):
    buf = torch.full((GUARD + n + GUARD,), float("nan"), device=device)
    return buf, buf[GUARD:GUARD + n]


def buffer_findings(name, buf, n):
    """The interior all finite, both guards all NaN."""
    out = []
    if not bool(torch.isfinite(buf[GUARD:GUARD + n]).all()):
        out.append(f"{name}: {int((~torch.isfinite(buf[GUARD:GUARD + n])).sum())} elements of the output were not written (or not finite)")
    if not bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all()):
        out.append(f"{name}: written outside the output")
    return out


def where_bad(name, bad, ratio):
    if not bool(bad.any()):
        return []
    return [f"{name}: {int(bad.sum())} elements outside the bound (largest err / bound {ratio:.3g}); first at {[tuple(i) for i in bad.nonzero()[:4].tolist()]}"]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The walks, restated.
def acc_row(r, h):
    """dcv_common.hpp:56: register r of half-wave h is row (here: key or query) acc_row of the 32 x 32 accumulator."""
    return (r & 3) + 8 * (r >> 2) + 4 * h


MassBlock = namedtuple("MassBlock", "key0 kind flushes goes_on past_n")


def mass_walk(C_, n_p):
    """attn_channel_mass.hip:74-121 for one wave.  Returns the 32-key blocks (kind: "whole", "whole+flush", "cross"; the flushes in the block; whether the
    running segment goes on into the next block; keys past N in the block) and the stores (segment, first key, end key) in order."""
    N = 1 + C_ * n_p
    cur, lo, hi = 0, 0, 1
    blocks, stores = [], []

    def flush():
        nonlocal cur, lo, hi
        if cur <= C_:
            stores.append((cur, lo, hi))
        cur, lo, hi = cur + 1, hi, hi + n_p

    for t in range(-(-N // 64)):
        for kb in range(2):
            key0 = t * 64 + kb * 32
            if key0 >= N:  # :96
                break
            kend = min(key0 + 32, N)
            assert lo <= key0  # :105's comment
            if hi >= key0 + 32:  # :105 whole
                if hi == key0 + 32:  # :109
                    flush()
                    blocks.append(MassBlock(key0, "whole+flush", 1, False, 0))
                else:
                    blocks.append(MassBlock(key0, "whole", 0, True, 0))
            else:
                n, goes_on = 0, False
                while True:  # :111-119
                    if hi > kend:
                        goes_on = True
                        break
                    flush()
                    n += 1
                    if lo >= kend:
                        break
                blocks.append(MassBlock(key0, "cross", n, goes_on, key0 + 32 - kend))
    return blocks, stores


def mean_plan(C_, n_p):
    """attn_channel_mean_kernel (attn_channel_mass.hip:128-152): columns per pass, row slots, passes, columns of the last pass, rows of the fullest slot."""
    W = C_ + 1
    Wc = min(W, 256)
    R = 256 // Wc
    passes = -(-W // Wc)
    return dict(Wc=Wc, R=R, passes=passes, last_cols=W - (passes - 1) * Wc, slot_rows=-(-n_p // R))


def probs_plan(N, Nq=None):
    """attn_probs.hip:43-65, 76-78: workgroups per (batch, head), key tiles, and per wave of the last workgroup full / partial / idle."""
    Nq = N if Nq is None else Nq
    nqt = -(-Nq // 128)
    waves = []
    for wv in range(4):
        q0 = (nqt - 1) * 128 + wv * 32
        waves.append("idle" if q0 >= Nq else "full" if q0 + 32 <= Nq else "partial")
    return dict(nqt=nqt, nt=-(-N // 64), waves=waves, key_tail=N % 32, second_block_skipped=0 < N % 64 <= 32)


def rollout_plan(N):
    """attn_keysweep_kernel (attn_rollout.hip), its nkt, nt, k0 / active and the break of the qb loop: key workgroups per image, query tiles, clamped query rows of the last tile, idle waves, the skipped second query block."""
    nkt, nt = -(-N // 128), -(-N // 64)
    idle = sum(1 for wv in range(4) if (nkt - 1) * 128 + wv * 32 >= N)
    return dict(nkt=nkt, nt=nt, clamped=nt * 64 - N, idle_waves=idle, second_block_skipped=0 < N % 64 <= 32, key_tail=N % 32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Float64 emulations of the kernels' bookkeeping on a materialised P, optionally with one defect.
HALF_KEYS = [[acc_row(r, h) for r in range(16)] for h in range(2)]


def emulate_mass(P, C_, n_p, defect=None):
    """P [N, N] float64 -> T [N, 1 + C] in a NaN-prefilled array.  The two half-waves' partials are kept apart as the kernel keeps them.  defect:
      "whole_flush_dropped"  :109 missing             "flush_before_adds"  :109 placed before :108
      "le"                   :115 with <= for <       "past_n"             keys past N (clamped copies of key N - 1) added in the last block
      "no_upper_half"        sum_halves returns the lower half's partial alone"""
    N, W = P.shape[1], 1 + C_
    T = torch.full((P.shape[0], W), float("nan"), dtype=torch.float64)
    acc = torch.zeros(2, P.shape[0], dtype=torch.float64)
    cur, lo, hi = 0, 0, 1

    def flush():
        nonlocal cur, lo, hi
        if cur <= C_:
            T[:, cur] = acc[0] + (0 if defect == "no_upper_half" else acc[1])
        acc.zero_()
        cur, lo, hi = cur + 1, hi, hi + n_p

    for key0 in range(0, N, 32):
        kend = min(key0 + 32, N)
        if hi >= key0 + 32:
            if hi == key0 + 32 and defect == "flush_before_adds":
                flush()
            for h in range(2):
                acc[h] += P[:, [key0 + o for o in HALF_KEYS[h]]].sum(1)
            if hi == key0 + 32 and defect not in ("whole_flush_dropped", "flush_before_adds"):
                flush()
        else:
            while True:
                for h in range(2):
                    for o in HALF_KEYS[h]:
                        key = key0 + o
                        inside = lo <= key <= hi if defect == "le" else lo <= key < hi
                        if defect == "past_n" and key >= N and hi == N:
                            inside = True
                        if inside:
                            acc[h] += P[:, min(key, N - 1)]
                if hi > kend:
                    break
                flush()
                if lo >= kend:
                    break
    return T


def emulate_mean(T, C_, n_p, defect=None):
    """T [N, W] -> A [W, W] in a NaN-prefilled array, slot by slot.  defect: "slot_last_row_dropped" (a slot with several rows loses its last),
    "second_pass_skipped" (columns from 256 on are not written)."""
    W = C_ + 1
    pl = mean_plan(C_, n_p)
    A = torch.full((W, W), float("nan"), dtype=torch.float64)
    for i in range(W):
        lo, ln = (0, 1) if i == 0 else (1 + (i - 1) * n_p, n_p)
        for j0 in range(0, W, pl["Wc"]):
            if j0 and defect == "second_pass_skipped":
                break
            tot = torch.zeros(min(pl["Wc"], W - j0), dtype=torch.float64)
            for slot in range(pl["R"]):
                rows = list(range(slot, ln, pl["R"]))
                if defect == "slot_last_row_dropped" and len(rows) > 1:
                    rows = rows[:-1]
                if rows:
                    tot += T[[lo + r for r in rows], j0:j0 + len(tot)].sum(0)
            A[i, j0:j0 + len(tot)] = tot / ln
    return A


def emulate_probs(Pfull, Nq, defect=None):
    """Pfull [N, N]: row q as the kernel would form it (rows >= Nq: q = 0 and LSE = 0 give 1 everywhere).  Returns the guarded flat buffer of one
    (batch, head) at the end of the allocation.  defect: "rows_past_nq" (:90 without the row test), "last_key" (:90 with key < N - 1)."""
    N = Pfull.shape[1]
    buf, inner = guarded_nan(Nq * N)
    buf = buf.double()
    nqt = -(-Nq // 128)
    for q0 in range(0, nqt * 128, 32):
        if q0 >= Nq:
            continue
        for row in range(q0, q0 + 32):
            if row >= Nq and defect != "rows_past_nq":
                continue
            keys = N - 1 if defect == "last_key" else N
            at = GUARD + row * N
            if at + keys <= len(buf):
                buf[at:at + keys] = Pfull[min(row, N - 1), :keys]
    return buf


def emulate_rollout(Ps, gs, w, alpha, defect=None):
    """Ps [H, N, N] float64, gs [H, N] the rows' group sizes, w [N] -> out [N].  defect: "clamped_row" (the rows past N of the last 64-query tile, copies of
    row N - 1, carry w[N - 1]), "lse_head0" (every head's row constant from head 0's LSE: p scaled by g_h / g_0), "zero_weight" (a zero weight counts as 1)."""
    H, N = Ps.shape[0], Ps.shape[1]
    w = w.double()
    tot = torch.zeros(N, dtype=torch.float64)
    for h in range(H):
        P = Ps[h] * (gs[h] / gs[0])[:, None] if defect == "lse_head0" else Ps[h]
        wq = torch.where(w > 0, w, torch.ones_like(w)) if defect == "zero_weight" else w
        tot += wq @ P
        if defect == "clamped_row":
            tot += (-(-N // 64) * 64 - N) * w[N - 1] * P[N - 1]
    return alpha * w + (1 - alpha) / H * tot


# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [MASS_SWEEP, [(c, n) for _, _, c, n in MASS_TABLE], OLD_MASS_SHAPES], ids=["sweep", "table", "older-test"])
def test_the_walk_stores_every_segment_once(shapes):
    for C_, n_p in shapes:
        blocks, stores = mass_walk(C_, n_p)
        N = 1 + C_ * n_p
        assert stores == [(0, 0, 1)] + [(1 + c, 1 + c * n_p, 1 + (c + 1) * n_p) for c in range(C_)], (C_, n_p)
        assert len(blocks) == -(-N // 32) and sum(b.flushes for b in blocks) == 1 + C_


def test_the_tables_reach_every_regime():
    walks = {s: mass_walk(*s)[0] for s in MASS_SWEEP}
    # a segment boundary (end key of a segment) on every residue mod 32
    assert {(1 + c * n_p) % 32 for C_, n_p in MASS_SWEEP for c in range(C_ + 1)} == set(range(32))
    wf = [s for s, bl in walks.items() if any(b.kind == "whole+flush" for b in bl)]
    assert len(wf) == 33 and set(NAMED_WHOLE_FLUSH) <= set(wf)
    assert all(n_p >= 32 and n_p % 2 == 1 for _, n_p in wf)
    assert any(b.kind == "whole" for bl in walks.values() for b in bl)
    assert {b.flushes for bl in walks.values() for b in bl if b.kind == "cross"} == set(range(1, 10))  # (a crossing block ends a segment)
    assert any(b.kind == "cross" and b.goes_on and b.flushes for bl in walks.values() for b in bl)
    assert any(b.kind == "cross" and not b.goes_on and not b.past_n for bl in walks.values() for b in bl)  # a boundary on the block's end, from the loop
    assert {bl[-1].past_n for bl in walks.values()} >= set(range(0, 32))
    assert any(bl[-1].kind == "whole+flush" for bl in walks.values())  # the sweep ends on the fast path
    assert any(b.kind == "whole+flush" for bl in walks.values() for b in bl[:-1])  # ... and passes through it
    # the gap: the shapes of the older test
    assert not [s for s in OLD_MASS_SHAPES if any(b.kind == "whole+flush" for b in mass_walk(*s)[0])]
    # the table
    table = {(c, n): mass_walk(c, n)[0] for _, _, c, n in MASS_TABLE}
    assert {(c, n) for _, _, c, n in MASS_TABLE} >= {(8, 196), (15, 49), (7, 169), (64, 1), (12, 4), (255, 1), (256, 1), (300, 1), (257, 2), (1, 1)}
    assert (2, 6, 8, 196) in MASS_TABLE
    for s in ((15, 49), (7, 169)):
        assert any(b.kind == "whole+flush" for b in table[s])
    assert max(b.flushes for b in table[(64, 1)]) == 32 and max(b.flushes for b in table[(12, 4)]) == 8
    plans = {s: mean_plan(*s) for s in table}
    assert [(plans[s]["passes"], plans[s]["last_cols"], plans[s]["R"]) for s in ((255, 1), (256, 1), (300, 1), (257, 2))] == \
        [(1, 256, 1), (2, 1, 1), (2, 45, 1), (2, 2, 1)]
    assert all(mean_plan(c, n)["passes"] == 1 for c, n in OLD_MASS_SHAPES)  # the wide case was never run
    sweep_plans = [mean_plan(*s) for s in MASS_SWEEP]
    assert {p["R"] for p in sweep_plans} == {128, 85, 64, 42, 28}
    assert {1, 2, 3, 5} <= {p["slot_rows"] for p in sweep_plans} and plans[(8, 196)]["slot_rows"] == 7
    assert plans[(257, 2)]["slot_rows"] == 2  # R = 1: one slot adds both rows
    # probabilities
    pp = {N: probs_plan(N) for N in PROBS_SWEEP}
    assert set(PROBS_SWEEP) == set(range(1, 331)) and sum(PROBS_SWEEP_CHUNKS, []) == PROBS_SWEEP
    assert {p["nt"] for p in pp.values()} == set(range(1, 7)) and {p["nqt"] for p in pp.values()} == {1, 2, 3}
    assert {p["key_tail"] for p in pp.values()} == set(range(32)) and any(p["second_block_skipped"] for p in pp.values())
    assert {tuple(p["waves"]) for p in pp.values()} >= {("partial", "idle", "idle", "idle"), ("full", "full", "full", "full"), ("full", "full", "partial", "idle")}
    tp = {(N, Nq): probs_plan(N, Nq) for _, _, N, Nq in PROBS_TABLE}
    assert set(tp) == {(200, 2), (200, 31), (200, 32), (200, 33), (300, 127), (300, 128), (300, 129), (300, 160), (1569, 1), (1569, 130), (300, None)}
    for key in ((200, 2), (200, 31), (200, 33), (300, 127), (300, 129), (1569, 1), (1569, 130)):
        assert "partial" in tp[key]["waves"], key
    for key in ((200, 32), (300, 128), (300, 160)):
        assert "partial" not in tp[key]["waves"], key
    assert tp[(300, 129)]["nqt"] == 2 and tp[(1569, 130)]["nt"] == 25 and (3, 5, 300, None) in PROBS_TABLE
    # rollout
    rp = {N: rollout_plan(N) for N in ROLLOUT_SWEEP}
    assert set(ROLLOUT_SWEEP) == set(range(1, 401)) and sum(ROLLOUT_SWEEP_CHUNKS, []) == ROLLOUT_SWEEP
    assert {p["nkt"] for p in rp.values()} == {1, 2, 3, 4} and {p["nt"] for p in rp.values()} == set(range(1, 8))
    assert {p["clamped"] for p in rp.values()} == set(range(64)) and {p["idle_waves"] for p in rp.values()} == {0, 1, 2, 3}
    assert any(p["second_block_skipped"] for p in rp.values()) and {p["key_tail"] for p in rp.values()} == set(range(32))
    assert ROLLOUT_TABLE == [(3, 6, 257), (2, 12, 197), (1, 6, 1569)]
    # the sweeps are cut into tests of about 80 shapes
    for chunks in (MASS_SWEEP_CHUNKS, PROBS_SWEEP_CHUNKS, ROLLOUT_SWEEP_CHUNKS):
        assert all(40 <= len(c) <= 90 for c in chunks)
    assert sum(MASS_SWEEP_CHUNKS, []) == MASS_SWEEP and len(MASS_SWEEP) == 650 and max(1 + c * n for c, n in MASS_SWEEP) == 1041


MIXUP_MIN_N = 8


def _all_cases():
    out = [(1, 2, 1 + c * n, None) for c, n in MASS_SWEEP] + [(B, H, 1 + c * n, None) for B, H, c, n in MASS_TABLE + MASS_FWD]
    out += [(1, 2, N, None) for N in PROBS_SWEEP] + PROBS_TABLE + PROBS_FWD
    out += [(1, 3, N, None) for N in ROLLOUT_SWEEP] + [(B, H, N, None) for B, H, N in ROLLOUT_TABLE + ROLLOUT_FWD]
    return sorted(set(out), key=lambda c: (c[2], c[0], c[1], c[3] or 0))


def test_every_batch_and_head_has_its_own_structure():
    """Any two (batch, head) pairs of a case differ in the target group (its set of keys) of at least half of their rows."""
    checked = 0
    for B, H, N, Nq in _all_cases():
        ops = probe_ops(B, H, N, Nq)
        assert all(set(st.gsize.tolist()) <= {1, 2, 4} for st in ops.sts)
        if N < MIXUP_MIN_N:
            continue
        rk = torch.stack([row_keys(st) for st in ops.sts])  # [P, Nq, 4]
        differ = (rk[:, None] != rk[None, :]).any(-1).double().mean(-1)  # [P, P]: share of rows
        differ.fill_diagonal_(1.0)
        assert float(differ.min()) >= 0.5, (B, H, N, Nq, float(differ.min()))
        checked += 1
    assert checked > 800
    _ops.clear()  # (the sweeps' structures: some hundred MB)


def test_rollout_weights_meet_the_conditions():
    for B, H, N in [(1, 3, N) for N in ROLLOUT_SWEEP] + ROLLOUT_TABLE + ROLLOUT_FWD:
        ws = rollout_weights(B, N)
        for w in ws.values():
            assert w.shape == (B, N) and w.dtype == torch.float32 and set(w.flatten().tolist()) <= set(W_VALUES)
            assert N == 1 or bool((w[:, N - 1] > 0).all())
        assert bool(((ws["sparse"] == 0).double().mean(-1) >= 0.25).all()) and bool((ws["dense"] > 0).all())
        assert bool((ws["sparse"] > 0).any()) or N == 1
        if N > 128:
            assert bool((ws["sparse"][:, 64:128] == 0).all())
        if N >= 32:
            assert len(set(ws["sparse"].flatten().tolist())) >= 4


def test_the_float32_arithmetic_stays_inside_the_bound():
    """The plain form as the kernels compute it, in float32 (the fma evaluated exactly in float64 and rounded once): p = exp2(fma(s, c, rowc)) with s = 6144
    for a key of the target group, for the three group sizes a row can have, and the rollout's row constant for the four weights, contracted or not.
    v_exp_f32's own ulp is allowed for on top."""
    f = np.float32
    log2e, s = f(LOG2E), 6144.0  # BETA * 12
    c = f(f(SCALE) * log2e)
    assert float(c) == SCALE * float(log2e)  # scale = 1/8: exact
    worst = 0.0
    for g in (1, 2, 4):
        lse = f(SCALE * BETA * 12 + math.log(g))
        rowc = f(-lse * log2e)
        p = 2.0 ** float(f(s * float(c) + float(rowc)))
        worst = max(worst, abs(p * g - 1))
        for w in W_VALUES[1:]:
            two_roundings = f(f(math.log2(w)) - f(lse * log2e))
            contracted = f(math.log2(w) - float(lse) * float(log2e))
            for cq in (two_roundings, contracted):
                pw = 2.0 ** float(f(s * float(c) + float(cq)))
                worst = max(worst, abs(pw * g / w - 1))
        # the other keys: at least 185 log2 units below, exactly zero
        assert 2.0 ** float(f((s - 2 * BETA) * float(c) + float(rowc))) < 2.0 ** -149
    assert worst <= 3.2e-4 * math.log(2) * 1.05 + 2.0 ** -22, worst  # the docstring's 3.1e-4 log2 units
    assert worst + 2.0 ** -22 <= REL
    # the pre-scaled operand: 92.5 exactly, 1110 in all
    assert float(torch.tensor(BETA * QC).to(torch.bfloat16)) == 92.5 and abs(QAMP_PS * QC - 92.5) < 1e-12


SOFTMAX_CASES = [(2, 3, 1, None), (1, 2, 64, None), (2, 2, 99, None), (1, 2, 200, 33), (1, 3, 197, None)]


@pytest.mark.parametrize("B,H,N,Nq", SOFTMAX_CASES)
def test_the_closed_forms_are_the_float64_softmax(B, H, N, Nq):
    """The materialised float64 softmax of the device operands, both forms, against p_ref; T, A and out computed densely from it against the closed forms;
    and the emulations without a defect against the same."""
    ops = probe_ops(B, H, N, Nq)
    ref = p_ref(ops)
    for prescaled in (False, True):
        t = device_qkv(ops, prescaled).double().view(B, N, 3, H, 64)
        q, k = t[:, :ops.Nq, 0].transpose(1, 2), t[:, :, 1].transpose(1, 2)
        s = q @ k.transpose(-1, -2) * (math.log(2.0) if prescaled else SCALE)
        assert float((torch.softmax(s, -1) - ref).abs().max()) <= DUST
        lse = closed_lse(ops, prescaled).double()[:, :, :ops.Nq]
        assert float((torch.logsumexp(s, -1) - lse).abs().max()) <= 2.0 ** -15 * 1.001  # half an fp32 ulp of 768
        assert bool((closed_lse(ops, prescaled)[:, :, ops.Nq:] == 0).all())
    if Nq is not None:
        full = torch.ones(N, N, dtype=torch.float64)
        full[:Nq] = ref[0, 0]
        buf = emulate_probs(full, Nq)
        assert not buffer_findings("P", buf, Nq * N) and not rule(buf[GUARD:GUARD + Nq * N].view(Nq, N), ref[0, 0])[0].any()
        return
    for C_ in sorted({c for c in (1, 2, 7, 9, 14, 49, 98) if (N - 1) % c == 0 and N > 1}):
        n_p = (N - 1) // C_
        Tr = t_ref(ops, C_, n_p)
        onehot = torch.nn.functional.one_hot(segment_of(N, n_p), 1 + C_).double()
        assert float((ref @ onehot - Tr).abs().max()) <= 1e-12 and float((Tr.sum(-1) - 1).abs().max()) <= 1e-12
        T = emulate_mass(ref[0, 0], C_, n_p)
        assert not rule(T, Tr[0, 0], 4)[0].any()
        assert not rule(emulate_mean(T, C_, n_p), seg_mean64(Tr[0, 0], C_, n_p), n_p)[0].any()
    for name, w in rollout_weights(B, N).items():
        for alpha in ALPHAS:
            out, cnt = out_ref(ops, w, alpha)
            dense = alpha * w.double() + (1 - alpha) * torch.einsum("bq,bqk->bk", w.double(), ref.mean(1))
            assert float((out - dense).abs().max()) <= 1e-12
            assert bool((cnt == torch.einsum("bq,bhqk->bk", (w > 0).double(), (ref > 0).double())).all())
            gs = torch.stack([st.gsize[st.tgt].double() for st in ops.sts[:H]])
            assert not rule(emulate_rollout(ref[0], gs, w[0], alpha), out[0], cnt[0])[0].any()


def _flagged_mass(ops, C_, n_p, defect):
    T = emulate_mass(p_ref(ops)[0, 0], C_, n_p, defect)
    return bool(rule(T, t_ref(ops, C_, n_p)[0, 0], 4)[0].any())


def test_every_injected_defect_is_flagged():
    """Each defect of the list, injected into the float64 emulation of one (batch, head) on the group operands, is flagged by the rules the GPU tests apply."""
    # channel mass
    for C_, n_p in ((1, 63), (1, 95), (1, 127)):  # the fast path is the sweep's last block: the segment stays unwritten
        assert _flagged_mass(probe_ops(1, 2, 1 + C_ * n_p), C_, n_p, "whole_flush_dropped"), (C_, n_p)
    for C_, n_p in NAMED_WHOLE_FLUSH + [(15, 49), (7, 169)]:
        assert _flagged_mass(probe_ops(1, 2, 1 + C_ * n_p), C_, n_p, "flush_before_adds"), (C_, n_p)
    # (mid-sweep the crossing loop of the next block repairs a dropped flush: the module docstring's finding)
    assert not _flagged_mass(probe_ops(1, 2, 127), 2, 63, "whole_flush_dropped")
    for C_, n_p in ((2, 63), (3, 53), (5, 16), (8, 3), (64, 1), (15, 49)):
        ops = probe_ops(1, 2, 1 + C_ * n_p)
        assert _flagged_mass(ops, C_, n_p, "le"), (C_, n_p)
        assert _flagged_mass(ops, C_, n_p, "no_upper_half"), (C_, n_p)
        if (1 + C_ * n_p) % 32:
            assert _flagged_mass(ops, C_, n_p, "past_n"), (C_, n_p)
        assert not _flagged_mass(ops, C_, n_p, None)
    # mean kernel
    for C_, n_p, defect in ((8, 196, "slot_last_row_dropped"), (5, 130, "slot_last_row_dropped"), (257, 2, "slot_last_row_dropped"),
                            (256, 1, "second_pass_skipped"), (300, 1, "second_pass_skipped"), (257, 2, "second_pass_skipped")):
        ops = probe_ops(1, 2, 1 + C_ * n_p)
        Tr = t_ref(ops, C_, n_p)[0, 0]
        A = emulate_mean(Tr, C_, n_p, defect)
        assert rule(A, seg_mean64(Tr, C_, n_p), n_p)[0].any(), (C_, n_p, defect)
        assert mean_rule(A[None], Tr[None], C_, n_p)[0].any(), (C_, n_p, defect)  # and by A against the mean of T
        ok = emulate_mean(Tr, C_, n_p)
        assert not rule(ok, seg_mean64(Tr, C_, n_p), n_p)[0].any() and not mean_rule(ok[None], Tr[None], C_, n_p)[0].any()
    # probabilities
    for N, Nq in ((200, 2), (200, 33), (300, 129)):
        ops = probe_ops(1, 2, N, Nq)
        ref = p_ref(ops)[0, 0]
        full = torch.ones(N, N, dtype=torch.float64)
        full[:Nq] = ref
        leak = emulate_probs(full, Nq, "rows_past_nq")
        assert buffer_findings("P", leak, Nq * N), (N, Nq)  # lands in the guard behind the last (batch, head) ...
        assert bool((leak[GUARD + Nq * N:GUARD + Nq * N + N] == 1).all())  # ... and anywhere else as a row of ones over the next head's rows
        assert rule(torch.ones(N), p_ref(ops)[0, 1, 0])[0].any()
        short = emulate_probs(full, Nq, "last_key")
        assert buffer_findings("P", short, Nq * N) and rule(short[GUARD:GUARD + Nq * N].view(Nq, N), ref)[0].any()
    # rollout
    for H, N in ((3, 65), (3, 197), (6, 257)):
        ops = probe_ops(1, H, N)
        P = p_ref(ops)[0]
        gs = torch.stack([st.gsize[st.tgt].double() for st in ops.sts])
        for name, w in rollout_weights(1, N).items():
            for alpha in ALPHAS:
                out, cnt = out_ref(ops, w, alpha)
                for defect in ("clamped_row", "lse_head0") + (("zero_weight",) if name == "sparse" else ()):
                    assert rule(emulate_rollout(P, gs, w[0], alpha, defect), out[0], cnt[0])[0].any(), (H, N, name, alpha, defect)
                assert not rule(emulate_rollout(P, gs, w[0], alpha), out[0], cnt[0])[0].any()
