"""The GEMM kernels of csrc/gemm_nt.hip and csrc/gemm_tn.hip bit for bit: exact operands, padded layouts, guard rows.

Two gaps of the older GEMM tests are closed here.

* No tolerance.  Operands are integers in [-8, 8] stored as bf16 (scaled by a power of two where noted), biases and residuals are
  half-integers.  Every product is then exact, and as long as the sum of |a w| over an output element (bias, residual and initial value
  included) stays below 2^24 quanta, so is every partial sum in fp32, in any order.  Each test asserts that condition on its own inputs
  before the launch (assert_exact).  The reference is the same product in float64, cast ONCE to the output type, and the assertion is
  equality of the bits.  With this distribution 9 - 22 % of the bf16 outputs are exact ties (an odd integer in [256, 512), and so on
  upward), so round-to-nearest-even is pinned on thousands of elements per case (tie_share, asserted >= 2 %); a bias or residual that
  took a detour through bf16, an accumulator rounded before the GELU-backward multiply, or a row of a ragged stage counted twice
  changes bits.  The one epilogue that cannot be compared bit for bit is BIAS_GELU (transcendental): it is held to half a bf16 ulp plus
  1e-6 max(1, |z|) from the float64 erf-GELU of the exact z; the slack follows from the code's own approximation (Abramowitz-Stegun
  7.1.26: 1.5e-7 on erf, hence 7.5e-8 |z| on GELU, a handful of fp32 roundings, the 1-ulp rcp / exp2; test_gemm_exact_cpu.py repeats a
  float32 emulation of gelu_parts2 that stays within 1.42e-7 max(1, |z|) for GELU and 1.87e-7 for its derivative).  The test prints the
  largest excess over the half ulp it sees, in units of max(1, |z|) ("[gelu slack]" lines).  Measured on an MI355X over all
  cases: 4.61e-8 for GELU and 7.2e-9 for its derivative, a twentieth of the bound.

* Leading dimensions and what lies behind a tensor.  Every case runs dense and in two padded layouts (PADS): each bf16 operand inside a
  larger buffer with a leading dimension of width + 8 (the smallest legal pad: rows only 16-byte aligned) or width + 72, pad columns
  NaN, 64 NaN guard rows behind row M of A / Y / X / aux and behind row N of W; each output in a buffer with its own distinct pad,
  pre-filled with a sentinel that must still be in every pad element and guard row afterwards.  A read that uses K where it means lda,
  a clamp that reaches a guard row, a 16-byte store past column N of a partial tile: each changes bits or a sentinel.  The entries
  must refuse (error code, nothing launched) a leading dimension below the width or off its alignment.

The case tables hold the smallest shapes that reach each regime of each kernel (multi-round walks through grid_cap); the regimes are
asserted from launch plans restated here in pure Python with file:line references — without a GPU by test_gemm_exact_cpu.py, which
also checks the exactness and tie-share premises of every case, and against the library's own answers in this module.
Needs an MI355X: run with -m gpu."""
import ctypes as C
import functools
import math
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -12352.0   # "never written": exact in bf16 and fp32, outside every result's grid
GUARD = 64        # guard rows behind every matrix
CUS = 256         # compute units of an MI355X: the launch plans below are restated for it
NAN = float("nan")
EPI_BIAS, EPI_GELU, EPI_RESID, EPI_PLAIN, EPI_GELU_BWD, EPI_PATCH = range(6)           # include/dcv.h DCV_EPI_*
TILE_AUTO, TILE_NARROW, TILE_WIDE, TILE_PAIR, TILE_ALT, TILE_WS, TILE_AUTO_WS = range(7)  # include/dcv.h DCV_TILE_*
ERR_SHAPE, ERR_ALIGN = -1, -2
WS_M_MIN = 8192   # csrc/gemm_nt.hip: DCV_WS_M_MIN
FACTORS = (1.25, 0.0, 2.0, 0.5, 1.0)  # per-sample branch factors (DropPath's keep_b / keep_prob)

# pads (in elements) per layout: bf16 operands (A, W, Y, X, the bf16 aux) share `op`; every output has its own
PADS = {
    "dense": dict(op=0, out=0, out2=0, f32o=0, f32r=0, y=0, ln_o=0, ln_r=0, ln_u=0, dw=0),
    "pad8": dict(op=8, out=16, out2=24, f32o=16, f32r=4, y=12, ln_o=4, ln_r=12, ln_u=16, dw=4),
    "pad72": dict(op=72, out=40, out2=56, f32o=24, f32r=20, y=4, ln_o=12, ln_r=4, ln_u=88, dw=12),
}
LAYOUTS = tuple(PADS)


def _cdiv(a, b):
    return -(-a // b)


# =====================================================================================================================================
# Case tables
# =====================================================================================================================================
NtCase = namedtuple("NtCase", "tile M N K cap")
# 256 x 128 tiles, 3-stage ring: smallest; partial M tile; partial N tile, one stage, three rounds with a short last one; 24 stages, an
# 8-column last tile, five rounds
NT_NARROW = [NtCase(TILE_NARROW, *c) for c in [(1, 8, 64, 0), (300, 384, 384, 0), (777, 200, 64, 3), (1100, 392, 1536, 4)]]
# 128 x 128 tiles, two workgroups per CU (the grid is 2 cap)
NT_PAIR = [NtCase(TILE_PAIR, *c) for c in [(1, 8, 64, 0), (300, 384, 384, 0), (777, 200, 64, 2), (1100, 392, 1536, 3)]]
# 256 x 384 tiles on the balanced plan: one round; three mixed plans (192-row tiles in the last rounds); four rounds, unmixed
NT_WIDE = [NtCase(TILE_WIDE, *c) for c in [(300, 384, 128, 0), (1500, 384, 384, 4), (1100, 1152, 384, 6), (1153, 384, 64, 4), (2900, 384, 1536, 3)]]
NT_WIDE_MIXED = {(1500, 384, 4): True, (1100, 1152, 6): True, (1153, 384, 4): True, (300, 384, 0): False, (2900, 384, 3): False}
# weight-stationary (K = 384): one row; one group of three slices, a 31-row last panel; one group of four, more panels than the ring is
# deep; three groups; and the automatic choice from DCV_WS_M_MIN rows on
NT_WS = [NtCase(TILE_WS, *c) for c in [(1, 384, 384, 0), (95, 1152, 384, 4), (1000, 1536, 384, 7), (4100, 384, 384, 3)]] + \
        [NtCase(TILE_AUTO_WS, 8200, 384, 384, 0)]
NT_CASES = NT_NARROW + NT_PAIR + NT_WIDE + NT_WS
NT_RESID_CASES = NT_NARROW + NT_PAIR + NT_WIDE  # the fp32-output epilogue is not on the weight-stationary kernel
PATCH_SPLIT = {1: (1, 1, 1), 300: (2, 3, 50), 777: (3, 7, 37), 1100: (4, 5, 55)}  # M -> (B, C, n): M = B C n token rows
LnCase = namedtuple("LnCase", "M K cap")
LN_CASES = [LnCase(300, 384, 0), LnCase(1500, 384, 4), LnCase(2100, 1536, 3), LnCase(777, 64, 3)]

TnCase = namedtuple("TnCase", "tile M P Q")
# 128 x 128 tiles, 64 rows per stage: smallest; fewer rows than one stage; partial tiles on both sides, one row in the second stage; -;
# 65 splits of one stage, the last with 3 rows; fewer splits launched than planned; six stages per split (more than the two buffers)
TN_NARROW = [TnCase(TILE_NARROW, *c) for c in [(1, 8, 8), (31, 128, 128), (65, 200, 72), (700, 384, 256), (4099, 192, 64), (5000, 384, 384),
                                               (3000, 1024, 1024)]]
# 384 x 128 tiles, 32 rows per stage, ring of 4: around one stage; one stage per split (fewer stages than the ring is deep); one stage
# per split and 12 column tiles (the kt % tiles_q == tq sharing of the bias sum leaves it to tq = 0); 26 of 28 planned splits, ragged end
TN_WIDE = [TnCase(TILE_WIDE, *c) for c in [(31, 384, 128), (32, 384, 128), (33, 384, 128), (1000, 384, 128), (333, 384, 1536), (4099, 1152, 384)]]
TN_CASES = TN_NARROW + TN_WIDE
GROUP_ITEMS = [(384, 1536, True), (1536, 384, True), (384, 384, False), (1152, 384, True)]  # (P, Q, bias): fc2, fc1, proj (no bias here), qkv
GROUP_MS = [31, 5000, 64 * 197 + 5]


def _with_layouts(cases):
    return [pytest.param(c, lay, id="-".join(str(v) for v in c) + "-" + lay) for c in cases for lay in LAYOUTS]


# =====================================================================================================================================
# Launch plans (pure Python; no GPU)
# =====================================================================================================================================
NtWalk = namedtuple("NtWalk", "tiles_m tiles_n grid rounds last_round stages")


def nt_walk(tile, M, N, K, cap, cus=CUS):
    """The static tile walks of the NARROW / PAIR kernels: csrc/gemm_nt.hip gemm_nt_kernel (tiles of 256 x 128, `L = k * G + pos`) with the
    grid of dcv_gemm_nt_ex (`grid = min(tiles, cap)`), gemm_nt_pair_kernel (128 x 128, `gp = min(tiles, 2 * cap)`); K in 64-wide stages."""
    bm, per_cu = (256, 1) if tile == TILE_NARROW else (128, 2)
    tm, tn = _cdiv(M, bm), _cdiv(N, 128)
    grid = min(tm * tn, per_cu * (cap or cus))
    rounds = _cdiv(tm * tn, grid)
    return NtWalk(tm, tn, grid, rounds, tm * tn - (rounds - 1) * grid, K // 64)


WsWalk = namedtuple("WsWalk", "slices panels groups panels_max last_rows")


def ws_walk(M, N, cap, cus=CUS):
    """gemm_nt_ws_kernel: `groups = min(cap / slices, panels)` workgroup groups of N / 384 slices (dcv_gemm_nt_ex), group g walks the
    32-row panels g, g + groups, ... through a ring of 6 (3 with the GELU-backward's aux) slots."""
    slices, panels = N // 384, _cdiv(M, 32)
    groups = min((cap or cus) // slices, panels)
    return WsWalk(slices, panels, groups, _cdiv(panels, groups), M - 32 * (panels - 1))


TnPlan = namedtuple("TnPlan", "tiles_q tiles planned mps splits stage nk_max last_rows ws_floats")


def tn_plan(tile, M, P, Q, cus=CUS):
    """csrc/gemm_tn.hip tn_plan and the workspace layout of tn_launch / dcv_gemm_tn_det_ws_floats: `planned` splits of the token rows (one
    resident round: 2 workgroups per CU for the 128 x 128 kernel, 1 for the 384 x 128 one; at most one per stage), `mps` rows per split
    rounded up to whole stages, `splits` = the leading ones that have rows."""
    if tile == TILE_WIDE:
        tq, tiles, bk = Q // 128, (P // 384) * (Q // 128), 32
        planned = cus // tiles
    else:
        tq, tiles, bk = _cdiv(Q, 128), _cdiv(P, 128) * _cdiv(Q, 128), 64
        planned = 2 * cus // tiles
    planned = max(1, min(planned, _cdiv(M, bk)))
    mps = _cdiv(_cdiv(M, planned), bk) * bk
    splits = _cdiv(M, mps)
    last = M - (splits - 1) * mps
    ws = splits * P * Q + splits * tq * P if tile == TILE_WIDE else (P * Q + P) * splits
    return TnPlan(tq, tiles, planned, mps, splits, bk, _cdiv(min(mps, M), bk), last, ws)


def tn_group_plan(items, M, cus=CUS):
    """csrc/gemm_tn.hip tn_group_plan: every product split the same way, `sp = min(cus / all tiles, stages)`; workspace per item
    [splits][P Q] then [splits * Q / 128][P].  Returns (tiles, mps, splits, ws floats)."""
    tiles = sum((P // 384) * (Q // 128) for P, Q, _ in items)
    sp = min(cus // tiles, _cdiv(M, 32))
    mps = _cdiv(_cdiv(M, sp), 32) * 32
    splits = _cdiv(M, mps)
    return tiles, mps, splits, sum(splits * P * Q + splits * (Q // 128) * P for P, Q, _ in items)


# =====================================================================================================================================
# Exact inputs (seeded CPU generator) and the premises every test asserts
# =====================================================================================================================================
def ints(rows, cols, seed, lim=8):
    """integers drawn uniformly from [-lim, lim], fp32 on the CPU (exact in bf16 up to 256)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-lim, lim + 1, (rows, cols), generator=g).float()


def halves(rows, cols, seed, lim=8):
    """half-integers drawn uniformly from [-lim, lim]"""
    return ints(rows, cols, seed, 2 * lim) * 0.5


def assert_exact(what, terms, amax, wmax, quantum, extra=0.0, factor=1.0):
    """The exactness condition: an output element is a sum of `terms` products, each bounded by amax wmax, times `factor`, plus `extra`
    (bias, residual, initial value); every partial sum is a multiple of `quantum`.  Below 2^24 quanta each of them is an fp32 number,
    whatever the order of the additions."""
    bound = (terms * amax * wmax * factor + extra) / quantum
    assert bound < 2 ** 24, f"{what}: up to {bound:.3g} quanta: the inputs are not exact in fp32"


def tie_share(x):
    """share of the values (float64 or fp32, exactly representable in fp32) that lie exactly half way between two bf16 numbers"""
    x32 = x.float()
    assert torch.equal(x32.double(), x.double())
    return ((x32.contiguous().view(torch.int32) & 0xFFFF) == 0x8000).float().mean().item()


def to_out(x64, dtype):
    """float64 -> the output type in ONE rounding: exact to fp32 (asserted), then fp32 -> bf16 to nearest even"""
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), "the reference is not an fp32 number: the inputs are not exact"
    return x32.to(dtype)


def ulp_bf16(x):
    """spacing of the bf16 numbers around x (float64): 2^(floor(log2 |x|) - 7), the subnormal spacing 2^-133 below 2^-126"""
    _, e = torch.frexp(x.abs())  # |x| = m 2^e, m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(e, -1000), e)
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp(min=-126) - 7)


def gelu64(z):
    """erf-GELU and its derivative in float64"""
    cdf = 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
    return z * cdf, cdf + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


@functools.lru_cache(maxsize=2)
def nt_inputs(M, N, K):
    """CPU fp32 tensors of one NT problem: A [M, K] and W [N, K] integers, bias [N] and resid [M, N] half-integers, gp [M, N] arbitrary bf16
    values (the saved GELU'), acc = A W^T (exact in fp32: integers below 2^24)"""
    seed = 1000 * M + 10 * N + K
    A, W = ints(M, K, seed + 1), ints(N, K, seed + 2)
    g = torch.Generator(device="cpu").manual_seed(seed + 5)
    gp = torch.randn(M, N, generator=g).to(torch.bfloat16).float()
    return dict(A=A, W=W, bias=halves(1, N, seed + 3)[0], resid=halves(M, N, seed + 4, 32), gp=gp, acc=A @ W.t())


def samples_of(M):
    """(samples, rows per sample) for the per-sample branch factor: the most samples of FACTORS that divide M"""
    s = next(s for s in (5, 4, 3, 2, 1) if M % s == 0)
    return s, M // s


@functools.lru_cache(maxsize=1)
def tn_inputs(M, P, Q):
    seed = 7000 * M + 10 * P + Q
    return dict(Y=ints(M, P, seed + 1), X=ints(M, Q, seed + 2), dW0=ints(P, Q, seed + 3, 100), db0=ints(1, P, seed + 4, 100)[0])


# =====================================================================================================================================
# GPU side
# =====================================================================================================================================
@pytest.fixture(scope="module")
def lib(gpu_device):
    from diverse_channel_vit_amd import hip as h
    return h.load()


class Mat:
    """rows x width inside a (rows + guard) x (width + pad) buffer filled with `fill` (NaN behind operands, SENT around outputs)"""

    def __init__(self, rows, width, dtype, pad, fill, data=None, guard=GUARD):
        self.rows, self.width, self.ld, self.fill = rows, width, width + pad, fill
        self.buf = torch.full((rows + guard, self.ld), fill, dtype=dtype, device="cuda")
        if data is not None:
            self.buf[:rows, :width] = data.to(device="cuda").reshape(rows, width)
        self.ptr = C.c_void_p(self.buf.data_ptr())

    @property
    def data(self):
        return self.buf[:self.rows, :self.width]

    def untouched(self):
        """every pad element and guard row still holds the sentinel"""
        return bool((self.buf[:self.rows, self.width:] == self.fill).all()) and bool((self.buf[self.rows:] == self.fill).all())


def vec(n, fill, data=None):
    """n floats with 64 more behind them"""
    return Mat(1, n, torch.float32, GUARD, fill, data, guard=0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pl(m):
    return (None, 0) if m is None else (m.ptr, m.ld)


def nt_ex(lib, A, W, M, N, K, epi, out, tile, cap, bias=None, out2=None, aux=None, aux2=None, T=0, n=0, ld=None):
    """dcv_gemm_nt_ex through ctypes (hip.gemm_nt cannot pass lda / ldw); ld: overrides of single leading dimensions (the refusal tests)"""
    l = dict(lda=A.ld, ldw=W.ld, ldo=out.ld, ldo2=_pl(out2)[1], ldaux=_pl(aux)[1])
    l.update(ld or {})
    return lib.dcv_gemm_nt_ex(A.ptr, l["lda"], W.ptr, l["ldw"], M, N, K, epi, bias.ptr if bias else None, out.ptr, l["ldo"], _pl(out2)[0], l["ldo2"],
                              _pl(aux)[0], l["ldaux"], aux2.ptr if aux2 else None, T, n, cap, tile, _stream())


def same_bits(got, want, what):
    got, want = got.contiguous(), want.contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype
    it = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    bad = got.view(it) != want.view(it)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference; first at {i}: "
                             f"got {got[i].item()!r}, want {want[i].item()!r}")


def _assert_runs(lib, c):
    """the kernel the table row is listed under is the one dcv_gemm_nt_ex launches, in the regime the row names"""
    want = TILE_WS if c.tile == TILE_AUTO_WS else c.tile
    for epi in (EPI_BIAS, EPI_GELU, EPI_PLAIN, EPI_GELU_BWD):
        assert lib.dcv_gemm_nt_pick(c.M, c.N, c.K, epi, c.tile) == want, f"{c}: epilogue {epi} would not run on tile variant {want}"
    if c.tile == TILE_AUTO_WS:
        assert c.M >= WS_M_MIN
    if c.tile == TILE_WIDE:
        tiles = _cdiv(c.M, 256) * (c.N // 384)
        a, b = C.c_int(-1), C.c_int(-1)
        assert lib.dcv_gemm_nt384_plan(c.M, c.N, min(tiles, c.cap) if c.cap else tiles, C.byref(a), C.byref(b)) == 0
        assert (b.value > 0) == NT_WIDE_MIXED[(c.M, c.N, c.cap)], f"{c}: plan ({a.value}, {b.value})"


class NtDev:
    """the device copies of one NT problem and its float64 accumulator"""

    def __init__(self, M, N, K):
        h = nt_inputs(M, N, K)
        self.h = h
        self.acc = h["A"].cuda().double() @ h["W"].cuda().double().t()
        assert torch.equal(self.acc, h["acc"].cuda().double())  # float64 on the GPU and fp32 on the CPU agree: both are exact
        self.bias, self.resid, self.gp = h["bias"].cuda().double(), h["resid"].cuda().double(), h["gp"].cuda().double()


@functools.lru_cache(maxsize=2)
def nt_dev(M, N, K):
    return NtDev(M, N, K)


def _operands(c, d, lay, w_scale=1.0):
    p = PADS[lay]["op"]
    return (Mat(c.M, c.K, torch.bfloat16, p, NAN, d.h["A"]), Mat(c.N, c.K, torch.bfloat16, p, NAN, d.h["W"] * w_scale), vec(c.N, NAN, d.h["bias"]))


@pytest.mark.parametrize("c,lay", _with_layouts(NT_CASES))
def test_nt_plain_and_bias_round_to_nearest_even(lib, c, lay):
    """PLAIN_BF16 and BIAS_BF16 (half-integer fp32 bias): the bf16 outputs bit-match the float64 product rounded once"""
    _assert_runs(lib, c)
    d = nt_dev(c.M, c.N, c.K)
    assert_exact("acc + bias", c.K, 8, 8, 0.5, extra=8)
    A, W, bias = _operands(c, d, lay)
    for epi, ref in ((EPI_PLAIN, d.acc), (EPI_BIAS, d.acc + d.bias)):
        if c.M * c.N >= 10 ** 4:
            share = tie_share(ref)
            assert share >= 0.02, f"epilogue {epi}: only {share:.2%} of the outputs are exact bf16 ties: the rounding mode is not pinned"
        out = Mat(c.M, c.N, torch.bfloat16, PADS[lay]["out"], SENT)
        assert nt_ex(lib, A, W, c.M, c.N, c.K, epi, out, c.tile, c.cap, bias=bias) == 0
        same_bits(out.data, to_out(ref, torch.bfloat16), f"epilogue {epi}")
        assert out.untouched(), f"epilogue {epi}: a pad column or guard row of the output was written"


@pytest.mark.parametrize("c,lay", _with_layouts(NT_RESID_CASES))
def test_nt_bias_resid_f32_exact(lib, c, lay):
    """BIAS_RESID_F32 in place and out of place, with and without the per-sample branch factor: torch.equal to resid + s (acc + bias)"""
    assert lib.dcv_gemm_nt_pick(c.M, c.N, c.K, EPI_RESID, c.tile) == c.tile
    d = nt_dev(c.M, c.N, c.K)
    # s (acc + bias) is a multiple of 1/8 (1.25 times a half-integer) bounded by 2 (64 K + 8); the residual adds at most 32
    assert_exact("resid + s (acc + bias)", c.K, 8, 8, 0.125, extra=2 * 8 + 32, factor=2.0)
    A, W, bias = _operands(c, d, lay)
    samples, T = samples_of(c.M)
    f = torch.tensor(FACTORS[:samples])
    fac = vec(samples, NAN, f)
    for scaled in (False, True):
        s_rows = f.cuda().double().repeat_interleave(T)[:, None] if scaled else 1.0
        want = to_out(d.resid + s_rows * (d.acc + d.bias), torch.float32)
        for inplace in (False, True):
            out = Mat(c.M, c.N, torch.float32, PADS[lay]["f32o"], SENT, d.h["resid"] if inplace else None)
            aux = None if inplace else Mat(c.M, c.N, torch.float32, PADS[lay]["f32r"], NAN, d.h["resid"])
            rc = nt_ex(lib, A, W, c.M, c.N, c.K, EPI_RESID, out, c.tile, c.cap, bias=bias, aux=aux, aux2=fac if scaled else None, T=T if scaled else 0)
            assert rc == 0
            what = f"scaled {scaled}, in place {inplace}"
            same_bits(out.data, want, what)
            assert out.untouched(), f"{what}: a pad column or guard row of the output was written"


@pytest.mark.parametrize("c,lay", _with_layouts(NT_CASES))
def test_nt_gelu_bwd_exact(lib, c, lay):
    """GELU_BWD_BF16: acc (at most 16 significant bits, asserted) times an arbitrary bf16 is exact in fp32: the output is that product
    rounded once — an accumulator rounded to bf16 before the multiply changes bits"""
    d = nt_dev(c.M, c.N, c.K)
    assert_exact("acc", c.K, 8, 8, 1.0)
    assert d.acc.abs().max().item() < 2 ** 16
    A, W, _ = _operands(c, d, lay)
    aux = Mat(c.M, c.N, torch.bfloat16, PADS[lay]["op"], NAN, d.h["gp"])
    out = Mat(c.M, c.N, torch.bfloat16, PADS[lay]["out"], SENT)
    assert nt_ex(lib, A, W, c.M, c.N, c.K, EPI_GELU_BWD, out, c.tile, c.cap, aux=aux) == 0
    same_bits(out.data, to_out(d.acc * d.gp, torch.bfloat16), "acc * aux")
    assert out.untouched()


GELU_SLACK = 1e-6  # times max(1, |z|), on top of half a bf16 ulp: see the module docstring


@pytest.mark.parametrize("c,lay", _with_layouts(NT_CASES))
def test_nt_bias_gelu_within_half_ulp(lib, c, lay, capsys):
    """BIAS_GELU_BF16 with W scaled by 2^-8: z = acc + bias is exact (steps of 2^-8, about +-15); out = GELU'(z) and out2 = GELU(z) within
    ulp_bf16(ref) / 2 + 1e-6 max(1, |z|) of the float64 erf-GELU of that z"""
    d = nt_dev(c.M, c.N, c.K)
    assert_exact("z = acc + bias", c.K, 8, 8 / 256, 1 / 256, extra=8)
    A, W, bias = _operands(c, d, lay, w_scale=2.0 ** -8)
    z = d.acc / 256 + d.bias
    g, gp = gelu64(z)
    out = Mat(c.M, c.N, torch.bfloat16, PADS[lay]["out"], SENT)
    out2 = Mat(c.M, c.N, torch.bfloat16, PADS[lay]["out2"], SENT)
    assert nt_ex(lib, A, W, c.M, c.N, c.K, EPI_GELU, out, c.tile, c.cap, bias=bias, out2=out2) == 0
    zs = z.abs().clamp(min=1.0)
    for name, got, ref in (("GELU'", out, gp), ("GELU", out2, g)):
        excess = ((got.data.double() - ref).abs() - 0.5 * ulp_bf16(ref)) / zs
        worst = excess.max().item()
        with capsys.disabled():
            print(f"\n[gelu slack] {name} {tuple(c)} {lay}: largest (|got - ref| - ulp / 2) / max(1, |z|) = {worst:.3e}, |z| up to {z.abs().max().item():.2f}")
        assert worst <= GELU_SLACK, f"{name}: {int((excess > GELU_SLACK).sum())} elements past half a bf16 ulp + {GELU_SLACK} max(1, |z|), worst {worst:.3e}"
        assert got.untouched(), f"{name}: a pad column or guard row of the output was written"


@pytest.mark.parametrize("c,lay", _with_layouts(NT_NARROW))
def test_nt_patch_exact(lib, c, lay):
    """PATCH (256 x 128 kernel only): Y = acc + bias and the token rows Y + E[c] + pos[1 + i] exact, half-integer E and pos; the CLS row of
    every sample keeps its sentinel; with and without the optional Y output"""
    B, Cc, n = PATCH_SPLIT[c.M]
    T = Cc * n
    assert B * T == c.M and lib.dcv_gemm_nt_pick(c.M, c.N, c.K, EPI_PATCH, c.tile) == TILE_NARROW
    d = nt_dev(c.M, c.N, c.K)
    assert_exact("acc + bias + E + pos", c.K, 8, 8, 0.5, extra=3 * 8)
    A, W, bias = _operands(c, d, lay)
    E, pos = halves(Cc, c.N, c.M + 11), halves(1 + n, c.N, c.M + 12)
    Em, posm = (Mat(t.shape[0], c.N, torch.float32, PADS[lay]["f32r"], NAN, t) for t in (E, pos))  # aux and aux2 share ldaux
    y = d.acc + d.bias
    emb = (E[:, None, :] + pos[None, 1:, :]).reshape(T, c.N).cuda().double()
    want = torch.full((B, T + 1, c.N), SENT, device="cuda")
    want[:, 1:] = to_out(y.reshape(B, T, c.N) + emb, torch.float32)
    for with_y in (True, False):
        out = Mat(B * (T + 1), c.N, torch.float32, PADS[lay]["f32o"], SENT)
        Y = Mat(c.M, c.N, torch.float32, PADS[lay]["y"], SENT) if with_y else None
        assert nt_ex(lib, A, W, c.M, c.N, c.K, EPI_PATCH, out, c.tile, c.cap, bias=bias, out2=Y, aux=Em, aux2=posm, T=T, n=n) == 0
        same_bits(out.data, want.reshape(-1, c.N), f"tokens (Y output: {with_y})")
        assert out.untouched()
        if with_y:
            same_bits(Y.data, to_out(y, torch.float32), "Y = acc + bias")
            assert Y.untouched()


def _close(a, b, rtol, atol, what):
    err = (a.double() - b.double()).abs()
    bad = err > atol + rtol * b.double().abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max().item():.4g} (ref max {b.abs().max().item():.4g})"


@pytest.mark.parametrize("c,lay", _with_layouts(LN_CASES))
def test_nt_resid_ln_exact(lib, c, lay):
    """dcv_gemm_nt_resid_ln: x' torch.equal to resid + s (acc + bias), with and without branch_scale, in place and out of place; mean,
    rstd and u against the float64 LayerNorm of that exact x' at the bounds of test_kernels_gpu.py::test_gemm_nt_resid_ln"""
    M, N, K = c.M, 384, c.K
    d = nt_dev(M, N, K)
    assert_exact("resid + s (acc + bias)", K, 8, 8, 0.125, extra=2 * 8 + 32, factor=2.0)
    P = PADS[lay]
    A, W, bias = _operands(NtCase(TILE_WIDE, M, N, K, c.cap), d, lay)
    g = torch.Generator(device="cpu").manual_seed(6)
    gamma_h, beta_h = 1.0 + 0.2 * torch.randn(N, generator=g), 0.3 * torch.randn(N, generator=g)
    gamma, beta = vec(N, NAN, gamma_h), vec(N, NAN, beta_h)
    samples, T = samples_of(M)
    f = torch.tensor(FACTORS[:samples])
    fac = vec(samples, NAN, f)
    eps = 1e-6
    for scaled in (False, True):
        s_rows = f.cuda().double().repeat_interleave(T)[:, None] if scaled else 1.0
        x64 = d.resid + s_rows * (d.acc + d.bias)
        mu = x64.mean(-1)
        var = ((x64 - mu[:, None]) ** 2).mean(-1)
        u64 = (x64 - mu[:, None]) * (var + eps).rsqrt()[:, None] * gamma_h.cuda().double() + beta_h.cuda().double()
        for inplace in (False, True):
            what = f"scaled {scaled}, in place {inplace}"
            x_out = Mat(M, N, torch.float32, P["ln_o"], SENT, d.h["resid"] if inplace else None)
            resid = x_out if inplace else Mat(M, N, torch.float32, P["ln_r"], NAN, d.h["resid"])
            u = Mat(M, N, torch.bfloat16, P["ln_u"], SENT)
            mean, rstd = vec(M, SENT), vec(M, SENT)
            rc = lib.dcv_gemm_nt_resid_ln(A.ptr, A.ld, W.ptr, W.ld, M, N, K, bias.ptr, resid.ptr, resid.ld, fac.ptr if scaled else None,
                                          T if scaled else 0, x_out.ptr, x_out.ld, gamma.ptr, beta.ptr, eps, u.ptr, u.ld, mean.ptr, rstd.ptr,
                                          c.cap, _stream())
            assert rc == 0
            same_bits(x_out.data, to_out(x64, torch.float32), f"x' ({what})")
            _close(mean.data[0], mu, 1e-6, 1e-6 * mu.abs().max().item() + 1e-6, f"mean ({what})")
            _close(rstd.data[0], (var + eps).rsqrt(), 2e-6, 1e-7, f"rstd ({what})")
            _close(u.data, u64, 1e-2, 2e-2, f"u = LayerNorm(x') ({what})")
            for name, m in (("x_out", x_out), ("u", u), ("mean", mean), ("rstd", rstd)):
                assert m.untouched(), f"{name} ({what}): a pad element or guard row was written"


# ---- TN -------------------------------------------------------------------------------------------------------------------------------
class TnItem(C.Structure):  # include/dcv.h: dcv_tn_item
    _fields_ = [("Y", C.c_void_p), ("X", C.c_void_p), ("dW", C.c_void_p), ("dbias", C.c_void_p),
                ("ldy", C.c_int), ("ldx", C.c_int), ("P", C.c_int), ("Q", C.c_int), ("lddw", C.c_int), ("reserved", C.c_int)]


def _assert_256_cus():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    assert n == CUS, f"the restated launch plans are for {CUS} compute units, this device has {n}"


def tn_call(lib, mode, Y, X, M, P, Q, dW, db, tile, ld=None):
    """dcv_gemm_tn_acc_ex (atomic) or dcv_gemm_tn_acc_det with a workspace of exactly the size the library asks for, poisoned with NaN"""
    l = dict(ldy=Y.ld, ldx=X.ld, lddw=dW.ld)
    l.update(ld or {})
    dbp = db.ptr if db is not None else None
    if mode == "atomic":
        return lib.dcv_gemm_tn_acc_ex(Y.ptr, l["ldy"], X.ptr, l["ldx"], M, P, Q, dW.ptr, l["lddw"], dbp, tile, _stream())
    need = lib.dcv_gemm_tn_det_ws_floats(M, P, Q, tile)
    assert need == tn_plan(tile, M, P, Q).ws_floats, "the restated plan and the library disagree on the workspace"
    ws = torch.full((need,), NAN, device="cuda")
    return lib.dcv_gemm_tn_acc_det(Y.ptr, l["ldy"], X.ptr, l["ldx"], M, P, Q, dW.ptr, l["lddw"], dbp, tile, C.c_void_p(ws.data_ptr()), need, _stream())


@pytest.mark.parametrize("c,lay", _with_layouts(TN_CASES))
def test_tn_exact(lib, reduction_mode, c, lay):
    """dcv_gemm_tn_acc_ex / dcv_gemm_tn_acc_det on both tiles: dW and dbias start from integers and end torch.equal to the float64 sums in
    both modes (hence between the modes), from a NaN workspace in the deterministic one"""
    _assert_256_cus()
    M, P, Q = c.M, c.P, c.Q
    assert lib.dcv_gemm_tn_pick(M, P, Q, c.tile) == c.tile
    h = tn_inputs(M, P, Q)
    assert_exact("dW", M, 8, 8, 1.0, extra=100)
    Y, X = (Mat(M, w, torch.bfloat16, PADS[lay]["op"], NAN, h[k]) for k, w in (("Y", P), ("X", Q)))
    want_w = to_out(h["dW0"].cuda().double() + h["Y"].cuda().double().t() @ h["X"].cuda().double(), torch.float32)
    want_b = to_out(h["db0"].cuda().double() + h["Y"].cuda().double().sum(0), torch.float32)
    for with_bias in (True, False):
        dW = Mat(P, Q, torch.float32, PADS[lay]["dw"], SENT, h["dW0"])
        db = vec(P, SENT, h["db0"]) if with_bias else None
        assert tn_call(lib, reduction_mode, Y, X, M, P, Q, dW, db, c.tile) == 0
        same_bits(dW.data, want_w, f"dW ({reduction_mode}, bias {with_bias})")
        assert dW.untouched(), "a pad column or guard row of dW was written"
        if with_bias:
            same_bits(db.data[0], want_b, f"dbias ({reduction_mode})")
            assert db.untouched(), "dbias was written past P"


@pytest.mark.parametrize("M", GROUP_MS)
@pytest.mark.parametrize("lay", LAYOUTS)
def test_tn_group_exact(lib, reduction_mode, M, lay):
    """dcv_gemm_tn_group on a block's four products (one of them without a bias): every dW / dbias torch.equal to the float64 sums in both
    modes — hence equal to the separate launches, which test_tn_exact holds to the same reference"""
    _assert_256_cus()
    assert_exact("dW", M, 8, 8, 1.0, extra=100)
    Yp, Xp = ints(M, 1536, 9000 + M).cuda(), ints(M, 1536, 9001 + M).cuda()  # the items take column ranges of two pools of token rows
    arr = (TnItem * len(GROUP_ITEMS))()
    keep, checks = [], []
    for i, (it, (P, Q, with_bias)) in enumerate(zip(arr, GROUP_ITEMS)):
        y, x = Yp[:, 1536 - P:], Xp[:, :Q]
        dW0, db0 = ints(P, Q, 9100 + i, 100), ints(1, P, 9200 + i, 100)[0]
        Y, X = Mat(M, P, torch.bfloat16, PADS[lay]["op"], NAN, y), Mat(M, Q, torch.bfloat16, PADS[lay]["op"], NAN, x)
        dW = Mat(P, Q, torch.float32, PADS[lay]["dw"], SENT, dW0)
        db = vec(P, SENT, db0) if with_bias else None
        it.Y, it.X, it.dW, it.dbias = Y.ptr.value, X.ptr.value, dW.ptr.value, (db.ptr.value if db is not None else None)
        it.ldy, it.ldx, it.P, it.Q, it.lddw = Y.ld, X.ld, P, Q, dW.ld
        keep.append((Y, X))
        checks.append((dW, to_out(dW0.cuda().double() + y.double().t() @ x.double(), torch.float32),
                       db, to_out(db0.cuda().double() + y.double().sum(0), torch.float32)))
    ptr = C.cast(arr, C.c_void_p)
    ws, need = None, 0
    if reduction_mode == "det":
        need = lib.dcv_gemm_tn_group_ws_floats(ptr, len(GROUP_ITEMS), M)
        assert need == tn_group_plan(GROUP_ITEMS, M)[3], "the restated plan and the library disagree on the workspace"
        ws = torch.full((need,), NAN, device="cuda")
    assert lib.dcv_gemm_tn_group(ptr, len(GROUP_ITEMS), M, C.c_void_p(ws.data_ptr()) if ws is not None else None, need, _stream()) == 0
    for i, (dW, want_w, db, want_b) in enumerate(checks):
        same_bits(dW.data, want_w, f"item {i}: dW ({reduction_mode})")
        assert dW.untouched(), f"item {i}: a pad column or guard row of dW was written"
        if db is not None:
            same_bits(db.data[0], want_b, f"item {i}: dbias ({reduction_mode})")
            assert db.untouched()


def test_tn_plans_match_the_library(lib):
    """the restated tn_plan / tn_group_plan against dcv_gemm_tn_det_ws_floats / dcv_gemm_tn_group_ws_floats on the device"""
    _assert_256_cus()
    for c in TN_CASES:
        assert lib.dcv_gemm_tn_det_ws_floats(c.M, c.P, c.Q, c.tile) == tn_plan(c.tile, c.M, c.P, c.Q).ws_floats, c


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_short_and_unaligned_leading_dimensions(lib):
    """a leading dimension below the width (rows would overlap) -> DCV_ERR_SHAPE, off its alignment -> DCV_ERR_ALIGN, and nothing is
    launched: the outputs keep their sentinel.  The buffers are padded by 72, so a call that slipped through would still stay inside them"""
    M, N, K = 64, 384, 384
    bf, f32 = torch.bfloat16, torch.float32
    A, W, bias = Mat(M, K, bf, 72, 0.0), Mat(N, K, bf, 72, 0.0), vec(N, 0.0)
    outs = []

    def fresh(dtype):
        outs.append(Mat(M, N, dtype, 72, SENT))
        return outs[-1]

    auxb, auxf = Mat(M, N, bf, 72, 0.0), Mat(M, N, f32, 72, 0.0)
    nt = [  # (epilogue, tile, field, value, code)
        (EPI_PLAIN, TILE_NARROW, "lda", K - 8, ERR_SHAPE), (EPI_PLAIN, TILE_WIDE, "ldw", K - 8, ERR_SHAPE), (EPI_PLAIN, TILE_PAIR, "ldo", N - 8, ERR_SHAPE),
        (EPI_PLAIN, TILE_WS, "lda", K - 64, ERR_SHAPE), (EPI_PLAIN, TILE_NARROW, "lda", K + 4, ERR_ALIGN), (EPI_PLAIN, TILE_WIDE, "ldw", K + 4, ERR_ALIGN),
        (EPI_PLAIN, TILE_PAIR, "ldo", N + 4, ERR_ALIGN), (EPI_GELU, TILE_NARROW, "ldo2", N - 8, ERR_SHAPE), (EPI_GELU, TILE_WIDE, "ldo2", N + 4, ERR_ALIGN),
        (EPI_GELU, TILE_WS, "ldo2", N + 4, ERR_ALIGN), (EPI_GELU_BWD, TILE_PAIR, "ldaux", N - 8, ERR_SHAPE), (EPI_GELU_BWD, TILE_NARROW, "ldaux", N + 4, ERR_ALIGN),
        (EPI_GELU_BWD, TILE_WS, "ldaux", N + 4, ERR_ALIGN), (EPI_RESID, TILE_NARROW, "ldaux", N - 4, ERR_SHAPE), (EPI_RESID, TILE_WIDE, "ldaux", N + 2, ERR_ALIGN),
        (EPI_RESID, TILE_WIDE, "ldo", N + 4, ERR_ALIGN),
    ]
    for epi, tile, field, value, code in nt:
        out = fresh(f32 if epi == EPI_RESID else bf)
        out2 = fresh(bf) if epi == EPI_GELU else None
        aux = auxb if epi == EPI_GELU_BWD else auxf if epi == EPI_RESID else None
        assert nt_ex(lib, A, W, M, N, K, epi, out, tile, 0, bias=bias, out2=out2, aux=aux) == 0, (epi, tile)  # the call is good but for the ld
        out.buf.fill_(SENT)
        if out2 is not None:
            out2.buf.fill_(SENT)
        assert nt_ex(lib, A, W, M, N, K, epi, out, tile, 0, bias=bias, out2=out2, aux=aux, ld={field: value}) == code, (epi, tile, field, value)
    # PATCH: aux / aux2 share ldaux, out2 is fp32
    E, pos = Mat(2, N, f32, 72, 0.0), Mat(33, N, f32, 72, 0.0)
    for field, value, code in (("ldaux", N - 4, ERR_SHAPE), ("ldaux", N + 2, ERR_ALIGN), ("ldo2", N - 4, ERR_SHAPE), ("ldo2", N + 2, ERR_ALIGN)):
        out, Y = Mat(M + 1, N, f32, 72, SENT), fresh(f32)
        outs.append(out)
        assert nt_ex(lib, A, W, M, N, K, EPI_PATCH, out, TILE_NARROW, 0, bias=bias, out2=Y, aux=E, aux2=pos, T=64, n=32, ld={field: value}) == code, (field, value)
    # the residual + LayerNorm entry
    gamma, beta = vec(N, 1.0), vec(N, 0.0)
    for field, value, code in (("lda", K - 8, ERR_SHAPE), ("ldw", K - 8, ERR_SHAPE), ("ldr", N - 4, ERR_SHAPE), ("ldo", N - 4, ERR_SHAPE), ("ldu", N - 8, ERR_SHAPE),
                               ("lda", K + 4, ERR_ALIGN), ("ldw", K + 4, ERR_ALIGN), ("ldr", N + 2, ERR_ALIGN), ("ldo", N + 2, ERR_ALIGN), ("ldu", N + 4, ERR_ALIGN),
                               (None, 0, 0)):
        x_out, u, mean, rstd = fresh(f32), fresh(bf), vec(M, SENT), vec(M, SENT)
        l = dict(lda=A.ld, ldw=W.ld, ldr=auxf.ld, ldo=x_out.ld, ldu=u.ld)
        if field:
            l[field] = value
        rc = lib.dcv_gemm_nt_resid_ln(A.ptr, l["lda"], W.ptr, l["ldw"], M, N, K, bias.ptr, auxf.ptr, l["ldr"], None, 0, x_out.ptr, l["ldo"], gamma.ptr,
                                      beta.ptr, 1e-6, u.ptr, l["ldu"], mean.ptr, rstd.ptr, 0, _stream())
        assert rc == code, (field, value)
        if field:
            outs.extend((mean, rstd))
        else:
            outs.pop(), outs.pop()  # the good call wrote its outputs
    # the weight-gradient entries
    P, Q = 384, 128
    Y, X = Mat(M, P, bf, 72, 0.0), Mat(M, Q, bf, 72, 0.0)
    for mode in ("atomic", "det"):
        for tile in (TILE_NARROW, TILE_WIDE):
            for field, value, code in (("ldy", P - 8, ERR_SHAPE), ("ldx", Q - 8, ERR_SHAPE), ("lddw", Q - 4, ERR_SHAPE), ("ldy", P + 4, ERR_ALIGN),
                                       ("ldx", Q + 4, ERR_ALIGN)) + ((("lddw", Q + 2, ERR_ALIGN),) if mode == "det" else ()):
                dW = Mat(P, Q, f32, 72, SENT)
                outs.append(dW)
                assert tn_call(lib, mode, Y, X, M, P, Q, dW, None, tile, ld={field: value}) == code, (mode, tile, field, value)
    for field, value, code in (("ldy", P - 8, ERR_SHAPE), ("ldx", Q - 8, ERR_SHAPE), ("lddw", Q - 4, ERR_SHAPE), ("ldy", P + 4, ERR_ALIGN), ("ldx", Q + 4, ERR_ALIGN)):
        dW = Mat(P, Q, f32, 72, SENT)
        outs.append(dW)
        arr = (TnItem * 1)()
        arr[0].Y, arr[0].X, arr[0].dW, arr[0].dbias = Y.ptr.value, X.ptr.value, dW.ptr.value, None
        arr[0].ldy, arr[0].ldx, arr[0].P, arr[0].Q, arr[0].lddw = Y.ld, X.ld, P, Q, dW.ld
        setattr(arr[0], field, value)
        assert lib.dcv_gemm_tn_group(C.cast(arr, C.c_void_p), 1, M, None, 0, _stream()) == code, ("group", field, value)
    torch.cuda.synchronize()
    for m in outs:
        assert bool((m.buf == SENT).all()), "a refused call launched a kernel"
