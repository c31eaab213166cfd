"""The case tables of tests/test_stream_kernels_gpu.py against the launch plans of the streaming kernels (restated there from csrc/norm.hip,
csrc/optim.hip, csrc/tokenizer.hip and csrc/dcv_common.hpp): every regime of every grid-stride walk is in its table, removing a row fails
a test here, the workspace-size entries of the library agree with the restated grids, and no shape of the older kernel-level tests walks
its loop twice.  Runs without a GPU (the library is loaded for its host-side size queries only)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stream_kernels_gpu as T  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from diverse_channel_vit_amd import hip
    return hip.load()


def test_plans_restate_the_launch_arithmetic():
    """Hand-checked values, and every cap and threshold read from the sources, re-derived from the restated plans."""
    # ln_fwd: 4096 workgroups = 16 384 rows; the first size past it gives one wave a second row
    assert T.ln_fwd_plan(16384) == (4096, 16384, 1, 1) and T.ln_fwd_plan(16385) == (4096, 16384, 2, 1)
    assert T.ln_fwd_plan(T.HEADLINE_M) == (4096, 16384, 7, 6)
    assert max(M for M in range(16000, 16500) if T.ln_fwd_plan(M).rows_max == 1) == 16384
    # ln_bwd: 1024 workgroups = 4096 rows; the paired loop first runs at M = 4097
    assert T.ln_bwd_plan(4096) == (1024, 4096, {(0, 1)}) and T.ln_bwd_plan(4097) == (1024, 4096, {(0, 1), (1, 0)})
    assert max(M for M in range(3000, 5000) if all(p == 0 for p, _ in T.ln_bwd_plan(M).classes)) == 4096
    assert T.ln_bwd_plan(8192).classes == {(1, 0)} and T.ln_bwd_plan(8193).classes == {(1, 0), (1, 1)}
    assert T.ln_bwd_plan(12293).classes == {(1, 1), (2, 0)} and T.ln_bwd_plan(T.HEADLINE_M).classes == {(12, 0), (12, 1)}
    assert T.ln_bwd_plan(1001).classes == {(0, 1), (0, 0)}
    # det_reduce: tall from 32 parts; its unrolled loop from 449 parts = LayerNorm M >= 1793
    assert not T.det_reduce_plan(31, 384, 384, 384, 384, 768).tall and T.det_reduce_plan(32, 384, 384, 384, 384, 768).tall
    assert not T.det_reduce_plan(448, 384, 384, 384, 384, 768).unrolled and T.det_reduce_plan(449, 384, 384, 384, 384, 768).unrolled
    assert min(M for M in range(1, 3000) if T.ln_bwd_det_plan(M, 384).tall and T.ln_bwd_det_plan(M, 384).unrolled) == 1793
    assert T.det_reduce_plan(7, 8, 4, 4, 0, 8) == (False, True, False, True, 2, 1) and T.det_reduce_plan(8, 8, 4, 4, 0, 8)[2:4] == (True, False)
    # 1024 parts: two unrolled rounds and nothing left; 750: one round, then parts 512 + pl, 576 + pl, ... one at a time
    assert T.det_reduce_plan(1024, 384, 384, 384, 384, 768)[2:4] == (True, False) and T.det_reduce_plan(750, 384, 384, 384, 384, 768)[2:4] == (True, True)
    assert T.det_reduce_plan(250, 384, 384, 384, 384, 768)[2:4] == (False, True)
    assert not T.det_reduce_plan(1024, 768, 768, 768, 768, 1536, aligned=False).vec and not T.det_reduce_plan(8, 1, 1, 1, 0, 1).vec
    assert not T.det_reduce_plan(64, 4 * 16385, 4, 4, 0, 4 * 16385).tall  # more than 16 384 column groups: the flat form whatever the part count
    # the flat kernels: caps in floats
    assert {k: 4 * 256 * c for k, c in T.FLAT_CAPS.items()} == {"adamw": 4194304, "clip_scale": 4194304, "cast_bf16": 8388608, "sumsq": 1048576}
    assert T.flat_plan(4194304, 4096) == (4096, 1048576, 1, 0, 0, 1) and T.flat_plan(4194308, 4096).iters_max == 2
    assert T.flat_plan(2 * 4194304 + 4 * 777 + 3, 4096) == (4096, 2097929, 2, 777, 3, 3)
    assert T.flat_plan(3, 4096) == (1, 0, 0, 0, 3, 0)
    assert T.flat_plan(3_400_000, 1024).iters_max == 4  # the one older size past a cap (sumsq), compared at 1e-5 n
    # gather / im2col: 8192 workgroups = 2 097 152 threads
    assert T.gather_plan(64, 1569, 785, 384) == (4823040, 8192, 2, 628736) and T.im2col_plan(64, 8, 224, 224, 16) == (6422528, 8192, 3, 131072)
    # patch_bwd: bpar = 256 / (D / 4)
    assert [T.patch_bwd_plan(4, 2, 4, D).bpar for D in (1024, 516, 384, 192, 4)] == [1, 1, 2, 5, 256]
    p = T.patch_bwd_plan(64, 8, 196, 384)
    assert (p.grid_x, p.grid_y, p.bpar, p.idle_threads, p.ragged_block, p.batches_max) == (98, 9, 2, 64, False, 32)
    assert T.ortho_plan(64, 8, 196, 384)[:3] == (7, 512, False) and T.ortho_plan(3, 5, 30, 384)[:3] == (2, 15, True)


def test_workspace_sizes_reproduce_the_restated_grids(lib):
    """dcv_*_det_ws_floats through the loaded library (host logic only) against the restated plans."""
    for M, D in [(c.M, c.D) for c in T.LN_CASES] + [(1, 4), (4095, 384), (4099, 1024), (10 ** 6, 768)]:
        assert lib.dcv_ln_bwd_det_ws_floats(M, D) == T.ln_bwd_ws_floats(M, D), (M, D)
    for n in T.SUMSQ_N + [4, 1023, 1024, 1025, 1048575, 1048577, 10 ** 9]:
        assert lib.dcv_sumsq_det_ws_floats(n) == T.sumsq_ws_floats(n), n
    for c in T.PATCH_CASES + [T.PatchCase(16, 8, 196, 768), T.PatchCase(2, 1, 1, 8)]:
        assert lib.dcv_patch_bwd_det_ws_floats(*c) == T.patch_bwd_plan(*c).ws_floats, c
    for c in T.ORTHO_CASES + [T.OrthoCase(16, 8, 196, 384), T.OrthoCase(1, 1, 28, 4), T.OrthoCase(1, 1, 29, 4)]:
        assert lib.dcv_ortho_fwd_det_ws_floats(*c) == T.ortho_plan(*c).ws_floats, c


def _ln_sig(c):
    d = T.ln_bwd_det_plan(c.M, c.D, not c.misaligned)
    return (T.ln_fwd_plan(c.M).rows_max, tuple(sorted(T.ln_bwd_plan(c.M).classes)), "tall" if d.tall else "flat",
            ("unrolled+rest" if d.remainder else "unrolled") if d.unrolled else "plain",
            "vec" if d.vec else "scalar", c.D, "f32" if c.du_f32 else "bf16", c.dx_in)


def test_layernorm_table_covers_every_regime():
    """Every row stands for a regime of its own (removing one changes the list below), and the regimes of both walks are all there."""
    sigs = [_ln_sig(c) for c in T.LN_CASES]
    assert len(set(sigs)) == len(sigs)
    assert [(s[0], s[1], s[2], s[3], s[4]) for s in sigs] == [
        (1, ((0, 1),), "flat", "plain", "scalar"), (1, ((0, 1),), "flat", "plain", "vec"),
        (1, ((0, 1),), "flat", "unrolled+rest", "scalar"), (1, ((0, 1),), "flat", "unrolled+rest", "vec"),
        (1, ((0, 0), (0, 1)), "tall", "plain", "scalar"), (1, ((0, 1),), "tall", "plain", "vec"),
        (1, ((0, 1),), "tall", "unrolled+rest", "vec"), (1, ((0, 1),), "tall", "unrolled", "vec"), (1, ((0, 1), (1, 0)), "tall", "unrolled", "vec"),
        (1, ((1, 0),), "tall", "unrolled", "vec"), (1, ((1, 0), (1, 1)), "tall", "unrolled", "scalar"),
        (1, ((1, 1), (2, 0)), "tall", "unrolled", "scalar"), (1, ((2, 0),), "tall", "unrolled", "vec"),
        (2, ((2, 0), (2, 1)), "tall", "unrolled", "vec"), (3, ((4, 1), (5, 0)), "tall", "unrolled", "vec"),
        (7, ((12, 0), (12, 1)), "tall", "unrolled", "vec"), (7, ((12, 0), (12, 1)), "tall", "unrolled", "scalar")]
    Ms = [c.M for c in T.LN_CASES]
    # ln_fwd: exactly at the cap, cap + 1, two full rounds and a ragged one, the headline size
    assert 16384 in Ms and 16385 in Ms and T.HEADLINE_M in Ms
    assert any(T.ln_fwd_plan(M).rows_min >= 2 and T.ln_fwd_plan(M).rows_max == T.ln_fwd_plan(M).rows_min + 1 and M < T.HEADLINE_M for M in Ms)
    # ln_bwd: at the cap, cap + 1; waves with 0, 1 and >= 2 pairs, with and without the trailing row, mixed in one launch
    assert 4096 in Ms and 4097 in Ms
    launches = {T.ln_bwd_plan(M).classes for M in Ms}
    for pairs in (0, 1, 2):
        assert any({(pairs, 0), (pairs, 1)} <= {(min(p, 2), s) for p, s in cl} for cl in launches)
        assert any((pairs, 0) in {(min(p, 2), s) for p, s in cl} for cl in launches) and any((pairs, 1) in {(min(p, 2), s) for p, s in cl} for cl in launches)
    assert any({(0, 1), (1, 0)} <= cl for cl in launches) and any({(1, 0), (1, 1)} <= cl for cl in launches) and any({(1, 1), (2, 0)} <= cl for cl in launches)
    # every D, both du types, all three dx_in forms; the DropPath row scale runs on every case (rows_per_sample 1569 at the headline size)
    assert {c.D for c in T.LN_CASES} == {384, 768, 192, 1024, 516, 4}
    assert {(c.du_f32, c.dx_in) for c in T.LN_CASES} == {(a, b) for a in (True, False) for b in ("given", "none", "alias")}
    assert T.HEADLINE_M % 1569 == 0
    assert any(c.D > 512 and max(p for p, _ in T.ln_bwd_plan(c.M).classes) >= 2 for c in T.LN_CASES)  # the four-register kernel past the cap too
    # the strided calls: the final norm's (M = B rows, N D apart) and padded rows past ln_bwd's cap
    assert (64, 384, 1569 * 384) in T.LN_STRIDED and any(s == D + 4 and M > 4096 for M, D, s in T.LN_STRIDED)
    assert all(s % 4 == 0 and s >= D for _, D, s in T.LN_STRIDED)
    assert [(s == D + 4, M > 4096, D > 512) for M, D, s in T.LN_STRIDED] == [(False, False, False), (True, True, False), (True, True, True)]  # both register widths


def test_det_reduce_regimes_are_all_reached():
    """flat / tall x plain / unrolled x vector / scalar over every det_reduce launch the tables cause; the tall scalar form also from the
    gradient norm (one column), the flat form with many parts from the diversity statistics' wide rows."""
    jobs = T.det_jobs()
    assert {(p.tall, p.unrolled, p.vec) for _, p in jobs} == {(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)}
    # the one-at-a-time loop alone, the unrolled loop alone, and one after the other - in both forms
    assert {(p.tall, p.unrolled, p.remainder) for _, p in jobs} == {(a, u, r) for a in (True, False) for u, r in ((False, True), (True, False), (True, True))}
    assert sum(1 for w, p in jobs if w.startswith("ln_bwd") and p.tall and p.unrolled and p.remainder) == 1  # M = 3000 alone holds this regime for LayerNorm
    ln = {(p.tall, p.unrolled, p.vec) for w, p in jobs if w.startswith("ln_bwd")}
    assert len(ln) == 8  # LayerNorm alone reaches all eight
    assert any(w.startswith("sumsq") and p.tall and p.unrolled and not p.vec and p.nv == 1 for w, p in jobs)
    assert any(w.startswith("sumsq") and not p.tall for w, p in jobs)
    assert any(w.startswith("patch dE") and p.tall for w, p in jobs) and any(w.startswith("patch dpos") and not p.tall and p.unrolled for w, p in jobs)
    assert any(w.startswith("ortho") and not p.tall and p.nv > 16384 for w, p in jobs)


def test_flat_tables_cover_every_regime():
    want = {"scalar only", "below cap", "at cap", "cap + 1", "rounds + ragged"}
    for kernel, table in (("adamw", T.ADAMW_N), ("cast_bf16", T.CAST_N), ("sumsq", T.SUMSQ_N)):
        cap = T.FLAT_CAPS[kernel]
        regimes = [T.flat_regime(n, cap) for n in table]
        assert want <= set(regimes), (kernel, regimes)
        assert {n % 4 for n in table if n >= 4} == {0, 1, 2, 3} and any(n < 4 for n in table), kernel
        assert len(set(table)) == len(table) and table == sorted(table)
        assert any(n >= T.ARENA_FLOATS for n in table), kernel  # the headline size
    # one signature per row: removing a row changes the list
    assert [(T.flat_regime(n, 4096), n % 4) for n in T.ADAMW_N] == [
        ("scalar only", 1), ("scalar only", 3), ("below cap", 1), ("below cap", 2), ("below cap", 0), ("at cap", 0), ("cap + 1", 2),
        ("rounds + ragged", 3), ("rounds + ragged", 1)]
    assert [(T.flat_regime(n, 8192), n % 4) for n in T.CAST_N] == [
        ("scalar only", 2), ("below cap", 1), ("at cap", 0), ("cap + 1", 3), ("past cap", 2), ("rounds + ragged", 1), ("rounds + ragged", 0)]
    assert [(T.flat_regime(n, 1024), n % 4) for n in T.SUMSQ_N] == [
        ("scalar only", 1), ("scalar only", 2), ("scalar only", 3), ("below cap", 2), ("at cap", 0), ("cap + 1", 1), ("rounds + ragged", 3),
        ("rounds + ragged", 0), ("rounds + ragged", 0), ("rounds + ragged", 1)]
    assert 2 * 4194304 + 4 * 777 + 3 in T.ADAMW_N and 8388608 + 4 * 333 + 2 in T.CAST_N  # two full rounds, a ragged one and a scalar tail; one round and a ragged one
    # sumsq: exactness needs fewer than 2^23 non-zeros whatever n: the test's density rule
    for n in T.SUMSQ_N:
        assert 1000 + min(0.6, 3.0e6 / n) * n * 1.01 + 100003 < 2 ** 23
    assert any(n < 2 ** 24 and T.flat_plan(n, 1024).iters_max >= 15 for n in T.SUMSQ_N)


def test_gather_and_im2col_tables_cover_every_regime():
    g = [T.stride_regime(T.gather_plan(*c), T.GATHER_CAP) for c in T.GATHER_CASES]
    assert g == ["rounds + ragged", "at cap", "cap + 1", "below cap", "below cap", "below cap"]
    assert T.GatherCase(64, 1569, 785, 384) in T.GATHER_CASES
    below = [c for c, r in zip(T.GATHER_CASES, g) if r == "below cap"]
    assert [(c.Nk == 1, c.D == 4, c.Nk == c.N) for c in below] == [(True, False, False), (False, True, False), (False, False, True)]
    assert any(c.Nk == c.N for c in T.GATHER_CASES) and all(c.Nk <= c.N and c.D % 4 == 0 for c in T.GATHER_CASES)
    i = [(T.stride_regime(T.im2col_plan(c.B, c.C, c.H, c.W, c.P), T.IM2COL_CAP), c.u8, c.H % c.P != 0) for c in T.IM2COL_CASES]
    assert i == [("rounds + ragged", False, False), ("rounds + ragged", True, False), ("at cap", False, False), ("cap + 1", False, False),
                 ("below cap", False, True), ("below cap", True, True)]
    assert T.Im2colCase(64, 10, 8, 224, 224, 16, False) in T.IM2COL_CASES
    assert all(c.P % 4 == 0 and c.W % 4 == 0 and c.C <= c.Ct for c in T.IM2COL_CASES) and any(c.H != c.W for c in T.IM2COL_CASES)
    # im2col's thread count is a multiple of 4 (full patches of a width that is a multiple of 4): cap + 4 is the first size past the cap
    assert T.im2col_plan(1, 3, 4, 699052, 4).threads == 256 * 8192 + 4


def test_patch_and_ortho_tables_cover_every_regime():
    plans = [(c, T.patch_bwd_plan(*c)) for c in T.PATCH_CASES]

    def rel(c, p):
        return "below" if c.B < p.bpar else "equal" if c.B == p.bpar else "multiple" if c.B % p.bpar == 0 else "ragged"

    assert [(p.bpar, rel(c, p), c.n % 2) for c, p in plans] == [
        (2, "multiple", 0), (2, "below", 1), (2, "equal", 1), (2, "ragged", 1), (5, "below", 1), (5, "equal", 0), (5, "ragged", 1),
        (1, "equal", 1), (1, "multiple", 1), (256, "below", 0)]
    for bpar in (2, 5):
        assert {rel(c, p) for c, p in plans if p.bpar == bpar} >= {"below", "equal", "ragged"}
    assert {rel(c, p) for c, p in plans if p.bpar == 1} == {"equal", "multiple"}  # B below 1 does not exist
    assert any(p.idle_threads == 127 for _, p in plans) and any(p.batches_max >= 32 for _, p in plans)
    assert any(p.batches_min == 0 for _, p in plans) and any(p.batches_max > p.batches_min > 0 for _, p in plans)
    assert T.PatchCase(64, 8, 196, 384) in T.PATCH_CASES
    # the exactness condition of test_patch_bwd_exact, worst case
    assert all(8 * c.B * max(c.n, c.C) + 100 < 2 ** 23 for c in T.PATCH_CASES)
    o = [(c.B * c.C >= 512, T.ortho_plan(*c).ragged_chunk, c.C == 1) for c in T.ORTHO_CASES]
    assert o == [(True, False, False), (False, True, False), (False, True, True)]
    assert T.OrthoCase(64, 8, 196, 384) in T.ORTHO_CASES


def test_the_older_kernel_level_shapes_stay_below_the_caps():
    """The gap these tests close: test_layernorm's shapes give every wave one row (no pair, no second round, the unrolled tall loop never),
    and test_adamw_and_casts' n gives every thread one float4."""
    shapes, n = T.older_test_sizes()
    assert len(shapes) >= 3
    for M, D in shapes:
        assert T.ln_fwd_plan(M).rows_max == 1, (M, D)
        assert all(p == 0 for p, _ in T.ln_bwd_plan(M).classes), (M, D)
        d = T.ln_bwd_det_plan(M, D)
        assert d.vec and not (d.tall and d.unrolled), (M, D)
    assert max(M for M, _ in shapes) == 1000 and T.ln_bwd_plan(1000).grid == 250
    for kernel in ("adamw", "cast_bf16"):
        assert T.flat_plan(n, T.FLAT_CAPS[kernel]).iters_max == 1 and T.flat_regime(n, T.FLAT_CAPS[kernel]) == "below cap"


def test_every_case_fits_in_six_gigabytes():
    worst = {}
    for kind, table in (("ln", T.LN_CASES), ("adamw", T.ADAMW_N), ("cast", T.CAST_N), ("sumsq", T.SUMSQ_N), ("gather", T.GATHER_CASES),
                        ("im2col", T.IM2COL_CASES), ("patch", T.PATCH_CASES), ("ortho", T.ORTHO_CASES)):
        worst[kind] = max(T.case_bytes(kind, c) for c in table)
        assert worst[kind] < 6e9, (kind, worst[kind])
    assert max(M * s * 4 * 4 for M, _, s in T.LN_STRIDED) < 6e9
