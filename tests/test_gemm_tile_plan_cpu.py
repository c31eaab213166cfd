"""dcv_gemm_nt384_plan, the row-tile plan of the 256 x 384 NT GEMM (host logic, no GPU call): rows [0, 256 n256) in 256-row tiles, the rest
in n192 tiles of 192 rows.  Tile L = (row tile L // tiles_n, column tile L % tiles_n) goes to workgroup L % grid in round L // grid, as the
kernel walks them.  The old plan (256-row tiles only) is recomputed here from ceil(M / 256)."""
import ctypes as C

import numpy as np
import pytest

HEADLINE_M = 64 * 1569
GRIDS = (1, 3, 4, 8, 248, 256)
WIDTHS = (384, 1152, 1536)


@pytest.fixture(scope="module")
def plan():
    import os
    from diverse_channel_vit_amd import _build, hip
    if not os.path.exists(hip.LIB_PATH):
        _build.build(verbose=False)
    lib = hip.load()

    def f(M, N, grid):
        a, b = C.c_int(-1), C.c_int(-1)
        assert lib.dcv_gemm_nt384_plan(M, N, grid, C.byref(a), C.byref(b)) == 0
        return a.value, b.value
    return f


def _walk(heights_m, tiles_n, grid):
    """(most tiles, most rows) a workgroup walks: tile L has the height of row tile L // tiles_n and belongs to workgroup L % grid"""
    h = np.repeat(np.asarray(heights_m, dtype=np.int64), tiles_n)
    rounds = -(-len(h) // grid)
    h = np.concatenate([h, np.zeros(rounds * grid - len(h), dtype=np.int64)]).reshape(rounds, grid)
    return int((h > 0).sum(0).max()), int(h.sum(0).max())


def _m_values():
    near64 = {m + d for m in range(64, 3000, 64) for d in (-1, 0, 1)}
    edges = {m + d for m in (HEADLINE_M, 2 * HEADLINE_M - 1, 200_000, 256 * 256, 256 * 448, 248 * 448, 256 * 512) for d in (-1, 0, 1) if m + d <= 200_000}
    return sorted(near64 | edges | set(range(1, 600)) | set(range(600, 3000, 7)) | set(range(3000, 200_001, 389)))


def test_plan_covers_rows_and_never_walks_more(plan):
    checked = engaged = 0
    for M in _m_values():
        old_m = -(-M // 256)
        for N in WIDTHS:
            tn = N // 384
            for grid in GRIDS:
                n256, n192 = plan(M, N, grid)
                assert n256 >= 0 and n192 >= 0 and n256 + n192 >= 1, (M, N, grid, n256, n192)
                # row tiles: starts 256 i, then 256 n256 + 192 j — contiguous by construction; they cover [0, M) exactly once when the
                # last one starts below M and ends at or beyond it
                starts = [256 * i for i in range(n256)] + [256 * n256 + 192 * j for j in range(n192)]
                heights = [256] * n256 + [192] * n192
                assert starts[0] == 0 and all(s + h == s2 for s, h, s2 in zip(starts, heights, starts[1:])), (M, N, grid)
                assert starts[-1] < M <= starts[-1] + heights[-1], (M, N, grid, n256, n192)
                old_tiles, old_rows = _walk([256] * old_m, tn, grid)
                new_tiles, new_rows = _walk(heights, tn, grid)
                assert new_tiles <= old_tiles, (M, N, grid, n256, n192)
                assert new_rows <= old_rows, (M, N, grid, n256, n192)
                if n192:
                    assert new_rows < old_rows, (M, N, grid, n256, n192)  # a mixed plan only where it lowers the longest walk
                    engaged += 1
                else:
                    assert n256 == old_m, (M, N, grid, n256)  # otherwise exactly the old plan
                if old_m * tn <= grid:
                    assert n192 == 0, (M, N, grid)  # one round or less
                checked += 1
    assert checked > 25_000 and engaged > 2_500


@pytest.mark.parametrize("grid", [256, 248])
def test_plan_headline(plan, grid):
    """M = 100 416 rows, one column tile: 512 rows per workgroup under the old plan (393 tiles, two rounds), at most 448 now — with the
    full grid and with the CUs the data-parallel backward leaves to the collectives (dp.reserved_cus: 248 workgroups)"""
    n256, n192 = plan(HEADLINE_M, 384, grid)
    assert n192 > 0 and 256 * n256 + 192 * n192 >= HEADLINE_M
    tiles, rows = _walk([256] * n256 + [192] * n192, 1, grid)
    assert tiles == 2 and rows <= 448
    assert _walk([256] * 393, 1, grid) == (2, 512)


def test_plan_refuses_bad_arguments(plan):
    from diverse_channel_vit_amd import hip
    lib = hip.load()
    a, b = C.c_int(), C.c_int()
    assert lib.dcv_gemm_nt384_plan(1000, 200, 4, C.byref(a), C.byref(b)) < 0   # N % 384 != 0
    assert lib.dcv_gemm_nt384_plan(0, 384, 4, C.byref(a), C.byref(b)) < 0
    assert lib.dcv_gemm_nt384_plan(1000, 384, 0, C.byref(a), C.byref(b)) < 0
    assert lib.dcv_gemm_nt384_plan(1000, 384, 4, None, C.byref(b)) < 0
