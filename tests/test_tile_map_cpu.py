"""The FP64 Gram kernel's workgroup -> tile maps (csrc/hip/tile_map.h), exhaustively, on the CPU.

rbf_gram_kernel turns blockIdx.x into its output tile with xcd_remap followed by the GROUP_M band map
(rectangular launch) or by tri_tile (upper-triangle launch).  The header compiles for the host as well and the
core library exports the composed maps, so these are the kernel's own functions.  A map that is no bijection
computes one tile twice and leaves another unwritten: on the device that only shows as a slightly wrong
prediction.
"""

import numpy as np
import pytest

from svm355 import _native as N


def _assert_bijection(codes: np.ndarray, expected: np.ndarray, what: str) -> None:
    """codes: one integer per workgroup naming its tile; expected: the sorted codes of every tile."""
    got = np.sort(codes)
    if not np.array_equal(got, expected):
        missing = np.setdiff1d(expected, got)
        extra = np.setdiff1d(got, expected)
        dup = got[1:][got[1:] == got[:-1]]
        raise AssertionError(f"{what}: {missing.size} tiles never computed (first {missing[:4]}), {extra.size} outside "
                             f"the grid (first {extra[:4]}), {np.unique(dup).size} computed more than once")


def test_rect_map_is_a_bijection_onto_the_grid():
    """tiles_m = 1..64 x tiles_n = 1..32: every band shape -- fewer than one band, whole bands, a partial last band
    of 1..7 row tiles -- with workgroup counts on both sides of every multiple of 8 (xcd_remap's remainder)."""
    for tiles_m in range(1, 65):
        for tiles_n in range(1, 33):
            tm, tn = N.tile_map("rect", tiles_m, tiles_n)
            assert tm.shape == tn.shape == (tiles_m * tiles_n,)
            inside = (tm >= 0) & (tm < tiles_m) & (tn >= 0) & (tn < tiles_n)
            assert inside.all(), f"{tiles_m} x {tiles_n}: tile {tm[~inside][0], tn[~inside][0]} outside the grid"
            _assert_bijection(tm * tiles_n + tn, np.arange(tiles_m * tiles_n), f"rect {tiles_m} x {tiles_n}")


def _tri_codes(T: int) -> np.ndarray:
    r, c = np.triu_indices(T)
    return r * T + c  # row-major upper triangle: ascending


@pytest.mark.parametrize("Ts", [range(1, 257), (469,), (3907,)], ids=["1-256", "469", "3907"])
def test_tri_map_is_a_bijection_onto_the_upper_triangle(Ts):
    """T = 469 is the 60k-row Gram, T = 3907 a 500k-row one (7.6 M tiles: the sqrt seed far from small ids)."""
    for T in Ts:
        tm, tn = N.tile_map("tri", T)
        assert tm.shape == tn.shape == (T * (T + 1) // 2,)
        inside = (tm >= 0) & (tm <= tn) & (tn < T)
        assert inside.all(), f"T = {T}: tile {tm[~inside][0], tn[~inside][0]} outside the upper triangle"
        _assert_bijection(tm * T + tn, _tri_codes(T), f"tri T = {T}")


def test_tile_map_ref_refuses_bad_arguments():
    z = np.zeros(4, dtype=np.int64)
    for kind, id0, count, tiles_m, tiles_n in [(2, 0, 1, 1, 1), (0, 0, 5, 2, 2), (0, -1, 1, 2, 2), (0, 0, 1, 0, 2),
                                               (0, 0, 1, 2, 0), (1, 0, 4, 2, 1)]:
        assert N.core().svm_tile_map_ref(kind, id0, count, tiles_m, tiles_n, N.ptr(z), N.ptr(z)) != 0
