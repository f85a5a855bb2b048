"""CPU test of the launch plan of the SYRK behind the dense KKT assembly and A^T A (csrc/dense_kernels.hip: syrk_plan, read by launch_syrk_t), fetched through
the host-only C-ABI call pq_debug_syrk_plan.  Without a device the library plans for 256 CUs = 512 resident workgroup slots, the MI355X's figures.

tests/test_dense_assembly_gpu.py compares the assembled matrix with NumPy at the smallest shape that reaches each branch of the launcher; this file pins, shape
by shape, that the branch is really reached: the arithmetic of the heuristics is restated below (expected_plan) and both the restatement and the library have to
give the tuple written beside the shape in tests/assembly_shapes.py.  When a heuristic changes, this test names the shapes that became vacuous."""
import ctypes as C

import pytest

from assembly_shapes import GRID, shape_id
from piqp_amd import _lib

TS, BK, SLOTS = 128, 16, 2 * 256  # tile size, columns per K stage, resident workgroups of k_syrk_lower<.., 2, 2> on 256 CUs (2 per CU)


def plan(n, kdim, with_workspace):
    out = (C.c_int * 6)()
    assert _lib.load().pq_debug_syrk_plan(n, kdim, int(with_workspace), C.byref(out)) == 0
    return tuple(out)


def expected_plan(n, kdim, with_workspace):
    """launch_syrk_t's decisions for 512 slots, restated"""
    T = -(-n // TS)
    ntiles = T * (T + 1) // 2
    low_latency = kdim <= 256
    tile_order = T >= 16 and not low_latency
    rem, k_split = 0, 1
    # tail: the tiles of the last, partial round of workgroups, when that round would fill < 60 % of the slots, are split along K into as many slices as fit in the
    # idle slots -- but no slice shorter than 4 K stages
    if with_workspace and ntiles > SLOTS and 0 < (ntiles % SLOTS) * 10 < SLOTS * 6:
        s = min(SLOTS // (ntiles % SLOTS), -(-kdim // BK) // 4)
        if s >= 2:
            rem, k_split = ntiles % SLOTS, s
    return (T, ntiles, int(low_latency), int(tile_order), rem, k_split)


def slices(kdim, k_split):
    """K stages per slice as syrk_lower_body cuts them: kt_per = ceil(nkt / k_split), slice s = stages [s kt_per, min(nkt, (s + 1) kt_per))"""
    nkt = -(-kdim // BK)
    kt_per = -(-nkt // k_split)
    return [max(0, min(nkt, (s + 1) * kt_per) - s * kt_per) for s in range(k_split)]


@pytest.mark.parametrize("shape", GRID, ids=shape_id)
def test_every_assembly_shape_reaches_its_branch(shape):
    if shape.assembly is not None:
        assert expected_plan(shape.n, shape.m, True) == shape.assembly, shape.branch
        assert plan(shape.n, shape.m, True) == shape.assembly, shape.branch
    else:
        assert shape.m == 0
    if shape.ata is not None:
        assert expected_plan(shape.n, shape.p, False) == shape.ata, shape.branch
        assert plan(shape.n, shape.p, False) == shape.ata, shape.branch
    else:
        assert shape.p == 0


def test_the_arithmetic_behind_the_pinned_plans():
    """the figures the branch descriptions of tests/assembly_shapes.py quote, worked out"""
    # T = 15 | 16 | 17: 1920 = 15 * 128, 1921 and 1922 need a 16th tile row of 1 and 2 rows, 2176 = 17 * 128; 120, 136, 153 tiles all fit in one round of 512 slots
    assert [-(-n // TS) for n in (1920, 1921, 1922, 2176)] == [15, 16, 16, 17] and 17 * 18 // 2 == 153 == 8 * 19 + 1
    # n = 4096: 32 * 33 / 2 = 528 = 512 + 16; 16 * 10 < 512 * 6; 512 // 16 = 32 slices would fit, m = 128 has 8 stages and 8 // 4 = 2 -> k_split = 2, slices of 4 + 4
    assert 32 * 33 // 2 - SLOTS == 16 and min(SLOTS // 16, (128 // BK) // 4) == 2 and slices(128, 2) == [4, 4]
    # n = 4100: T = 33 (the last tile row has 4100 - 32 * 128 = 4 rows), 33 * 34 / 2 = 561 = 512 + 49; 512 // 49 = 10
    assert -(-4100 // TS) == 33 and 4100 - 32 * TS == 4 and 33 * 34 // 2 - SLOTS == 49 and SLOTS // 49 == 10
    #   m = 200: 13 stages (12 full + 8 columns), 13 // 4 = 3 -> k_split = 3, kt_per = 5: slices of 5 / 5 / 3
    assert -(-200 // BK) == 13 and 200 - 12 * BK == 8 and min(10, 13 // 4) == 3 and slices(200, 3) == [5, 5, 3]
    #   m = 520: 33 stages (32 full + 8 columns), 33 // 4 = 8 -> k_split = 8, kt_per = 5: slices 0..5 have 5 stages, slice 6 stages 30, 31, 32 (the last one ragged), and
    #   slice 7 would begin at stage 35 of 33: empty, its partial tiles are zeros that the reduction still adds
    assert -(-520 // BK) == 33 and 520 - 32 * BK == 8 and min(10, 33 // 4) == 8 and slices(520, 8) == [5, 5, 5, 5, 5, 5, 3, 0]
    # the split workspace of the largest case: 49 tiles x 8 slices x 128 x 128 doubles = 51 MB
    assert 49 * 8 * TS * TS * 8 == 51380224


@pytest.mark.parametrize("n,kdim", [(1920, 272), (1921, 272), (1921, 256), (2048, 257), (4096, 512), (4096, 4096), (4100, 520)])
def test_without_the_workspace_nothing_is_split(n, kdim):
    """A^T A and the trailing updates pass no workspace: same shape and table, no tail"""
    with_ws, without = plan(n, kdim, True), plan(n, kdim, False)
    assert without[:4] == with_ws[:4] and without[4:] == (0, 1)
    assert with_ws == expected_plan(n, kdim, True)


def test_the_flagship_shape_keeps_its_tail():
    """n = m = 4096 (the bench line): 256 K stages, min(512 // 16, 256 // 4) = 32 -> 16 tail tiles in 32 slices of 8 stages"""
    assert plan(4096, 4096, True) == (32, 528, 0, 1, 16, 32)
    assert plan(4096, 512, True) == (32, 528, 0, 1, 16, 8)  # tests/test_dense_gpu.py::test_assembly_split_k_tail_matches_numpy


def test_bad_arguments_are_refused():
    out = (C.c_int * 6)()
    L = _lib.load()
    assert L.pq_debug_syrk_plan(0, 16, 1, C.byref(out)) < 0
    assert L.pq_debug_syrk_plan(128, -1, 1, C.byref(out)) < 0
    assert L.pq_debug_syrk_plan(128, 16, 1, None) < 0
    assert L.pq_debug_syrk_plan(32767 * 128 + 1, 16, 1, C.byref(out)) < 0  # (the tile count would leave an int from about 8 million rows on)
    assert L.pq_debug_syrk_plan(32767 * 128, 16, 1, C.byref(out)) == 0 and tuple(out)[:2] == (32767, 32767 * 32768 // 2)
