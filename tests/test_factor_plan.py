"""CPU test of the facts beside every shape of tests/factor_shapes.py: which factorisation path the size takes (launch_factor_panels, csrc/dense_kkt.cpp), what
the ticket list of the persistent launch holds at its T (chol_build_tasks through the host-only pq_debug_chol_plan), and which form and how many helpers the sweeps
run with (DenseKKT::alloc and launch_trsv), each restated below from the source.  tests/test_dense_factor_componentwise_gpu.py holds the arithmetic at these
shapes; this file pins that each shape really reaches the branch it is listed for, and that the size one panel smaller does not."""
import ctypes as C

import numpy as np
import pytest

from factor_shapes import FACTOR_SHAPES, FIRST_WITH, GRID, SWEEP_SHAPES, SWEEP_VARIANTS, UPDATE_SHAPES, by_n, shape_id
from piqp_amd import _lib

NB = 128


def plan(T):
    L = _lib.load()
    n = L.pq_debug_chol_plan(T, None, 0)
    assert n > 0
    out = np.zeros((n, 5), dtype=np.int32)
    assert L.pq_debug_chol_plan(T, out.ctypes.data_as(C.c_void_p), n) == n
    return out


def plan_facts(T):
    """(kind7, parities, whole) of the ticket list at T: the most kind-7 visits on one tile, the parities of the columns visited, any whole panel tile.  Also
    checks that every visit spans two panels (chol_far = 2) and that the visits of a tile are disjoint and ascending."""
    tasks = plan(T)
    visits = {}
    for kind, rnd, a, b, gate in tasks:
        if kind == 7:
            assert gate + 1 - rnd == 2, (T, rnd, gate)
            visits.setdefault((int(a), int(b)), []).append((int(rnd), int(gate) + 1))
    for (i, j), v in visits.items():
        assert all(v[q][1] == v[q + 1][0] for q in range(len(v) - 1)), (T, i, j, v)
        assert v[0][0] == j % 2, (T, i, j, v)  # odd columns: the leading panel is taken singly (an ordinary kind-3 task), the visits start at panel 1
    kind7 = max((len(v) for v in visits.values()), default=0)
    parities = tuple(sorted({j % 2 for _, j in visits}))
    whole = bool(((tasks[:, 0] == 2) & (tasks[:, 3] == -1)).any())
    if whole:
        w = tasks[(tasks[:, 0] == 2) & (tasks[:, 3] == -1)]
        assert (w[:, 2] > 2).all() and (T - w[:, 1] - 1 >= 22).all()  # rows beyond CHOL_FAST_ROWS of rounds with >= 22 trailing tile rows
    return kind7, parities, whole


def sweep_facts(n):
    """(nblk, inverse, H): DenseKKT::alloc sets inv_sweeps_ for 8 <= nblk <= 224; launch_trsv takes H = min(7, 256 / nblk - 1) helpers with the inverses"""
    nblk = -(-n // NB)
    inverse = 8 <= nblk <= 224
    H = min(7, 256 // nblk - 1) if inverse else 0
    return nblk, inverse, H


@pytest.mark.parametrize("shape", GRID, ids=shape_id)
def test_shape_reaches_its_branch(shape):
    n = shape.n
    persistent = n % NB == 0 and 3 <= n // NB <= 1024  # chol_persistent_supported
    assert persistent == shape.persistent, shape.branch
    assert -(-n // NB) == shape.T
    if persistent:
        assert plan_facts(shape.T) == (shape.kind7, shape.parities, shape.whole), shape.branch
    else:
        assert (shape.kind7, shape.parities, shape.whole) == (0, (), False)  # no ticket list on the launch-per-panel path
    assert sweep_facts(n) == (shape.nblk, shape.inverse, shape.H), shape.branch


def test_first_sizes_of_the_ticket_list_branches():
    """T = 9, 11 and 23 are the first with their property: T - 1 lacks it"""
    assert sorted(FIRST_WITH) == [9, 11, 23]
    assert by_n(9 * NB).kind7 == 1 and plan_facts(8)[0] == 0, "kind 7 below T = 9, or none at T = 9"
    k7, par, _ = plan_facts(10)
    s = by_n(11 * NB)
    assert s.kind7 == 2 and s.parities == (0, 1) and not (k7 >= 2 and par == (0, 1)), "T = 10 already has two visits on one tile"
    assert by_n(23 * NB).whole and not plan_facts(22)[2], "whole panel tiles below T = 23"
    # every T below 9 of the table has no kind 7 at all, and T = 3 (the smallest) is accepted by the call
    assert all(plan_facts(T)[0] == 0 for T in range(3, 9))


def test_sweep_thresholds_sit_where_the_table_says():
    """each sweep shape is the first (or, for 896 and 4096, the last) size of its form / helper count"""
    f = sweep_facts
    assert f(896) == (7, False, 0) and f(897) == (8, True, 7)
    assert f(4096)[2] == 7 and f(4097)[2] == 6
    assert f(4608)[2] == 6 and f(4609)[2] == 5
    assert f(5376)[2] == 5 and f(5377)[2] == 4
    assert f(6528)[2] == 4 and f(6529)[2] == 3
    assert f(8192)[2] == 3 and f(8193)[2] == 2  # H <= 2: not covered (tests/factor_shapes.py)
    # one-XCD ticket mode: nblk <= 32 with H = 0 (896 if the probe allows); the local hand-over: H = 7 (897, 4096): the shapes of the variant runs
    assert {n for n, _ in SWEEP_VARIANTS} == {896, 897, 4096}
    assert all(by_n(n).nblk <= 32 for n, _ in SWEEP_VARIANTS)
    assert by_n(896).H == 0 and by_n(897).H == 7 and by_n(4096).H == 7


def test_lists():
    assert [s.n for s in FACTOR_SHAPES] == [1, 16, 17, 127, 128, 129, 255, 256, 257, 383, 384, 385, 512, 1152, 1408, 2944]
    assert [s.n for s in SWEEP_SHAPES] == [127, 129, 896, 897, 4096, 4097, 4609, 5377, 6529]
    assert all(by_n(n).persistent and by_n(n) in FACTOR_SHAPES for n in UPDATE_SHAPES)
