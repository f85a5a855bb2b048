"""CPU test of the persistent dense factorisation's ticket list (csrc/dense_kernels.hip: chol_build_tasks), fetched through the host-only
C-ABI call pq_debug_chol_plan.  The launch is deadlock-free under ANY number of resident workgroups because a workgroup inside a task only ever waits for results
of EARLIER tickets; this test replays the list in ticket order with every earlier task complete and checks, for each task, exactly the conditions the kernel
waits for (k_chol_persistent) -- plus coverage: every tile receives the updates of panels 0 .. j-1 once, in order (the factorisation of
Eigen::LLT / dense/ldlt_no_pivot.hpp:313-354 as a task graph)."""
import ctypes as C

import numpy as np
import pytest

from piqp_amd import _lib

FAST_ROWS = 2


def split(T, k):
    return 1 if T - k - 1 >= 22 else 2


def split_row(T, k, ti):
    return 2 if ti <= FAST_ROWS else split(T, k)


def plan(T):
    L = _lib.load()
    n = L.pq_debug_chol_plan(T, None, 0)
    assert n > 0
    out = np.zeros((n, 5), dtype=np.int32)
    assert L.pq_debug_chol_plan(T, out.ctypes.data_as(C.c_void_p), n) == n
    return out


@pytest.mark.parametrize("T", [3, 5, 8, 16, 32, 40])
def test_every_task_waits_for_earlier_tickets_only(T):
    tasks = plan(T)
    tver = np.zeros((T, T), dtype=int)  # updates received
    lready = np.zeros((T + 1, T), dtype=int)
    pdone = np.zeros(T, dtype=int)
    owner_seen = np.zeros(T, dtype=bool)
    dhalf = np.zeros(T, dtype=int)
    panel_final = np.zeros((T, T), dtype=bool)

    def rows_ready(k, i):
        return k == 0 or lready[k, i] == split_row(T, k - 1, i - k)

    def rounds_complete():
        p = 0
        while p + 1 < T and pdone[p] == sum(split_row(T, p, ti) for ti in range(1, T - p - 1)):
            p += 1
        return p

    for pos, (kind, rnd, a, b, gate) in enumerate(tasks):
        assert gate <= rounds_complete(), (pos, kind, rnd, a, b, gate)  # the gate only ever refers to rounds finished by earlier tickets
        if kind == 7:
            i, j, klo, khi = a, b, rnd, gate + 1
            assert 1 <= j <= i < T and 0 <= klo < khi <= j - 3
            assert tver[i, j] == klo, (pos, i, j, klo, tver[i, j])
            assert rows_ready(khi - 1, i) and rows_ready(khi - 1, j), (pos, i, j, khi)
            tver[i, j] = khi
            continue
        k = rnd
        d = k + 1
        if kind in (0, 1):
            assert tver[d, d] == k, (pos, kind, k, tver[d, d])
            assert rows_ready(k, d)
            if kind == 1:
                if k >= 2:
                    assert pdone[k - 2] == sum(split_row(T, k - 2, ti) for ti in range(1, T - (k - 2) - 1))
                owner_seen[k] = True
            continue
        ti = a
        tj = 0 if kind == 2 else b
        i, j = k + 1 + ti, k + 1 + tj
        assert tver[i, j] == k, (pos, kind, k, i, j, tver[i, j])
        assert rows_ready(k, i) and rows_ready(k, j), (pos, kind, k, i, j)
        if kind == 2:
            assert owner_seen[k], (pos, k)  # the panel rows follow the factorisation of the diagonal block
            lready[k + 1, i] += 1
            pdone[k] += 1
            if lready[k + 1, i] == split_row(T, k, ti):
                panel_final[i, j] = True
        elif kind in (4, 5):
            dhalf[k] += 1
            if dhalf[k] == 2:
                tver[i, j] = k + 1
        else:
            tver[i, j] = k + 1
    # coverage
    for j in range(1, T):
        for i in range(j, T):
            assert tver[i, j] == j - 1, (i, j, tver[i, j])  # (the last update, k = j - 1, is the crew's on the diagonal tile and the panel task's below it)
            if i > j:
                assert panel_final[i, j], (i, j)
    assert owner_seen[: T - 1].all()
