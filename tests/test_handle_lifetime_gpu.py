"""Lifetimes of the handles' streams, events and backends that no other test exercises: a handle destroyed with work pending on its side stream, the launch-order
registry of the reference-order sparse engine across destroyed handles, the batched solver's timing events over repeated solves, and the profiler's event pool.
Every handle type releases what it owns through its members alone (csrc/common.hpp, pq::Stream): streams first, then events, then buffers."""
import numpy as np
import pytest

from qp_gen import dense_strongly_convex_qp, mpc_batch, mpc_chain

pytestmark = pytest.mark.gpu


def _dense_handle(hip, q):
    return hip.DenseKKT(hip.Data(**q))


def _bitwise(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_dense_handle_destroyed_with_an_inverse_pass_pending(hip):
    """n = 1024: eight 128-row blocks, the smallest size with the side stream of the block inverses, its two events and the persistent factorisation.  Handle A factors
    and goes without a solve (the inverse pass is still pending on the side stream); B on the same data factors and solves; a clone of B outlives B and solves to B's bits."""
    n, m = 1024, 16
    q = dense_strongly_convex_qp(n, 0, m, seed=11, exact_shift=False)
    rng = np.random.default_rng(3)
    x_reg, z_reg = rng.uniform(1e-6, 1e-4, n), rng.uniform(1e-3, 1e1, m)
    rhs = (rng.standard_normal(n), np.zeros(0), rng.standard_normal(m))
    a = _dense_handle(hip, q)
    assert a.update_scalings_and_factor(1e-4, x_reg, z_reg)
    del a
    b = _dense_handle(hip, q)
    assert b.update_scalings_and_factor(1e-4, x_reg, z_reg)
    ref = b.solve(*rhs)
    assert all(np.isfinite(v).all() for v in ref)
    c = b.clone()
    del b
    assert _bitwise(c.solve(*rhs), ref)


def test_reference_order_engine_launch_order_across_destroyed_handles(hip):
    """a chain QP of ten KKT rows on the reference-order engine.  A and B factor in that order; B goes as the last entry of the device's launch order; A factors and
    solves again to its first bits; A goes, and a fresh handle factors and solves."""
    chain = mpc_chain(1, 1, 3, seed=5)  # n = 7, p = 3, m = 0
    data = hip.SparseData(*chain)
    n, p = data.n, data.p
    assert n + p == 10
    rng = np.random.default_rng(4)
    x_reg = rng.uniform(1e-6, 1e-4, n)
    rhs = (rng.standard_normal(n), rng.standard_normal(p), np.zeros(0))

    def make():
        k = hip.DenseKKT(data, kkt_solver=hip.SPARSE_LDLT)
        assert k.exact_factor()["perm"].size == n + p  # (the reference-order engine, not the multifrontal one)
        return k

    a, b = make(), make()
    assert a.update_scalings_and_factor(1e-4, x_reg, np.zeros(0))
    first = a.solve(*rhs)
    assert b.update_scalings_and_factor(1e-4, x_reg, np.zeros(0))
    del b
    assert a.update_scalings_and_factor(1e-4, x_reg, np.zeros(0))
    assert _bitwise(a.solve(*rhs), first)
    del a
    c = make()
    assert c.update_scalings_and_factor(1e-4, x_reg, np.zeros(0))
    assert _bitwise(c.solve(*rhs), first)


def test_batch_solver_repeated_solves_create_nothing(hip):
    """the timing events of BatchSparseSolver.solve() live with the handle: three solves, bitwise equal, each timed, and no allocation after the first"""
    B = 4
    mb = mpc_batch(B, T=10, nx=2, nu=2, seed=5)
    bs = hip.BatchSparseSolver()
    assert bs.setup(mb["P_pattern"], mb["P_values"], mb["c"], mb["A_pattern"], mb["A_values"], mb["b"], x_l=mb["x_l"], x_u=mb["x_u"])
    L = hip._lib.load()
    runs, counts = [], []
    for _ in range(3):
        assert bs.solve() == B
        ms, _ = bs.last_kernel_ms()
        assert ms > 0
        runs.append([bs.result(f).copy() for f in ("x", "y", "z_bl", "z_bu", "s_bl", "s_bu")])
        counts.append(L.pq_debug_alloc_count())
    assert _bitwise(runs[1], runs[0]) and _bitwise(runs[2], runs[0])
    assert counts[0] == counts[1] == counts[2]


def test_profiler_event_pool_is_reused(hip):
    """two rounds of factor, solve, get_profile on a dense and a sparse handle: the second round takes its event pairs from the pool the first one filled"""
    q = dense_strongly_convex_qp(256, 8, 16, seed=2)
    rng = np.random.default_rng(6)
    dense = (_dense_handle(hip, q), rng.uniform(1e-6, 1e-4, 256), rng.uniform(1e-3, 1e1, 16), (rng.standard_normal(256), rng.standard_normal(8), rng.standard_normal(16)))
    data = hip.SparseData(*mpc_chain(2, 1, 6, seed=8))
    sparse = (hip.DenseKKT(data, kkt_solver=hip.SPARSE_LDLT), rng.uniform(1e-6, 1e-4, data.n), np.zeros(0), (rng.standard_normal(data.n), rng.standard_normal(data.p), np.zeros(0)))
    for k, x_reg, z_reg, rhs in (dense, sparse):
        k.set_profiling(True)
        for _ in range(2):
            assert k.update_scalings_and_factor(1e-4, x_reg, z_reg)
            k.solve(*rhs)
            for stage in (1, 2):
                ms, count = k.get_profile(stage)
                assert count == 1 and ms > 0, (stage, ms, count)
