"""The interior-point loop (piqp_amd/csrc/device_ipm.hip; the host loop of csrc/solver.cpp) against the CPU oracle at every launch shape of tests/ipm_shapes.py.

(a) Behind the reference-order engines (PIQP_AMD_SPARSE_LDLT=exact; dense kkt_solver = 19) a whole solve is the oracle's sequence of IEEE operations, so status,
    count, the whole per-iteration table, ALL TEN result vectors and every info field the oracle has are held BITWISE -- which makes one cheap solve a test of each
    elementwise kernel, each max / min / amax slot of the two-stage reduction, k_seq_dots and k_finish at that grid.  Tolerance: none.
(b) Behind the default engines (multifrontal sparse; dense Cholesky / LDL') mu, sigma and the objective dots come from the tree sums (block_reduce_store into
    k_final_reduce with OP_SUM), which (a) never sees.  They are held to the oracle within tolerances measured on the reference alone: the oracle solves the shape
    as generated and with variables and rows reversed (every summation and elimination order changes); per trace column (relative, rows with oracle mu >= 1e-6) and
    per result vector (absolute) the tolerance is the larger of 30 x that reorder difference and rtol 1e-6 (tests/test_solver_gpu.py::
    test_iteration_parity_random_qp).  On primal_obj, dual_obj and mu it must stay below 1 / (2 N), N the terms of the longest sum, or one lost term would pass.

Reorder differences of the oracle (tests/test_ipm_shapes.py prints them), trace columns primal_obj dual_obj gap primal_res dual_res rho delta mu steps | results:
  L1  1.9e-14 1.4e-12 2.0e-08 2.9e-08 7.3e-11 5.9e-15 5.2e-14 3.0e-12 6.0e-13 | x 5.4e-12  s 5.4e-12  y 4.0e-06  z 3.1e-05   1/(2N) = 8.7e-06 (mu)
  L2  3.8e-14 5.5e-14 5.0e-09 5.5e-08 9.9e-10 9.1e-14 1.7e-13 2.2e-10 2.7e-11 | x 2.4e-14  s 2.4e-14  y 1.6e-06  z 5.0e-06   1/(2N) = 1.9e-06 (mu)
  L3  1.4e-14 1.9e-12 2.6e-10 2.3e-09 4.9e-08 5.7e-13 2.8e-10 2.8e-10 3.1e-11 | x 2.2e-16  s 5.0e-14  y 5.8e-05  z 2.0e-04   1/(2N) = 2.0e-05 (mu)
  L4  1.0e-14 1.2e-10 3.2e-09 2.1e-08 2.0e-07 5.1e-14 5.1e-14 6.5e-10 1.8e-10 | x 2.2e-16  s 1.9e-14  y 1.0e-04  z 5.6e-04   1/(2N) = 2.5e-06 (mu)
so every trace tolerance is the 1e-6 floor except dual_res on L3 / L4 (1.5e-6, 6.0e-6) -- below 1 / (2 N) on the three sum-carrying columns everywhere -- and the
dual vectors are loose (weakly active bounds leave them poorly determined; up to 1.7e-2 absolute on z of L4): (a) is what holds k_finish.  (The figures are
those of one CPU; they move in their last digit with the BLAS that forms A x_sol and G x_sol in the generator.  The tests measure them afresh.)

Device solves on an MI355X: (a) 0.01 s or less on the six small shapes with either loop, L1 0.07 s (host loop 0.06 s), L2 0.38 s, L3 0.13 s, L4 0.98 s, each twice
per case; (b) L1 0.01 s, L2 0.01 s, L3 0.03 s, L4 0.20 s.  The slowest case, L4 of (a), takes 2.5 s with its share of the oracle's solve; the module 11 s."""
import time

import numpy as np
import pytest

import ipm_shapes as S

pytestmark = pytest.mark.gpu

DENSE_EXACT = 19


@pytest.fixture(scope="module")
def problem():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = S.args_of(S.BY_NAME[name])
        return cache[name]
    return get


@pytest.fixture(scope="module")
def oracle(orc, problem):
    """the oracle's solve per (shape, kkt_solver), computed once and left unchanged"""
    cache = {}

    def get(name, kkt_solver=None):
        if (name, kkt_solver) not in cache:
            cache[name, kkt_solver] = S.oracle_solve(orc, problem(name), S.BY_NAME[name].dense, kkt_solver)
        return cache[name, kkt_solver]
    return get


@pytest.fixture(scope="module")
def tolerance(orc, problem, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            shape, ref = S.BY_NAME[name], oracle(name)
            rev = S.unreverse(S.oracle_solve(orc, S.reversed_args(problem(name), shape.dense), shape.dense))
            diff = S.reorder_differences(ref, rev)
            assert diff is not None, "the reordered oracle solve is not comparable (tests/test_ipm_shapes.py)"
            cache[name] = S.tolerances(diff, ref)
        return cache[name]
    return get


def _device_solver(hip, shape, args, kkt_solver):
    sh = hip.DenseSolver() if shape.dense else hip.SparseSolver()
    sh.settings.kkt_solver = kkt_solver
    sh.enable_trace(256)
    assert sh.setup(*args)
    return sh


def _timed_solve(sh, label):
    t0 = time.perf_counter()
    snap = S.snapshot(sh, sh.solve())
    print(f"{label}: device solve {time.perf_counter() - t0:.2f} s, {snap['info']['iter']} iterations")
    return snap


HOST_LOOP = [s.name for s in S.SMALL] + ["L1"]
EXACT_CASES = [(s.name, "device") for s in S.SHAPES] + [(name, "host") for name in HOST_LOOP]


@pytest.mark.parametrize("name,loop", EXACT_CASES, ids=[f"{n}-{l}" for n, l in EXACT_CASES])
def test_reference_order_solve_is_bitwise_the_oracle(hip, orc, problem, oracle, name, loop, monkeypatch):
    """(a): status, count, the whole trace, all ten result vectors and every shared info field, bit for bit; then the same again from a second solve() of the same
    handle (state left in the resident vectors would show)"""
    shape = S.BY_NAME[name]
    monkeypatch.setenv("PIQP_AMD_SPARSE_LDLT", "exact")
    if loop == "host":
        monkeypatch.setenv("PIQP_AMD_HOST_IPM", "1")
    ref = oracle(name)
    assert ref["info"]["status"] == orc.SOLVED
    sh = _device_solver(hip, shape, problem(name), DENSE_EXACT if shape.dense else hip.SPARSE_LDLT)
    for run in ("first", "second"):
        sh.enable_trace(256)
        got = _timed_solve(sh, f"{name} {loop} loop, {run} solve")
        bad = S.first_difference(got, ref)
        assert bad is None, f"{name}, {loop} loop, {run} solve: {bad}"


TREE_CASES = [("L1", "multifrontal"), ("L2", "multifrontal"), ("L3", 0), ("L3", 16), ("L4", 0), ("L4", 16)]


@pytest.mark.parametrize("name,engine", TREE_CASES, ids=[f"{n}-{e}" for n, e in TREE_CASES])
def test_tree_sums_behind_the_default_engines(hip, orc, problem, oracle, tolerance, name, engine, monkeypatch):
    """(b): the device loop behind the default engines against the oracle, within the reference's own reorder differences (module docstring)"""
    shape = S.BY_NAME[name]
    args = problem(name)
    if shape.dense:
        ref = oracle(name, engine)
        sh = _device_solver(hip, shape, args, engine)
    else:
        monkeypatch.setenv("PIQP_AMD_SPARSE_LDLT", engine)
        ref = oracle(name)
        sh = _device_solver(hip, shape, args, hip.SPARSE_LDLT)
    tol = tolerance(name)
    N = S.summed_terms(shape, args)
    for col in ("primal_obj", "dual_obj", "mu"):
        assert tol["trace"][S.TRACE_COLS.index(col)] < 1.0 / (2 * N[col]), (col, tol["trace"][S.TRACE_COLS.index(col)], N[col])
    got = _timed_solve(sh, f"{name} {engine}")
    assert got["info"]["status"] == ref["info"]["status"] == orc.SOLVED
    assert got["info"]["iter"] == ref["info"]["iter"], (got["info"]["iter"], ref["info"]["iter"])
    assert got["trace"].shape == ref["trace"].shape
    rows = S.kept_rows(ref["trace"])
    assert rows.size >= 5
    tg, tr = got["trace"][rows], ref["trace"][rows]
    assert np.array_equal(tg == 0.0, tr == 0.0)
    err = np.abs(tg - tr) / np.where(tr == 0.0, 1.0, np.abs(tr))  # (exact zeros, the steps of row 0, are equal by the line above)
    print(f"{name} {engine}: trace, largest relative difference per column " + " ".join(f"{c}={e:.1e}" for c, e in zip(S.TRACE_COLS[1:], err.max(axis=0)[1:])))
    for c, col in enumerate(S.TRACE_COLS):
        r = int(np.argmax(err[:, c] / tol["trace"][c]))
        assert err[r, c] <= tol["trace"][c], f"{name} {engine}: trace row {rows[r]} column {col}: {tg[r, c]!r} vs {tr[r, c]!r}, relative {err[r, c]:.3e} > {tol['trace'][c]:.3e}"
    worst = {}
    for k in S.VARS:
        g, r = got["result"][k], ref["result"][k]
        sg, sr = S.special(g), S.special(r)
        bad = np.nonzero((sg != sr) | (sr & (g != r)))[0]
        assert bad.size == 0, f"{name} {engine}: result.{k}[{bad[0]}]: {g[bad[0]]!r} vs {r[bad[0]]!r}: the exact 0.0 / 1e30 entries differ ({bad.size})"
        d = np.where(sr, 0.0, np.abs(g - r))
        i = int(np.argmax(d)) if d.size else 0
        worst[k] = float(d[i]) if d.size else 0.0
        assert worst[k] <= tol["result"][k], f"{name} {engine}: result.{k}[{i}]: {g[i]!r} vs {r[i]!r}, difference {worst[k]:.3e} > {tol['result'][k]:.3e}"
    print(f"{name} {engine}: results, largest difference " + " ".join(f"{k}={v:.1e}/{tol['result'][k]:.1e}" for k, v in worst.items()))
