"""CPU test of the inputs of tests/test_ipm_loop_gpu.py: the oracle alone, once per shape of tests/ipm_shapes.py, asserting that the generated problems can carry
what the GPU test concludes from them -- the counts sit where the launch-shape edges are, the planted maxima are the maxima, the solve is long enough, a second
solve of one handle repeats the first, and the final unscale / expand has every kind of entry to get wrong."""
import numpy as np
import pytest

import ipm_shapes as S


@pytest.fixture(scope="module")
def solved(orc):
    cache = {}

    def get(name):
        if name not in cache:
            shape = S.BY_NAME[name]
            args = S.args_of(shape)
            cache[name] = (shape, args) + S.oracle_solve(orc, args, shape.dense, twice=True)
        return cache[name]
    return get


def test_every_count_lands_on_or_beside_every_edge():
    """the five index spaces hit the edges independently: each of 0, 1, 64, 256, 16 384 and 131 072 is reached (on it or one beside it) by some count, each of n, m,
    nxl and nxu is at or above, and somewhere at most 1 below, 64, 256, 16 384 and 131 072 + 1 (p only up to 256: the equality rows share every kernel with m)"""
    counts = {f: [getattr(s, f) for s in S.SHAPES] for f in ("n", "p", "m", "nxl", "nxu")}
    every = [c for v in counts.values() for c in v]
    for edge in (0, 1, 64, 256, 16384, 131072):
        assert any(abs(c - edge) <= 1 for c in every), edge
    for f in ("n", "m", "nxl", "nxu"):
        for edge in (64, 256):
            assert any(abs(c - edge) <= 1 for c in counts[f]), (f, edge)
    assert {63, 64, 65} <= set(counts["n"]) and {255, 256, 257} <= set(counts["n"]) and {63, 64, 65} <= set(counts["p"])
    # the lengths of the left-to-right dot products (k_seq_dots: 64 products at a time) are n, p, m, nxl and nxu
    assert {0, 1, 63, 64, 65} <= set(counts["m"]) | set(counts["nxl"]) | set(counts["nxu"])
    for edge in (16384, 131072):
        for f in ("n", "m", "nxl", "nxu"):
            assert any(c > edge for c in counts[f]), (f, edge)
        assert any(c == edge + 1 for c in every), edge
    assert [s.name for s in S.SHAPES if max(s.n, s.p, s.m) > 64 * 256] == ["L1", "L2", "L3", "L4"]  # more than 64 blocks
    assert [s.name for s in S.SHAPES if max(s.n, s.p, s.m) > 512 * 256] == ["L2", "L4"]             # the grid-stride loops wrap


@pytest.mark.parametrize("name", [s.name for s in S.SHAPES])
def test_generated_problem_has_the_stated_structure(name):
    shape = S.BY_NAME[name]
    P, c, A, b, G, h_l, h_u, x_l, x_u = S.args_of(shape)
    n, p, m = shape.n, shape.p, shape.m
    assert P.shape == (n, n) and c.shape == (n,)
    assert (A is None and b is None) if p == 0 else (A.shape == (p, n) and b.shape == (p,))
    assert (G is None and h_l is None and h_u is None) if m == 0 else (G.shape == (m, n) and h_l.shape == h_u.shape == (m,))
    # exactly nxl / nxu bounded variables, the last variable among them
    assert int(np.isfinite(x_l).sum()) == shape.nxl and int(np.isfinite(x_u).sum()) == shape.nxu
    assert np.isfinite(x_l[-1]) == (shape.nxl > 0) and np.isfinite(x_u[-1]) == (shape.nxu > 0)
    assert (x_l <= x_u).all()
    if m:
        kind = np.isfinite(h_l) * 1 + np.isfinite(h_u) * 2
        assert kind[:4].tolist() == [0, 1, 2, 3][:min(4, m)]
        assert set(kind.tolist()) == {0, 1, 2, 3}
        assert kind[-1] == 3
        assert (h_l <= h_u).all()
    if not shape.dense:
        import scipy.sparse as sp
        assert (P != sp.diags(P.diagonal())).nnz == 0 and P.diagonal().min() >= 0.5 and P.diagonal().max() <= 2.0
        for M, w in ((A, 3), (G, 2)):
            if M is not None:
                R = sp.csr_matrix(M)
                assert (np.diff(R.indptr) == w).all()
                assert R.indices[R.indptr[-2]:].tolist() == list(range(n - w, n))  # the last row touches the last variables
    # the planted elements are the strict maxima of their vectors, in the last place
    assert c[-1] == 40.0 and np.abs(c[:-1]).max() < 40.0
    if p > 1:
        assert np.abs(b[:-1]).max() < abs(b[-1])
    if m > 1:
        fin = lambda v: np.where(np.isfinite(v), np.abs(v), 0.0)
        hm = np.maximum(fin(h_l), fin(h_u))
        assert hm[:-1].max() < h_u[-1]  # (positive: the reference takes a signed maximum over the general rows)


@pytest.mark.parametrize("name", [s.name for s in S.SHAPES])
def test_oracle_solve_can_carry_the_gpu_checks(solved, orc, name):
    shape, args, first, second = solved(name)
    P, c, A, b, G, h_l, h_u, x_l, x_u = args
    info, trace, res = first["info"], first["trace"], first["result"]
    assert info["status"] == orc.SOLVED
    assert trace.shape[0] == info["iter"] + 1
    has_ineq = shape.m + shape.nxl + shape.nxu > 0
    assert has_ineq
    assert S.kept_rows(trace).size >= 5, trace[:, 8]
    # the norms behind the relative residuals are at least the planted elements (they ARE those elements' up to the rounding of the scaling, unless an activity
    # term is larger still): dropping the last element of c, b or h from its amax slot changes dual_res_rel / primal_res_rel
    dual_rel_norm = info["dual_res"] / info["dual_res_rel"]
    assert dual_rel_norm >= 0.99 * abs(c[-1]), (dual_rel_norm, c[-1])
    planted = 0.0
    if shape.p:
        planted = max(planted, abs(b[-1]))
    if shape.m:
        assert h_u[-1] > 0
        planted = max(planted, h_u[-1])  # (the general rows enter through a signed maximum: update_residuals_nr, solver.hpp:960-1105)
    if planted:
        primal_rel_norm = info["primal_res"] / info["primal_res_rel"]
        assert primal_rel_norm >= 0.99 * planted, (primal_rel_norm, planted)
    # a second solve() of the same handle is bitwise the first
    assert S.first_difference(second, first) is None, S.first_difference(second, first)
    # k_finish has something to get wrong: absent bounds (z = 0, s = 1e30) beside present ones (finite s, nonzero z), wherever the counts allow.  (A general row
    # without any finite bound is kept as the zero row with bounds -1, 1 -- data.hpp disable_inf_constraints -- so both of its sides count as present.)
    free_row = None if shape.m == 0 else ~np.isfinite(h_l) & ~np.isfinite(h_u)
    for s_name, z_name, bound, count, size in (("s_l", "z_l", h_l, None, shape.m), ("s_u", "z_u", h_u, None, shape.m),
                                               ("s_bl", "z_bl", x_l, shape.nxl, shape.n), ("s_bu", "z_bu", x_u, shape.nxu, shape.n)):
        if size == 0:
            continue
        s, z = res[s_name], res[z_name]
        present = np.isfinite(bound) | free_row if count is None else np.isfinite(bound)
        assert np.array_equal(s == S.BIG, ~present), s_name   # (no z of a present bound has come out as an exact zero: the 1e30 entries are the absent bounds)
        assert np.array_equal(z == 0.0, ~present), z_name
        assert np.isfinite(s).all() and (s[present] < 1e29).all() and (s[present] >= 0).all()
        count = int(present.sum()) if count is None else count
        if 0 < count < size:
            assert (s == S.BIG).any() and (s != S.BIG).any(), s_name
        if count:
            assert (z[present] != 0).all(), z_name
        if count >= 8:
            assert np.abs(z[present]).max() > 1e-3, z_name  # some bound is active
    assert shape.nxl + shape.nxu == 0 or (np.count_nonzero(res["z_bl"]) + np.count_nonzero(res["z_bu"]) > 0)


@pytest.mark.parametrize("name", [s.name for s in S.LARGE])
def test_reordered_oracle_solve_is_comparable(solved, orc, name):
    """the reference perturbation behind the tolerances of the tree-sum leg: the same problem with variables and rows reversed takes the same number of iterations,
    keeps every 0.0 / 1e30 in place, and leaves tolerances on the sum-carrying columns below 1 / (2 N)"""
    shape, args, first, _ = solved(name)
    rev = S.unreverse(S.oracle_solve(orc, S.reversed_args(args, shape.dense), shape.dense))
    diff = S.reorder_differences(first, rev)
    assert diff is not None, (first["info"]["iter"], rev["info"]["iter"])
    tol = S.tolerances(diff, first)
    print(name, "trace", " ".join(f"{c}={d:.1e}" for c, d in zip(S.TRACE_COLS[1:], diff["trace"][1:])))
    print(name, "result", " ".join(f"{k}={d:.1e}" for k, d in diff["result"].items()))
    N = S.summed_terms(shape, args)
    for col in ("primal_obj", "dual_obj", "mu"):
        assert tol["trace"][S.TRACE_COLS.index(col)] < 1.0 / (2 * N[col]), (col, tol["trace"][S.TRACE_COLS.index(col)], N[col])
