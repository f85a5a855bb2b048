"""CPU test of the inputs of tests/test_multistage_branches_gpu.py: the oracle and NumPy alone, once per row of tests/multistage_shapes.py, asserting that the generated
problems can carry what the GPU test concludes from them -- each row reaches the launch branch it is pinned to, the table covers every branch, the reference is
accurate far below the tolerance it is used for, and the `well` regime is as well conditioned as the margin of the GPU test assumes."""
import numpy as np
import pytest

import multistage_shapes as S

NAMES = [s.name for s in S.SHAPES]


@pytest.fixture(scope="module")
def built(orc):
    cache = {}

    def get(name):
        if name not in cache:
            shape = S.BY_NAME[name]
            args = S.args_of(shape)
            od = orc.Data.sparse(*args)
            cache[name] = (shape, args, od, orc.KKT(od, kind="multistage").block_info())
        return cache[name]
    return get


def test_table_covers_every_branch():
    plans = [s.plan for s in S.SHAPES]
    assert {(pl["factor_in_lds"], pl["li_in_lds"], pl["solve_in_lds"]) for pl in plans} == S.CONFIGURATIONS
    chunks = {pl["asm_chunks"] for pl in plans}
    assert 1 in chunks and max(chunks) > 1
    # more than one chunk on both sides of the factorisation's LDS / HBM switch
    assert any(pl["asm_chunks"] > 1 and pl["factor_in_lds"] for pl in plans) and any(pl["asm_chunks"] > 1 and not pl["factor_in_lds"] for pl in plans)
    # the inverse's LDS / HBM switch from both sides: 142^2 <= 20352 < 143^2
    assert {142, 143} <= {pl["max_w"] for pl in plans}
    assert S.BY_NAME["hbm-li142-hbm"].plan["li_in_lds"] == 1 and S.BY_NAME["hbm-hbm143-hbm"].plan["li_in_lds"] == 0
    # m = 0, p = 0 and arrow width 0 on a shape whose factorisation runs in HBM
    for pick in (lambda s: s.dims[2] == 0, lambda s: s.dims[1] == 0, lambda s: s.arrow == 0):
        assert any(pick(s) and not s.plan["factor_in_lds"] for s in S.SHAPES)
    # ascending novelty: the all-LDS rows first, the all-HBM row last
    order = [pl["factor_in_lds"] + pl["li_in_lds"] + pl["solve_in_lds"] for pl in plans]
    assert order == sorted(order, reverse=True) and S.SHAPES[-1].name == S.ALL_HBM
    assert all(max(s.dims) <= 400 for s in S.SHAPES)


def test_plan_of_restates_the_budget():
    """plan_of at hand-made structures on both sides of each threshold (159 KiB = 20352 doubles, 4096 entries per chunk)"""
    one = lambda w, off, arrow: S.plan_of([[0, w, off], [w, off, 0], [w + off, arrow, 0]])
    assert S.LDS_DOUBLES == 20352
    pl = one(64, 0, 0)
    assert (pl["max_h"], pl["max_w"], pl["asm_chunks"], pl["factor_in_lds"], pl["factor_lds_bytes"]) == (64, 64, 1, 1, 8 * 2 * 4096)
    assert one(65, 0, 0)["asm_chunks"] == 2
    assert one(100, 0, 0)["factor_in_lds"] == 1 and one(101, 0, 0)["factor_in_lds"] == 0  # 2 w^2: 20000 / 20402
    assert one(100, 0, 0)["solve_in_lds"] == 1 and one(101, 0, 0)["solve_in_lds"] == 0    # 2 w + 2 w^2: 20200 / 20604
    assert one(142, 0, 0)["li_in_lds"] == 1 and one(142, 0, 0)["factor_lds_bytes"] == 8 * 142 * 142
    assert one(143, 0, 0)["li_in_lds"] == 0 and one(143, 0, 0)["factor_lds_bytes"] == 0
    pl = one(60, 30, 10)  # h = 100, u = 40: 10000 + 1600 + 3600; the solve holds 2 * 100 + 100 * 60 + 3600
    assert (pl["max_h"], pl["factor_in_lds"], pl["solve_in_lds"], pl["factor_lds_bytes"]) == (100, 1, 1, 8 * 15200)


@pytest.mark.parametrize("name", NAMES)
def test_shape_reaches_its_branch(built, name):
    shape, args, od, bi = built(name)
    assert (od.n, od.p, od.m) == shape.dims
    assert int(bi[-1, 1]) == shape.arrow
    assert S.plan_of(bi) == shape.plan
    assert S.stages_of(bi) < 16  # below the cost model: the chain engine whatever the model says
    # the fronts are dense where the kernels index them: every stage holds dense dynamics blocks (a sparse L would hide a wrong index)
    Pf, A, G = S.dense3(args)
    delta, x_reg, z_reg = S.scalings("well", od.n, od.m)
    L = np.linalg.cholesky(S.condensed_matrix(Pf, A, G, x_reg, delta, z_reg))
    for b, (start, w, off) in enumerate(bi[:-1]):
        if b < len(bi) - 2 and off > 0:
            assert np.count_nonzero(L[start + w:start + w + off, start:start + w]) == off * w, b
        assert np.count_nonzero(np.tril(L[start:start + w, start:start + w])) == w * (w + 1) // 2, b


@pytest.mark.parametrize("name", NAMES)
def test_reference_and_conditioning(built, name):
    shape, args, od, bi = built(name)
    n, p, m = shape.dims
    Pf, A, G = S.dense3(args)
    R = np.stack([np.concatenate(r) for r in S.right_hand_sides(n, p, m)], axis=1)
    for regime in S.REGIMES:
        delta, x_reg, z_reg = S.scalings(regime, n, m)
        sol, res = S.reference_solve(Pf, A, G, x_reg, delta, z_reg, R)
        rel = np.asarray(res / np.abs(R).max(axis=0), dtype=np.float64)
        kappa = max(S.block_conditions(S.condensed_matrix(Pf, A, G, x_reg, delta, z_reg), bi))
        print(f"{name} {regime}: reference residual / |rhs| = {rel.max():.2e}, largest kappa_2 of a diagonal block of L = {kappa:.1f}")
        assert np.isfinite(sol).all()
        assert (rel <= 1e-16).all(), rel
        if regime == "well":
            assert kappa <= 100.0, kappa
