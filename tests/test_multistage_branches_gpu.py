"""The chain engine of the `sparse_multistage` backend (csrc/multistage_kkt.hip, csrc/multistage_device.hpp) at every branch of MultistageKKT::plan_lds(): factor in LDS /
in place in HBM, inverse staged in LDS / written to HBM, solve in LDS / from HBM, one / several assembly and Gram chunks -- the rows of tests/multistage_shapes.py, which
tests/test_multistage_shapes.py pins to their branches on the CPU.  The cases run in the table's order, the all-LDS rows first and the all-HBM row last.

Reference: the full 3 x 3 KKT system solved in fp64 and refined with longdouble residuals (multistage_shapes.reference_solve; its own residual is below
1e-16 |rhs|, asserted on the CPU).  Per field v of (x, y, z) and per right-hand side, err(v) = max |v - v_ref| / max |v_ref|, and the device is held to
    err_dev <= MARGIN * max(err_oracle, 8 * 2^-53),   MARGIN = 8,
with err_oracle the CPU oracle's error on the same input, computed at run time: the oracle runs the reference's algorithm (the same block recurrence, substitution
with L instead of multiplication by an explicit inverse), so its error is what this algorithm costs on this input, and the margin is what another summation order and
the explicit inverses of the w x w diagonal blocks may add (their condition number is capped at 100 in the `well` regime, on the CPU).  No figure of the device enters
a tolerance.  For orientation, err_oracle is 0.8e-15 .. 4e-15 in the `well` regime and 0.7e-12 .. 2.6e-11 in the `ipm` regime.

Largest err_dev / max(err_oracle, 8 * 2^-53) observed on an MI355X, per row of the table (well / ipm; each test prints its own):
    lds-lds-1chunk 1.03 / 1.30    lds-lds 1.60 / 1.82          hbm-li-lds 2.62 / 1.12      hbm-li-lds-m0 1.14 / 1.23     hbm-li-lds-p0 2.25 / 2.93
    hbm-li-hbm-arrow0 1.08 / 1.59 hbm-li-hbm 2.81 / 2.90       hbm-li142-hbm 3.35 / 2.39   hbm-hbm143-hbm 1.32 / 4.55    hbm-hbm-hbm 1.50 / 2.25
and 4.79 in the update_data check (hbm-li-lds, field z, where the oracle's own error happens to be 6e-16); no branch needs more than the margin of 8.
"""
import numpy as np
import pytest

import multistage_shapes as S
from qp_gen import random_vars

pytestmark = pytest.mark.gpu

MARGIN = 8.0
FLOOR = 8.0 * S.U
FIELDS = ("x", "y", "z")


class Case:
    """one row of the table with everything the CPU contributes, computed once: the oracle's block structure, per regime the reference solutions and the oracle's errors"""

    def __init__(self, orc, shape):
        self.orc, self.shape = orc, shape
        self.args = S.args_of(shape)
        self.n, self.p, self.m = shape.dims
        self.rhs = S.right_hand_sides(self.n, self.p, self.m)
        self.od = orc.Data.sparse(*self.args)
        self.ko = orc.KKT(self.od, kind="multistage")
        self.bi = self.ko.block_info()
        self._regime = {}
        self._updated = None

    def _reference(self, args, od, ko, delta, x_reg, z_reg, rhs):
        """(reference solutions split per right-hand side, tolerance per right-hand side and field, the oracle's errors)"""
        Pf, A, G = S.dense3(args)
        sol, _ = S.reference_solve(Pf, A, G, x_reg, delta, z_reg, np.stack([np.concatenate(r) for r in rhs], axis=1))
        assert ko.update_scalings_and_factor(delta, x_reg, z_reg)
        refs = [S.split(sol[:, q], self.n, self.p, self.m) for q in range(len(rhs))]
        err_orc = [S.field_errors(ko.solve(*r), ref) for r, ref in zip(rhs, refs)]
        return refs, [[MARGIN * max(e, FLOOR) for e in row] for row in err_orc], err_orc

    def regime(self, name):
        if name not in self._regime:
            delta, x_reg, z_reg = S.scalings(name, self.n, self.m)
            self._regime[name] = (delta, x_reg, z_reg) + self._reference(self.args, self.od, self.ko, delta, x_reg, z_reg, self.rhs)
        return self._regime[name]

    def updated(self):
        """new values on the same patterns, with the reference and the oracle's error for the first right-hand side in the `well` regime"""
        if self._updated is None:
            args2 = S.new_values(self.args)
            od2 = self.orc.Data.sparse(*args2)
            delta, x_reg, z_reg = S.scalings("well", self.n, self.m)
            self._updated = (args2,) + self._reference(args2, od2, self.orc.KKT(od2, kind="multistage"), delta, x_reg, z_reg, self.rhs[:1])
        return self._updated


_CASES = {}


def _case(orc, name):
    if name not in _CASES:
        _CASES[name] = Case(orc, S.BY_NAME[name])
    return _CASES[name]


@pytest.fixture(scope="module", params=[s.name for s in S.SHAPES])
def case(request, orc):
    """module scope: pytest runs every test of one row before the next row, in the table's order"""
    return _case(orc, request.param)


@pytest.fixture(autouse=True)
def _engine_by_structure(monkeypatch):
    monkeypatch.delenv("PIQP_AMD_MULTISTAGE", raising=False)


def _handle(hip, args):
    return hip.SparseKKT(hip.SparseData(*args), kkt_solver=hip.SPARSE_MULTISTAGE)


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def _check(label, sol, ref, tol, err_orc):
    """asserts err_dev <= tol per field; returns the largest err_dev / max(err_oracle, FLOOR)"""
    assert all(np.isfinite(v).all() for v in sol), label
    err = S.field_errors(sol, ref)
    ratios = [e / max(o, FLOOR) for e, o in zip(err, err_orc)]
    print(f"  {label}: " + "  ".join(f"{f}: dev {e:.2e} oracle {o:.2e} ratio {r:.2f}" for f, e, o, r in zip(FIELDS, err, err_orc, ratios)))
    for f, e, t in zip(FIELDS, err, tol):
        assert e <= t, f"{label}, field {f}: err_dev {e:.3e} > {t:.3e} = {MARGIN:g} x max(err_oracle, 8 u)"
    return max(ratios)


def test_plan(case, hip):
    """the library plans what the table pins and what plan_of derives from the oracle's structure, on the chain engine"""
    k = _handle(hip, case.args)
    plan = k.multistage_plan()
    assert plan["engine"] == 0
    assert {key: plan[key] for key in S.PLAN_KEYS} == case.shape.plan == S.plan_of(case.bi)
    assert np.array_equal(k.block_info(), case.bi)


@pytest.mark.parametrize("regime", S.REGIMES)
def test_accuracy_and_determinism(case, hip, regime):
    delta, x_reg, z_reg, refs, tols, err_orc = case.regime(regime)
    k = _handle(hip, case.args)
    assert k.update_scalings_and_factor(delta, x_reg, z_reg)
    sols = [k.solve(*r) for r in case.rhs + case.rhs[:1]]
    worst = max(_check(f"{case.shape.name} {regime} rhs {q}", sols[q], refs[q], tols[q], err_orc[q]) for q in range(4))
    print(f"RATIO {case.shape.name} {regime} {worst:.2f}")
    assert _same(sols[4], sols[0]), "the fifth solve repeats the first right-hand side and differs"
    assert k.update_scalings_and_factor(delta, x_reg, z_reg)
    assert _same(k.solve(*case.rhs[0]), sols[0]), "a second factorisation of the same inputs gives another solution"


def test_ipm_condensed_residual(case, hip):
    """the project's own criterion through KKTSystem, at an interior-point state: condensed residual <= 1e-10 |rhs|"""
    n, p, m = case.shape.dims
    ks = hip.KKTSystem(hip.SparseData(*case.args), hip.default_settings(kkt_solver=hip.SPARSE_MULTISTAGE))
    rng = np.random.default_rng([n, 13])
    state = random_vars(n, p, m, rng, positive=True)
    assert ks.update_scalings_and_factor(False, 1e-6, 1e-4, state)
    ok, _ = ks.solve(random_vars(n, p, m, rng))
    assert ok
    res, nrm = ks.condensed_residual()
    print(f"  {case.shape.name}: condensed residual / |rhs| = {res / nrm:.2e}")
    assert res <= 1e-10 * nrm, (res, nrm)


def test_update_data_matches_fresh(case, hip):
    """new values on the same pattern (the only multi-chunk k_ms_gram after construction): bitwise a fresh handle, and the reference within the tolerance"""
    args2, refs, tols, err_orc = case.updated()
    delta, x_reg, z_reg = S.scalings("well", case.n, case.m)
    k = _handle(hip, case.args)
    assert k.update_scalings_and_factor(delta, x_reg, z_reg)
    before = k.solve(*case.rhs[0])
    k.update_data(hip.SparseData(*args2), hip.KKT_UPDATE_P | hip.KKT_UPDATE_A | hip.KKT_UPDATE_G)
    assert k.update_scalings_and_factor(delta, x_reg, z_reg)
    a = k.solve(*case.rhs[0])
    assert not np.array_equal(a[0], before[0])
    k2 = _handle(hip, args2)
    assert k2.update_scalings_and_factor(delta, x_reg, z_reg)
    assert _same(a, k2.solve(*case.rhs[0])), "updated handle and fresh handle differ"
    _check(f"{case.shape.name} updated data", a, refs[0], tols[0], err_orc[0])


def test_clone_bitwise(case, hip):
    delta, x_reg, z_reg = S.scalings("well", case.n, case.m)
    k = _handle(hip, case.args)
    assert k.update_scalings_and_factor(delta, x_reg, z_reg)
    c = k.clone()
    first = k.solve(*case.rhs[0])
    assert _same(c.solve(*case.rhs[0]), first), "the clone's copy of the factor solves differently"
    delta2, x_reg2, z_reg2 = S.scalings("ipm", case.n, case.m)
    assert c.update_scalings_and_factor(delta2, x_reg2, z_reg2) and k.update_scalings_and_factor(delta2, x_reg2, z_reg2)
    second = k.solve(*case.rhs[1])
    assert _same(c.solve(*case.rhs[1]), second), "the clone's own factorisation differs"
    assert not np.array_equal(second[0], first[0])


def _product_bound(M, v, k):
    return 8.0 * S.gamma(k) * (np.abs(M).astype(np.longdouble) @ np.abs(v).astype(np.longdouble))


@pytest.mark.parametrize("name", [S.ALL_HBM])
def test_eval_products_componentwise(orc, hip, name):
    """eval_* against longdouble products on the largest shape: |z - alpha M v| <= 8 gamma_k |alpha| |M| |v| componentwise, k the largest number of nonzeros in a row or
    column of M (k products, k - 1 additions and the scaling by alpha are at most k + 1 roundings in any order of summation: gamma_(k + 1) <= 2 gamma_k; 8 is generous
    and derived, not measured)"""
    case = _case(orc, name)
    n, p, m = case.shape.dims
    Pf, A, G = S.dense3(case.args)
    k = _handle(hip, case.args)
    rng = np.random.default_rng([n, 17])
    x, y, z = rng.standard_normal(n), rng.standard_normal(p), rng.standard_normal(m)
    ld = lambda M, v: M.astype(np.longdouble) @ v.astype(np.longdouble)
    nnz = lambda M: int(max((M != 0).sum(axis=0).max(), (M != 0).sum(axis=1).max()))
    out = k.eval_P_x(-1.5, x)
    assert (np.abs(out - (-1.5) * ld(Pf, x)) <= 1.5 * _product_bound(Pf, x, nnz(Pf))).all()
    for M, v, fn, an, at in ((A, y, k.eval_A_xn_and_AT_xt, -1.0, 2.0), (G, z, k.eval_G_xn_and_GT_xt, 0.5, -3.0)):
        zn, zt = fn(an, at, x, v)
        kk = nnz(M)
        assert (np.abs(zn - an * ld(M, x)) <= abs(an) * _product_bound(M, x, kk)).all()
        assert (np.abs(zt - at * ld(M.T, v)) <= abs(at) * _product_bound(M.T, v, kk)).all()
        assert np.abs(zn).max() > 0 and np.abs(zt).max() > 0
