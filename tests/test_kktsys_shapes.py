"""CPU checks of tests/kktsys_shapes.py, the cases and the reference that tests/test_kktsys_kernels_gpu.py holds the KKTSystem shell to bit for bit.  Everything here
runs on the oracle alone (oracle/orc_kkt_system.c over its dense and its sparse_ldlt backend) and asserts what keeps the GPU test from being vacuous: every case
factors and solves, the refinement loop leaves through each of its five exits and takes three steps somewhere, the NumPy restatement of the elementwise formulas IS the
oracle's arithmetic on every case, and every non-finite right-hand side makes the oracle's solve return false while staying in its place."""
import numpy as np
import pytest
import scipy.sparse as sp

import kktsys_shapes as ks

BACKENDS = [pytest.param(False, id="dense"), pytest.param(True, id="sparse_ldlt")]


def kind_of(orc, sparse):
    return orc.SPARSE_LDLT if sparse else orc.DENSE_CHOLESKY


_runs = {}


def runs(orc, sparse):
    """every step of every handle on the oracle, computed once per backend: [(case, step index, lists, inputs, result, settings)]"""
    if sparse not in _runs:
        out = []
        for shape, rows, boxes, variant in ks.cases():
            q, xbs = ks.problem(shape, rows, boxes, sparse)
            od = ks.oracle_data(orc, q, xbs, sparse)
            d = ks.lists(od)
            st = orc.Settings(kkt_solver=kind_of(orc, sparse), **ks.VARIANTS[variant])
            ko = orc.KKTSystem(od, st)
            for i, inp in enumerate(ks.step_inputs(shape, rows, boxes, sparse, variant)):
                R = ks.oracle_step(ko, d, *inp)
                if R.ok_f and R.ok_s:  # what the restatement needs of the backend, taken while the oracle stands at this step
                    S = ks.scalings(d, inp[1], inp[2], inp[3])
                    R.mul_np = ks.mul_from_backend(ko.backend(), d, S, inp[5])
                    R.residual = ks.condensed_residual(ko, d, S, R.x_reg, R, inp[4])
                out.append(((shape, rows, boxes, variant), i, d, inp, R, st.s))
        _runs[sparse] = out
    return _runs[sparse]


def test_the_case_list_covers_what_it_claims():
    cs = ks.cases()
    assert len(cs) == len(set(cs)) == 16 * len(ks.SHAPES)
    for shape in ks.SHAPES:
        mine = [c for c in cs if c[0] == shape]
        assert {(r, b) for _, r, b, _ in mine} == {(r, b) for r in ks.ROW_PATTERNS for b in ks.BOX_PATTERNS}
        assert {v for *_, v in mine} == set(ks.VARIANTS)
    n, p, m = (np.array(a) for a in zip(*ks.SHAPES))
    assert ((n > p) & (n > m)).any() and ((p > n) & (p > m)).any() and ((m > n) & (m > p)).any()
    sizes = set(n) | set(p) | set(m)
    assert {63, 64, 65, 255, 256, 257} <= sizes and 0 in set(p) and 0 in set(m)
    assert n.max() > 512 and p.max() > 512 and m.max() > 512  # three blocks of 256 threads in each index space
    assert {(st, rk) for st, rk, _ in ks.STEPS} == {("early", "normal"), ("late", "normal"), ("early", "zero")} and {ref for *_, ref in ks.STEPS} == {0, 1}


@pytest.mark.parametrize("sparse", BACKENDS)
def test_bound_patterns_are_what_their_names_say(orc, sparse):
    for shape, rows, boxes, _ in ks.cases():
        q, xbs = ks.problem(shape, rows, boxes, sparse)
        d = ks.lists(ks.oracle_data(orc, q, xbs, sparse))
        n, p, m = shape
        assert (d.n, d.p, d.m) == shape and ks.same(d.xbs, xbs) and (xbs >= 0.5).all() and (xbs < 2.0).all()
        l, u = np.zeros(m, bool), np.zeros(m, bool)
        l[d.h_l], u[d.h_u] = True, True
        assert (l | u).all(), "a row without a finite bound"
        if rows == "two-sided":
            assert (l & u).all()
        elif rows == "lower":
            assert l.all() and not u.any()
        elif rows == "upper":
            assert u.all() and not l.any()
        elif m >= 63:
            assert (l & u).any() and (l & ~u).any() and (u & ~l).any()
        nl, nu = len(d.x_l), len(d.x_u)
        assert (nl, nu) == dict(none=(0, 0), both=(n, n), lower=(n, 0)).get(boxes, (nl, nu))
        if boxes == "mixed" and n >= 64:
            bl, bu = np.zeros(n, bool), np.zeros(n, bool)
            bl[d.x_l], bu[d.x_u] = True, True
            assert (bl & bu).any() and (bl & ~bu).any() and (bu & ~bl).any() and (~bl & ~bu).any()
        if sparse and n >= 2:
            assert (d.P_diag == 0.0).any() and (d.P_diag != 0.0).any(), "no structurally absent diagonal entry of P"


@pytest.mark.parametrize("sparse", BACKENDS)
def test_every_case_factors_and_solves_and_every_loop_exit_is_taken(orc, sparse):
    rs = runs(orc, sparse)
    assert len(rs) == 16 * len(ks.SHAPES) * len(ks.STEPS)
    bad = [(case, i) for case, i, d, inp, R, st in rs if not (R.ok_f and R.ok_s)]
    assert not bad, bad
    exits = np.array([R.exit for case, i, d, inp, R, st in rs if inp[0]])
    steps = np.array([R.steps for case, i, d, inp, R, st in rs if inp[0]])
    print("exits 0..4:", np.bincount(exits, minlength=5), "steps:", np.bincount(steps))
    assert set(exits) == {0, 1, 2, 3, 4}, np.bincount(exits, minlength=5)
    assert steps.max() >= 3, np.bincount(steps)
    for case, i, d, inp, R, st in rs:
        if not inp[0]:  # refinement off: one backend solve, nothing recorded
            assert (R.steps, R.solves, R.exit, R.refine_error, R.rhs_norm) == (0, 1, -1, 0.0, 0.0), (case, i)
            continue
        # what an exit says about the course of the loop
        assert R.solves == R.steps + 1 and 0 <= R.steps <= st.iterative_refinement_max_iter, (case, i)
        tol = st.iterative_refinement_eps_abs + st.iterative_refinement_eps_rel * R.rhs_norm
        if R.exit == 0:
            assert R.steps == 0 and R.refine_error <= tol and st.iterative_refinement_max_iter > 0, (case, i)
        elif R.exit == 1:
            assert R.steps >= 1 and R.refine_error <= tol, (case, i)
        elif R.exit in (2, 3):
            assert R.steps >= 1, (case, i)  # (the stall is seen before the tolerance is looked at again)
        else:
            assert R.steps == st.iterative_refinement_max_iter, (case, i)
        # the recorded error is that of the iterate the loop kept: the residual recomputed from what the solve returned
        assert ks.same(R.residual[0], R.refine_error) and ks.same(R.residual[1], R.rhs_norm), (case, i, R.residual, R.refine_error, R.rhs_norm)
    # an all-zero right-hand side: zeros of both signs come out of the shell
    zero = [R for case, i, d, inp, R, st in rs if ks.STEPS[i][1] == "zero"]
    assert all(not np.any(R.lhs[nm]) for R in zero for nm in ks.NAMES)
    assert any(np.signbit(R.lhs[nm]).any() for R in zero for nm in ks.NAMES) and any((~np.signbit(R.lhs[nm])).any() for R in zero for nm in ks.NAMES)


@pytest.mark.parametrize("sparse", BACKENDS)
def test_the_numpy_restatement_is_the_oracle_bit_for_bit(orc, sparse):
    bad = []
    for case, i, d, (refine, rho, delta, v, rhs, lhs_mul), R, st in runs(orc, sparse):
        S = ks.scalings(d, rho, delta, v)
        x_reg = ks.static_regularization(d, S, st)[1] if refine else S.x_reg
        rxb, rzb = ks.rhs_bars(d, S, rhs)
        rec = ks.recover(d, S, rhs, R.lhs["x"], R.lhs_z)
        what = [("x_reg", ks.same(x_reg, R.x_reg)), ("z_reg", ks.same(S.z_reg, R.z_reg)), ("rhs_x_bar", ks.same(rxb, R.rxb)), ("rhs_z_bar", ks.same(rzb, R.rzb)),
                ("recover", not ks.differing(d, rec, R.lhs, ks.NAMES[2:])), ("mul", not ks.differing(d, R.mul_np, R.mul))]
        bad += [(case, i, nm) for nm, ok in what if not ok]
    assert not bad, (len(bad), bad[:20])


# ------------------------------------------------------------------------------------------------------------------- non-finite right-hand sides
def nonfinite_setup(orc, slot, refine):
    q, xbs = ks.decoupled_problem(slot)
    od = ks.oracle_data(orc, q, xbs, True)
    d = ks.lists(od)
    ko = orc.KKTSystem(od, orc.Settings(kkt_solver=orc.SPARSE_LDLT))
    rng = np.random.default_rng([ord(slot), refine])
    rho, delta, v = ks.state("early", ks.SLOT_SHAPES[slot], rng)
    assert ko.update_scalings_and_factor(refine, rho, delta, v)
    return od, d, ko, (rho, delta, v), ks.rhs_of("normal", ks.SLOT_SHAPES[slot], rng)


def test_the_decoupled_problems_are_decoupled():
    for slot, (n, p, m) in ks.SLOT_SHAPES.items():
        q, _ = ks.decoupled_problem(slot)
        assert (q["P"].shape[0], q["A"].shape[0], q["G"].shape[0]) == (n, p, m) and dict(x=n, y=p, z=m)[slot] == max(n, p, m) == ks.POSITIONS[-1] + 1
        assert sorted(i for i in ks.POSITIONS if i >= min(n, p, m)) == [63, 64, 255, 256, 299] and max(sorted((n, p, m))[:2]) <= 63
        assert (q["P"] - sp.diags(q["P"].diagonal())).nnz == 0
        A, G = q["A"].tocsr(), q["G"].tocsr()
        assert np.diff(A.indptr).max() == 1 and np.diff(G.indptr).max() == 1 and np.diff(A.indptr).min() == 0 and np.diff(G.indptr).min() == 0
        touched = np.zeros(n, bool)
        touched[A.indices] = True
        touched[G.indices] = True
        assert not touched.all()
        for pos in ks.POSITIONS:
            if slot == "x":
                assert not touched[pos] and np.isinf(q["x_l"][pos]) and np.isinf(q["x_u"][pos])
            else:
                M = A if slot == "y" else G
                assert M.indptr[pos + 1] == M.indptr[pos]
                assert slot == "y" or np.isfinite(q["h_u"][pos])


@pytest.mark.parametrize("refine", [0, 1], ids=["off", "on"])
@pytest.mark.parametrize("slot", ["x", "y", "z"])
def test_a_non_finite_right_hand_side_fails_on_the_oracle_and_stays_in_its_place(orc, slot, refine):
    od, d, ko, state, rhs = nonfinite_setup(orc, slot, refine)
    ok, clean = ko.solve(rhs)
    assert ok and all(np.isfinite(a).all() for a in clean.values())
    kb = orc.KKT(od, kind="sparse", mode=0)  # the backend alone, on the matrix of this state: where the spoiled entry of the condensed right-hand side goes
    assert kb.update_scalings_and_factor(state[1], ko.x_reg(), ko.z_reg())
    for s, pos, val in ks.nonfinite_cases():
        if s != slot:
            continue
        bad = ks.spoiled(rhs, slot, pos, val)
        ok, _ = ko.solve(bad)
        assert not ok, (slot, pos, val, "the oracle's solve returns true")
        lx, ly, lz = kb.solve(ko.rhs_x_bar(), bad["y"], ko.rhs_z_bar())
        where = {nm: np.flatnonzero(~np.isfinite(a)) for nm, a in (("x", lx), ("y", ly), ("z", lz))}
        assert {nm: list(w) for nm, w in where.items()} == {nm: ([pos] if nm == slot else []) for nm in "xyz"}, (slot, pos, val, where)
        ok, again = ko.solve(rhs)
        assert ok and not ks.differing(d, again, clean), (slot, pos, val)
