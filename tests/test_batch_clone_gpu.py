"""clone() of the batched dense stack, whole or by a list of instances (pq_kkt_batch_clone_select, pq_kktsys_batch_clone_select, pq_solver_batch_clone,
pq_solver_batch_clone_select; piqp_amd.BatchDenseKKT / BatchKKTSystem / BatchDenseSolver .clone(instances)): instance j of the clone is instance idx[j] of the source.
A clone is a copy of bits, and what it computes afterwards is held to the CPU oracle of instance idx[j] (orc.KKT, orc.KKTSystem, orc.Solver) taken through the same
sequence of calls, on the raw doubles.  There is no tolerance in this file: equality is same() of tests/test_dense_exact_gpu.py.

Inputs and helpers are those of the existing tests of each layer (tests/batch_qp.py, tests/batch_qp_mixed.py, the Batch / Sys / MixedSys / Twin classes), imported as
they are.  Batches of 67 for n <= 31 and 9 for n >= 32.  The lists, one per source batch B: [B - 1, 0, 0, 3 % B, B - 1] (repeats, both ends, an odd count of 5 that
leaves the last workgroup of the four-instances-per-workgroup launch partly empty), the fan-out [2] * (B + 3) (count > B) and the single [1]."""
import gc

import numpy as np
import pytest

from batch_qp import feasible_batch, stacked
from batch_qp_mixed import mixed_batch
from test_dense_exact_gpu import lower, same
from test_dense_kkt_batch_gpu import batch_of, check_factor, check_solve as kb_check_solve, scalings
from test_dense_solver_batch_gpu import (KINDS, LDLT, LLT, MAX_ITER_REACHED, NAMES, PRIMAL_INFEASIBLE, SHAPES, SOLVED, TRACE_ROWS, check_solve, device, info_fields, oracle_of,
                                         oracle_run)
from test_dense_solver_batch_update_gpu import Twin, check_scaled, is_trap, new_handle, stack, update_args
from test_kktsys_batch_gpu import row, step as sys_step, sys_of
from test_kktsys_batch_lists_gpu import VARIANT, step as mixed_step, sys_of as mixed_sys_of

pytestmark = pytest.mark.gpu

PQ_ERR_INVALID = -1
ITEMS = ("P_utri", "AT", "GT", "c", "b", "h_l", "h_u", "x_l", "x_u", "x_b_scaling", "delta", "delta_b", "c_scale")


def sel(B):
    return [B - 1, 0, 0, 3 % B, B - 1]


def fan(B):
    return [2] * (B + 3)


ONE = [1]


def lists_of(B):
    return (sel(B), fan(B), ONE)


# ---- 1. the backend
@pytest.mark.parametrize("n,p,m", [(1, 0, 0), (3, 2, 3), (31, 7, 5), (32, 3, 5), (33, 0, 300), (128, 7, 5)], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_backend_clone_solves_without_factoring(hip, orc, kind, n, p, m):
    batch = 67 if n < 32 else 9
    B = batch_of(orc, n, p, m, batch, seed=1000 * n + 10 * p + m)
    rng = np.random.default_rng([n, p, m, kind, 5])
    k, kos = B.handle(hip, kind), B.oracles(orc, kind)
    flags = check_factor(k, kos, scalings(rng, batch, n, m), (n, p, m), matrices=False)
    assert flags.all()
    rx, ry, rz = rng.standard_normal((batch, n)), rng.standard_normal((batch, p)), rng.standard_normal((batch, m))
    before = [a.copy() for a in k.solve(rx, ry, rz)]
    for lst in lists_of(batch):
        c = k.clone(lst)
        assert (c.batch, c.n, c.p, c.m) == (len(lst), n, p, m)
        assert c.ok().all() and np.array_equal(c.first_bad_col(), k.first_bad_col()[lst])
        assert all(same(lower(c.internal_factor(j)), lower(kos[i].internal_factor())) for j, i in enumerate(lst))
        kb_check_solve(c, [kos[i] for i in lst], np.ones(len(lst), dtype=bool), rng, (n, p, m, "clone", len(lst)))  # no factorisation on the clone before this
        # other scalings on the clone: it is the oracle's handle of idx[j] with those, and the source keeps its bits
        kos2 = [orc.KKT(B.od[i], use_ldlt=kind == LDLT) for i in lst]
        f2 = check_factor(c, kos2, scalings(rng, len(lst), n, m), (n, p, m, "clone: its own factorisation"))
        kb_check_solve(c, kos2, f2, rng, (n, p, m, "clone: after its own factorisation"))
        after = k.solve(rx, ry, rz)
        assert all(same(a, b) for a, b in zip(before, after)), "the source's solve after the clone factored"


def test_the_refusals_of_the_two_lower_layers(hip, orc):
    import ctypes as C
    B = sys_of(orc, 4, 2, 3, 67)
    ks = B.handle(hip, LLT)
    for h, fn in ((ks.backend(), "pq_kkt_batch_clone_select"), (ks, "pq_kktsys_batch_clone_select")):
        f = getattr(h.L, fn)
        good, high, low = (np.array(v, dtype=np.intc) for v in ([0, 66, 3], [0, 67, 3], [0, 1, -1]))
        out = C.c_void_p(0x5A5A)
        a0 = h.L.pq_debug_alloc_count()
        for idx, count, words in ((None, 3, ("idx",)), (good, 0, ("count", "0")), (good, -2, ("count", "-2")), (high, 3, ("idx[1]", "67")), (low, 3, ("idx[2]", "-1"))):
            assert f(h.h, None if idx is None else idx.ctypes.data, count, C.byref(out)) == PQ_ERR_INVALID
            msg = h.L.pq_last_error_string().decode()
            assert all(w in msg for w in words), msg
            assert out.value == 0x5A5A
        assert f(h.h, good.ctypes.data, 3, None) == PQ_ERR_INVALID
        assert h.L.pq_debug_alloc_count() == a0, "a refusal comes before the device is touched"
    with pytest.raises(RuntimeError, match=r"idx\[1\] = 67"):
        ks.clone([0, 67])


# ---- 2. the KKT system
def vars_rows(rng, B, count):
    return {nm: rng.standard_normal((count, B.shapes[nm][1])) for nm in NAMES}


def check_sys_clone(c, kos, B, lst, used_of, rng, tag):
    """solve and mul on the clone, which was not factored: every number against the oracle of idx[j], which stands where the source stands"""
    rhs, lhs_mul = vars_rows(rng, B, len(lst)), vars_rows(rng, B, len(lst))
    xr, zr = c.x_reg(), c.z_reg()
    got = c.solve(rhs)
    mul = c.mul(lhs_mul)
    ok_d, steps_d, solves_d = c.solve_ok(), c.refine_steps(), c.backend_solves()
    bad = []
    for j, i in enumerate(lst):
        ko, used = kos[i], used_of(i)
        n0 = ko.L.orc_kkt_system_backend_solves(ko.ptr)
        ok, lhs = ko.solve(row(rhs, j))
        ref_mul = ko.mul(row(lhs_mul, j))
        assert ok, (tag, "the oracle solves", i)
        if not (ok_d[j] and steps_d[j] == ko.last_refine_steps() and solves_d[j] == ko.L.orc_kkt_system_backend_solves(ko.ptr) - n0):
            bad.append((j, "counts"))
        if not (same(xr[j], ko.x_reg()) and same(zr[j], ko.z_reg())):
            bad.append((j, "x_reg / z_reg"))
        bad += [(j, nm) for nm in NAMES if not same(got[nm][j, :used[nm]], lhs[nm][:used[nm]])]
        bad += [(j, "mul " + nm) for nm in NAMES if not same(mul[nm][j, :used[nm]], ref_mul[nm][:used[nm]])]
    assert not bad, (tag, bad)
    return steps_d


@pytest.mark.parametrize("n,p,m,batch", [(4, 2, 3, 67), (31, 7, 5, 67), (64, 40, 257, 9)], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_kkt_system_clone_solves_and_multiplies_without_factoring(hip, orc, kind, n, p, m, batch):
    B = sys_of(orc, n, p, m, batch)
    rng = np.random.default_rng([B.seed, kind, 23])
    k, kos = B.handle(hip, kind, "B"), B.oracles(orc, kind, "B")
    R = sys_step(k, kos, B, 1, rng, (n, p, m, "source"))  # refinement on in every instance
    assert all(R["ok_f"]) and all(R["ok_s"]) and max(R["steps"]) >= 1, "refinement is to run"
    for lst in lists_of(batch):
        c = k.clone(lst)
        assert (c.batch, c.n, c.p, c.m) == (len(lst), n, p, m) and c.lists is k.lists
        assert np.array_equal(c.refine_steps(), k.refine_steps()[lst]) and same(c.refine_error(), k.refine_error()[lst]) and same(c.rhs_norm(), k.rhs_norm()[lst])
        assert same(c.rhs_x_bar(), k.rhs_x_bar()[lst]) and same(c.rhs_z_bar(), k.rhs_z_bar()[lst])
        check_sys_clone(c, kos, B, lst, lambda i: B.used, rng, (n, p, m, len(lst)))
    # the source goes on from where it stands
    sys_step(k, kos, B, 0, rng, (n, p, m, "the source after the clones"))


@pytest.mark.parametrize("kind", KINDS)
def test_kkt_system_clone_with_lists_per_instance(hip, orc, kind):
    n, p, m, batch = 4, 2, 3, 67
    B = mixed_sys_of(orc, n, p, m, batch)
    rng = np.random.default_rng([B.seed, kind, 29])
    k, kos = B.handle(hip, kind), B.oracles(orc, kind, VARIANT)
    mixed_step(k, kos, B, 1, rng, (n, p, m, "source"))
    for lst in (sel(batch) + [1, 2], fan(batch), ONE):  # (instances 0 .. 3 are the forced patterns of tests/batch_qp_mixed.py)
        c = k.clone(lst)
        assert c.batch == len(lst) and c.per_inst and all(all(np.array_equal(a, b) for a, b in zip(c.lists[j], B.lists[i])) for j, i in enumerate(lst))
        check_sys_clone(c, kos, B, lst, B.used, rng, ("per instance", len(lst)))
    mixed_step(k, kos, B, 0, rng, (n, p, m, "the source after the clones"))


# ---- 3. the solver, fresh from setup
def box_counts(q):
    return int(np.isfinite(q["x_l"]).sum()), int(np.isfinite(q["x_u"]).sum())


def check_scaled_against_source(c, s, lst, qs):
    for j, i in enumerate(lst):
        nl, nu = box_counts(qs[i])
        for item in ITEMS:
            a, b = c.scaled_data(j, item), s.scaled_data(i, item)
            cut = nl if item == "x_l" else nu if item == "x_u" else None
            assert same(a[:cut], b[:cut]), f"clone instance {j} (source {i}): scaled {item}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,p,m,batch", SHAPES, ids=lambda v: str(v))
def test_solver_clone_fresh_from_setup(orc, hip, n, p, m, batch, kind):
    qs, ref = oracle_of(orc, hip, n, p, m, batch, kind)
    s = device(hip, qs, kind)
    for lst in (sel(batch), ONE):
        c = s.clone(lst)
        assert (c.batch, c.n, c.p, c.m) == (len(lst), n, p, m)
        check_scaled_against_source(c, s, lst, qs)
        assert c.solve() == sum(ref[i]["status"] == SOLVED for i in lst)
        check_solve(hip, c, [ref[i] for i in lst], f"clone {lst}")
    w = s.clone()
    assert w.batch == batch
    assert w.solve() == batch
    check_solve(hip, w, ref, "whole clone")
    assert s.solve() == batch
    check_solve(hip, s, ref, "the source after its clones")


# ---- 4. after a solve
def odd_batch(orc, hip):
    """8 instances at (4, 2, 3): instance 1 primal infeasible (as tests/test_dense_solver_batch_gpu.py builds it), instance 2 with a bound a billion away, which keeps
    it iterating (far_bounds there), and an iteration limit one above what the infeasible one needs: instance 2 stops short under it, the others solve"""
    qs = feasible_batch(4, 2, 3, 8)
    q = qs[1]
    q["G"], q["h_l"] = q["G"].copy(), q["h_l"].copy()
    q["G"][0] = q["A"][0]
    q["h_l"][0] = q["b"][0] + 100.0
    assert np.isfinite(qs[2]["h_l"][0])
    qs[2]["h_l"] = qs[2]["h_l"].copy()
    qs[2]["h_l"][0] -= 1e9
    full = oracle_run(orc, hip, qs, LLT)
    limit = full[1]["info"]["iter"] + 1
    assert limit < full[2]["info"]["iter"]
    short = oracle_run(orc, hip, qs, LLT, max_iter=limit)
    return qs, full, short, limit


def test_solver_clone_after_a_solve_hands_out_the_source_s_answers_and_solves_the_stragglers(orc, hip):
    qs, full, short, limit = odd_batch(orc, hip)
    st = [o["status"] for o in short]
    assert st == [SOLVED, PRIMAL_INFEASIBLE, MAX_ITER_REACHED] + [SOLVED] * 5, st
    assert all(o["status"] == SOLVED for i, o in enumerate(full) if i != 1)
    B = len(qs)
    lst = sel(B) + [1, 2]
    s = device(hip, qs, LLT, max_iter=limit)
    assert s.solve() == st.count(SOLVED)
    check_solve(hip, s, short)
    c = s.clone(lst)
    assert c.settings.max_iter == limit
    assert np.array_equal(c.statuses(), s.statuses()[lst]) and np.array_equal(c.iterations(), s.iterations()[lst])
    for nm in NAMES:
        assert same(c.result(nm), s.result(nm)[lst]), nm
        if s.result(nm).size:
            assert same(c.result(nm, device=True).cpu().numpy(), s.result(nm, device=True).cpu().numpy()[lst]), nm
    for j, i in enumerate(lst):
        a, b = c.info(j), s.info(i)
        assert all(same(getattr(a, k), getattr(b, k)) for k, _ in hip._lib.Info._fields_), (j, i)
        assert same(c.trace(j), s.trace(i)) and len(c.trace(j)) > 0
    check_solve(hip, c, [short[i] for i in lst], "the clone, not solved")
    # the stragglers again with a higher limit: each is the oracle that solves from scratch under that limit
    c.settings.max_iter = 250
    assert c.solve() == sum(full[i]["status"] == SOLVED for i in lst)
    check_solve(hip, c, [full[i] for i in lst], "the clone, solved with a higher limit")
    assert s.settings.max_iter == limit
    check_solve(hip, s, short, "the source after the clone's solve")


# ---- 5. after an update: the stored scalings and the stored P_diag
@pytest.mark.parametrize("reuse", [0, 1], ids=["reuse=0", "reuse=1"])
@pytest.mark.parametrize("n,p,m,batch", [(4, 2, 3, 67), (31, 7, 5, 67)], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_solver_clone_after_an_update(orc, hip, kind, n, p, m, batch, reuse):
    qs = feasible_batch(n, p, m, batch)
    settings = dict(preconditioner_reuse_on_update=reuse)
    lst = sel(batch)
    first = [dict(update_args(qs, i, "P"), **update_args(qs, i, "c")) for i in range(batch)]
    rng = np.random.default_rng([n, p, m, kind, reuse])
    second = [dict(c=qs[i]["c"] + 0.1 * rng.standard_normal(n)) for i in lst]
    exp_scaled, exp = [], []
    for j, i in enumerate(lst):
        t = Twin(orc, hip, qs[i], kind, settings)
        t.update(first[i], is_trap(first[i], p, reuse))
        t.update(second[j], False)
        exp_scaled.append(t.expected_scaled())
        exp.append(t.solve())
    s = new_handle(hip, qs, kind, settings)
    assert s.update(**stack(first)) is True
    c = s.clone(lst)
    assert c.settings.preconditioner_reuse_on_update == reuse
    assert c.update(**stack(second)) is True
    check_scaled(c, exp_scaled, "the clone after update(c)")
    assert c.solve() == sum(o["status"] == SOLVED for o in exp)
    check_solve(hip, c, exp, "the clone after update(c)")


# ---- 6. bound sets per instance
BOUNDS = ("h_l", "h_u", "x_l", "x_u")


def test_solver_clone_with_bound_sets_per_instance(orc, hip):
    n, p, m, batch = 4, 2, 3, 67
    q0, q1 = mixed_batch(n, p, m, batch), mixed_batch(n, p, m, batch, salt=1)
    lst = sel(batch) + [1, 2]  # 0 .. 3: the four forced patterns
    exp, scaled, counts = [], [], []
    for i in lst:
        o = orc.Solver()
        o.settings.kkt_solver = LLT
        assert o.setup(**q0[i])
        before = o.data().counts()
        assert o.update(**{k: q1[i][k] for k in BOUNDS})
        d = o.data()
        counts.append((before, d.counts()))
        sc = {k: np.array(d.mat(k)) for k in ("P_utri", "AT", "GT")}
        sc.update({k: np.array(d.vec(k)) for k in ("c", "b", "h_l", "h_u", "x_l", "x_u", "x_b_scaling")})
        scaled.append(sc)
        o.enable_trace(TRACE_ROWS)
        status = o.solve()
        exp.append(dict(status=status, info={k: getattr(o.info, k) for k in info_fields(hip)}, trace=o.trace(), result=o.result()))
    assert sum(a != b for a, b in counts) >= 5, "the update is to switch bounds off and on"
    s = hip.BatchDenseSolver(kkt_solver=LLT, bounds="per_instance")
    s.enable_trace(TRACE_ROWS)
    s.setup(**stacked(q0))
    c = s.clone(lst)
    assert c.bounds == "per_instance"
    for j, i in enumerate(lst):
        nl, nu = box_counts(q0[i])
        for item in ITEMS:
            cut = nl if item == "x_l" else nu if item == "x_u" else None
            assert same(c.scaled_data(j, item)[:cut], s.scaled_data(i, item)[:cut]), (j, item)
    a0 = s.L.pq_debug_alloc_count()
    assert c.update(**{k: np.stack([q1[i][k] for i in lst]) for k in BOUNDS}) is True
    for j, sc in enumerate(scaled):
        for k, v in sc.items():
            cut = counts[j][1][2] if k == "x_l" else counts[j][1][3] if k == "x_u" else None
            assert same(c.scaled_data(j, k)[:cut], v[:cut]), f"clone instance {j}: scaled {k} after the update"
    assert c.solve() == sum(o["status"] == SOLVED for o in exp)
    assert s.L.pq_debug_alloc_count() == a0
    check_solve(hip, c, exp, "per-instance sets")
    # the source still holds the sets of its setup
    ref0 = oracle_run(orc, hip, [q0[i] for i in (0, 1, 2, 3)], LLT)
    s.solve()
    res = {nm: s.result(nm) for nm in NAMES}
    assert all(same(res[nm][i], ref0[i]["result"][nm]) for i in range(4) for nm in NAMES)


def test_the_clone_of_a_shared_handle_refuses_an_update_that_changes_the_set(orc, hip):
    qs, _ = oracle_of(orc, hip, 4, 2, 3, 67, LLT)
    s = device(hip, qs, LLT)
    c = s.clone(sel(67))
    assert c.bounds == "shared"
    name = "x_l" if np.isfinite(qs[0]["x_l"]).any() else "x_u"
    j = int(np.flatnonzero(np.isfinite(qs[0][name]))[0])
    for h, rows in ((s, list(range(67))), (c, sel(67))):
        v = np.stack([qs[i][name] for i in rows])
        v[-1, j] = -np.inf if name == "x_l" else np.inf
        with pytest.raises(RuntimeError, match=f"the set of finite bounds of variable {j} changes in instance {len(rows) - 1}"):
            h.update(**{name: v})


# ---- 7. fan-out
def test_fan_out_one_nominal_problem_into_scenarios(orc, hip):
    n, p, m, batch = 4, 2, 3, 67
    qs, _ = oracle_of(orc, hip, n, p, m, batch, LLT)
    lst = fan(batch)
    copies = [qs[2]] * len(lst)
    args = [update_args(copies, j, "vectors") for j in range(len(lst))]
    exp_scaled, exp = [], []
    for a in args:
        t = Twin(orc, hip, qs[2], LLT, {})
        t.update(a, False)
        exp_scaled.append(t.expected_scaled())
        exp.append(t.solve())
    assert len({o["result"]["x"].tobytes() for o in exp}) == len(lst), "the scenarios are to differ"
    s = new_handle(hip, qs, LLT, {})
    c = s.clone(lst)
    assert c.batch == batch + 3
    assert c.update(**stack(args)) is True
    check_scaled(c, exp_scaled, "fan-out")
    assert c.solve() == sum(o["status"] == SOLVED for o in exp)
    check_solve(hip, c, exp, "fan-out")


# ---- 8. independence and lifetime
def scaled_of(s):
    return [s.scaled_data(i, item).copy() for i in range(s.batch) for item in ITEMS]


def snapshot(s):
    """everything a solved handle hands out"""
    return (scaled_of(s), [s.result(nm) for nm in NAMES], [s.trace(i) for i in range(s.batch)], s.statuses(), s.iterations())


def same_snapshot(a, b):
    return all(same(x, y) for u, v in zip(a[:3], b[:3]) for x, y in zip(u, v)) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


def test_source_and_clone_do_not_see_each_other(orc, hip):
    n, p, m, batch = 4, 2, 3, 67
    qs, ref = oracle_of(orc, hip, n, p, m, batch, LLT)
    lst = sel(batch)
    s = device(hip, qs, LLT)
    assert s.solve() == batch
    c = s.clone(lst)
    src = snapshot(s)
    assert c.update(c=np.stack([qs[(i + 1) % batch]["c"] for i in lst])) is True
    c.solve()
    assert same_snapshot(snapshot(s), src), "update and solve on the clone moved the source"
    cl = snapshot(c)
    assert not all(same(x, y) for x, y in zip(cl[1], [r[lst] for r in src[1]])), "the clone's update is to change its results"
    assert s.update(c=np.stack([qs[(i + 2) % batch]["c"] for i in range(batch)])) is True
    s.solve()
    assert same_snapshot(snapshot(c), cl), "update and solve on the source moved the clone"
    ks = c.kktsys()
    assert (ks.batch, ks.n, ks.p, ks.m) == (len(lst), n, p, m) and (ks.backend().batch, ks.backend().n) == (len(lst), n)
    assert ks.x_reg().shape == (len(lst), n)


def test_the_clone_outlives_its_source(orc, hip):
    n, p, m, batch = 31, 7, 5, 67
    qs, ref = oracle_of(orc, hip, n, p, m, batch, LLT)
    lst = sel(batch)
    s = device(hip, qs, LLT)
    c = s.clone(lst)
    s.L.pq_solver_batch_destroy(s.h)
    s.h = None
    del s
    gc.collect()
    filler = device(hip, qs, LLT)  # (takes memory again, some of it where the source's stood)
    assert filler.solve() == batch
    assert c.solve() == len(lst)
    check_solve(hip, c, [ref[i] for i in lst], "after the source's destruction")


def test_a_clone_of_a_clone_is_the_clone_by_the_composed_list(orc, hip):
    n, p, m, batch = 4, 2, 3, 67
    qs, ref = oracle_of(orc, hip, n, p, m, batch, LLT)
    s = device(hip, qs, LLT)
    assert s.solve() == batch
    l1, l2 = [5, 66, 0, 9, 9, 31, 2], [6, 6, 0, 3, 1]
    a = s.clone(l1).clone(l2)
    b = s.clone([l1[k] for k in l2])
    assert same_snapshot(snapshot(a), snapshot(b))
    for h in (a, b):
        assert h.solve() == len(l2)
    assert same_snapshot(snapshot(a), snapshot(b))
    check_solve(hip, a, [ref[l1[k]] for k in l2], "clone of a clone")
    w = s.clone().clone()
    assert same_snapshot(snapshot(w), snapshot(s))


# ---- 9. allocation
def test_only_the_clone_call_allocates(orc, hip):
    n, p, m, batch = 4, 2, 3, 67
    qs, ref = oracle_of(orc, hip, n, p, m, batch, LLT)
    s = device(hip, qs, LLT)
    count = s.L.pq_debug_alloc_count
    a0 = count()
    lst = fan(batch)
    c = s.clone(lst)
    a1 = count()
    assert a1 > a0
    assert c.update(c=np.stack([qs[2]["c"]] * len(lst))) is True
    assert c.solve() == len(lst)
    dev = {nm: c.result(nm, device=True) for nm in NAMES}
    assert count() == a1, "update, solve and the result calls of a clone must not allocate"
    assert all(same(dev[nm].cpu().numpy(), c.result(nm)) for nm in NAMES)
    assert s.update(c=np.stack([q["c"] for q in qs])) is True
    assert s.solve() == batch
    dev = {nm: s.result(nm, device=True) for nm in NAMES}
    assert count() == a1, "the source's loop stays free of allocations"


# ---- 10. torch, and the scalars of a handle that was never set up
def test_a_handle_set_up_from_cuda_tensors_clones_to_the_same_bits(orc, hip):
    import torch
    n, p, m, batch = 32, 3, 5, 9
    qs, ref = oracle_of(orc, hip, n, p, m, batch, LLT)
    host = device(hip, qs, LLT)
    t = hip.BatchDenseSolver(kkt_solver=LLT)
    t.enable_trace(TRACE_ROWS)
    t.setup(**{k: (None if v is None else torch.as_tensor(v).cuda()) for k, v in stacked(qs).items()})
    lst = sel(batch)
    a, b = t.clone(lst), host.clone(lst)
    assert all(same(x, y) for x, y in zip(scaled_of(a), scaled_of(b)))
    assert a.solve() == b.solve() == len(lst)
    assert same_snapshot(snapshot(a), snapshot(b))
    check_solve(hip, a, [ref[i] for i in lst], "clone of the torch-fed handle")


def test_the_clone_of_a_handle_that_was_never_set_up_carries_trace_rows_and_bound_mode(orc, hip):
    s = hip.BatchDenseSolver(kkt_solver=LDLT, bounds="per_instance")
    s.enable_trace(3)
    c = s.clone()
    assert c.batch is None and c.bounds == "per_instance" and c.kkt_solver == LDLT and c.settings.kkt_solver == LDLT
    with pytest.raises(RuntimeError, match="before setup"):
        c.clone([0])
    qs = mixed_batch(4, 2, 3, 8)
    c.setup(**stacked(qs))  # (a handle in the shared mode refuses this batch)
    assert c.solve() >= 1
    assert all(len(c.trace(i)) == 3 for i in range(8))
    shared = hip.BatchDenseSolver(kkt_solver=LDLT)
    with pytest.raises(RuntimeError, match="finite bounds"):
        shared.clone().setup(**stacked(qs))
