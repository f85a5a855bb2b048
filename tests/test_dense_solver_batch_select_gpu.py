"""BatchDenseSolver.solve / update / result with instances=... (pq_solver_batch_solve_select, pq_solver_batch_update_dense_select,
pq_solver_batch_get_result_select_mem; piqp_amd/csrc/dense_solver_batch.hip): the calls that act on a list of instances of a batch in place.

The yardstick is the WHOLE-BATCH path on a twin handle, bit for bit: a listed instance must end where the whole-batch call given the same row leaves it, an unlisted
instance must be, byte for byte, what a snapshot taken before the call shows.  There is no tolerance in this file and no instance is left out: equality is same() of
tests/test_dense_exact_gpu.py.  What is compared per instance (record()): the 13 items of scaled_data, every field of pq_info (the time fields only against a
snapshot of the same handle), the trace, the ten result vectors, and of the borrowed KKT system x_reg, z_reg, rhs_x_bar, rhs_z_bar, the five diagnostics of
pq_kktsys_batch_info and the stored factor.  The KKT system's x_b_scaling and P_diag have no getter of their own: x_b_scaling enters x_reg of the next
factorisation and P_diag the regularisation of a refined one.  So every test that updates by list ends with a whole solve() after which the UNLISTED instances, whose
data did not change and which start from INIT, must again be bitwise the snapshot (results, info, trace, KKT state and factor) and the listed ones the twin's; and one
test gives the unlisted instances a stale P_diag first (a whole update(A, b) that recomputes the scalings and leaves P_diag alone), updates P of the others by list
and holds the whole solve with refinement always on against a handle that got the first update only.  One test anchors the listed rows to the CPU oracle.

Inputs: feasible_batch / mixed_batch of tests/batch_qp.py and tests/batch_qp_mixed.py.  What a test needs from them (every instance SOLVED, at least two iteration
counts in a batch, a mixed outcome under a low max_iter) is asserted on the twin before it is used."""
import numpy as np
import pytest

from batch_qp import feasible_batch, stacked
from batch_qp_mixed import mixed_batch
from test_dense_exact_gpu import same
from test_dense_solver_batch_gpu import LDLT, LLT, MAX_ITER_REACHED, NAMES, SOLVED, TIMES, TRACE_ROWS, info_fields
from test_dense_solver_batch_update_gpu import Twin, stack, to_torch, update_args

pytestmark = pytest.mark.gpu

ITEMS = ("P_utri", "AT", "GT", "c", "b", "h_l", "h_u", "x_l", "x_u", "x_b_scaling", "delta", "delta_b", "c_scale")
KKT = ("x_reg", "z_reg", "rhs_x_bar", "rhs_z_bar", "solve_ok", "refine_steps", "backend_solves", "refine_error", "rhs_norm")
# (n, p, m, batch), kind: the packed path at its smallest n; four instances per workgroup, ragged; below, at and above n = 32 (m past one K block); the 64-thread solve;
# the full LDS square
CASES = [((1, 0, 0, 6), LLT), ((4, 2, 3, 13), LLT), ((4, 2, 3, 13), LDLT), ((31, 7, 5, 9), LLT), ((32, 3, 5, 9), LLT), ((33, 0, 300, 6), LLT), ((64, 40, 257, 6), LLT),
         ((128, 7, 5, 6), LLT), ((128, 7, 5, 6), LDLT)]
MIXED = [c for c in CASES if c[0] != (1, 0, 0, 6)]  # the batches whose instances take at least two different numbers of iterations (the CPU oracle's: 5-7, 6-8, 7-9, 9-12, 7-12, 8-10)
case_id = lambda c: f"{c[0]}-{'llt' if c[1] == LLT else 'ldlt'}"
SETS = ("c", "vectors", "P", "A,b", "G,h", "all")


def lists_of(shape):
    """a single instance, a descending list, first and last, a permutation of all, the identity; at (4, 2, 3, 13) lists whose members sit in different packed workgroups"""
    B = shape[3]
    perm = np.random.default_rng(97 + B).permutation(B).tolist()
    out = [[B // 2], list(range(B - 1, -1, -2)), [0, B - 1], perm, list(range(B))]
    if shape == (4, 2, 3, 13):
        out += [[12], [9, 2, 7, 0], [11, 3, 4, 8, 0]]
    return out


def handle(hip, qs, kind, bounds="shared", **settings):
    s = hip.BatchDenseSolver(kkt_solver=kind, bounds=bounds)
    for k, v in settings.items():
        setattr(s.settings, k, v)
    s.enable_trace(TRACE_ROWS)
    s.setup(**stacked(qs))
    return s


def record(hip, s):
    """per instance a dict of everything the handle hands out about it, as arrays"""
    B = s.batch
    rec = [dict() for _ in range(B)]
    for i in range(B):
        for k in ITEMS:
            rec[i]["scaled " + k] = s.scaled_data(i, k).copy()
        info = s.info(i)
        for k in info_fields(hip) + ["n_backend_solve"]:
            rec[i]["info " + k] = np.array(getattr(info, k))
        rec[i]["times"] = np.array([getattr(info, k) for k in TIMES])
    try:
        res = {nm: s.result(nm) for nm in NAMES}
    except RuntimeError:  # no solve yet
        return rec
    for i in range(B):
        rec[i]["trace"] = s.trace(i)
        for nm in NAMES:
            rec[i]["result " + nm] = res[nm][i].copy()
    ks = s.kktsys()
    try:
        kk = {k: getattr(ks, k)() for k in KKT}
        fac = [ks.backend().internal_factor(i) for i in range(B)]
    except RuntimeError:  # lists replaced and no factorisation since
        return rec
    for i in range(B):
        for k in KKT:
            rec[i]["kkt " + k] = np.array(kk[k][i])
        rec[i]["kkt factor"] = fac[i]
    return rec


def hold(a, b, pairs, tag, times):
    """instance i of record a is instance j of record b for (i, j) in pairs, on every key (the time fields only if asked)"""
    for i, j in pairs:
        assert a[i].keys() == b[j].keys(), f"{tag}: instance {i} hands out {sorted(set(a[i]) ^ set(b[j]))} on one side only"
        for k in a[i]:
            if k == "times" and not times:
                continue
            assert same(a[i][k], b[j][k]), f"{tag}: instance {i}: {k}"


def listed(a, twin, lst, tag):
    hold(a, twin, [(i, i) for i in lst], tag + " (listed, against the twin)", times=False)


def unlisted(a, snap, lst, tag, times=True):
    hold(a, snap, [(i, i) for i in range(len(a)) if i not in set(lst)], tag + " (unlisted, against the snapshot)", times=times)


_twins = {}


def solved_twin(hip, shape, kind):
    """(the batch, the record of a handle that was set up and solved whole with the default settings): computed once per case and shared; nobody changes it"""
    key = (shape, kind)
    if key not in _twins:
        qs = feasible_batch(*shape)
        t = handle(hip, qs, kind)
        assert t.solve() == shape[3], "every instance is to end SOLVED"
        if (shape, kind) in MIXED:
            assert len(set(t.iterations().tolist())) >= 2, f"the instances run in lock step: {t.iterations().tolist()}"
        _twins[key] = (qs, record(hip, t))
    return _twins[key]


# ---- 1. solve by list on a fresh handle
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_solve_by_list_on_a_fresh_handle(hip, case):
    shape, kind = case
    qs, twin = solved_twin(hip, shape, kind)
    B = shape[3]
    count = hip._lib.load().pq_debug_alloc_count
    for lst in lists_of(shape):
        s = handle(hip, qs, kind)
        snap = record(hip, s)
        a0 = count()
        assert s.solve(instances=lst) == len(lst)  # (every instance of the twin is SOLVED)
        assert count() == a0 + 1, "the first call on a list allocates the list's buffer and nothing else"
        rec = record(hip, s)
        listed(rec, twin, lst, f"solve({lst})")
        for i in set(range(B)) - set(lst):  # never solved: what the setup left, zeros and no trace row
            for k, v in snap[i].items():
                assert same(rec[i][k], v), f"solve({lst}): unlisted instance {i}: {k}"
            assert rec[i]["trace"].shape == (0, 11) and all(not rec[i]["result " + nm].any() for nm in NAMES)
            assert s.info(i).status == snap[i]["info status"] and s.info(i).iter == 0
        a1 = count()
        assert s.solve(instances=lst) == len(lst) and count() == a1, "a second call on a list allocates nothing"
        again = record(hip, s)
        listed(again, twin, lst, f"second solve({lst})")
        unlisted(again, rec, lst, f"second solve({lst})")
        assert s.solve() == B
        hold(record(hip, s), twin, [(i, i) for i in range(B)], f"the whole solve after solve({lst})", times=False)


# ---- 2. stragglers
@pytest.mark.parametrize("case", MIXED, ids=case_id)
def test_stragglers_are_run_again_in_place_under_a_larger_cap(hip, case):
    shape, kind = case
    qs, twin = solved_twin(hip, shape, kind)
    cap = min(int(r["info iter"]) for r in twin) + 1  # the batch's smallest iteration count + 1: the instances that need it end SOLVED, every other one hits the cap
    s = handle(hip, qs, kind)
    large = s.settings.max_iter
    s.settings.max_iter = cap
    n_solved = s.solve()
    st = s.statuses()
    assert 0 < n_solved < shape[3] and set(st.tolist()) == {SOLVED, MAX_ITER_REACHED}, f"no mixed outcome under max_iter = {cap}: {st.tolist()}"
    assert all((st[i] == SOLVED) == (twin[i]["info iter"] < cap) for i in range(shape[3]))
    snap = record(hip, s)
    stragglers = np.flatnonzero(st != SOLVED)
    s.settings.max_iter = large
    assert s.solve(instances=stragglers) == len(stragglers)
    rec = record(hip, s)
    listed(rec, twin, stragglers.tolist(), "stragglers")
    unlisted(rec, snap, stragglers.tolist(), "stragglers")
    ms = s.last_ms()
    assert 3 * max(int(twin[i]["info iter"]) for i in stragglers) <= ms["rounds"] <= s.max_rounds()


# ---- 3. update by list, then solve by list
def twin_args(qs, lst, new):
    """the whole-batch arguments that give the listed instances their new rows: for every key some listed instance gets, an unlisted instance gets its own data"""
    keys = sorted({k for a in new for k in a})
    rows = {i: a for i, a in zip(lst, new)}
    return {k: np.stack([rows[i][k] if i in rows else qs[i][k] for i in range(len(qs))]) for k in keys}


def update_cases():
    out = []
    for shape, kind in CASES:
        for name in SETS:
            if (name == "A,b" and shape[1] == 0) or (name == "G,h" and shape[2] == 0):
                continue
            out.append(pytest.param(shape, kind, name, id=f"{case_id((shape, kind))}-{name}"))
    return out


@pytest.mark.parametrize("shape,kind,name", update_cases())
def test_update_by_list_then_solve_by_list(hip, shape, kind, name):
    qs = feasible_batch(*shape)
    B = shape[3]
    count = hip._lib.load().pq_debug_alloc_count
    feeds = ("numpy", "row-major", "column-major") if any(k in name for k in "PAG") else ("numpy", "row-major")  # (the order is the matrices')
    for lst, reuse, feed in [(l, r, f) for l in lists_of(shape) for r in (0, 1) for f in feeds]:
        tag = f"update({name}, {lst}), reuse = {reuse}, {feed}"
        s, t = (handle(hip, qs, kind, preconditioner_reuse_on_update=reuse) for _ in range(2))
        assert s.solve() == B and t.solve() == B  # (the unlisted instances keep the results and the factor of this solve)
        snap = record(hip, s)
        new = [update_args(qs, i, name) for i in lst]
        a = stack(new)
        a0 = count()
        assert s.update(**(a if feed == "numpy" else to_torch(a, feed)), instances=lst) is True
        assert count() == a0 + 1
        assert t.update(**twin_args(qs, lst, new)) is True
        rec, twin = record(hip, s), record(hip, t)
        for i in lst:
            for k in ITEMS:
                assert same(rec[i]["scaled " + k], twin[i]["scaled " + k]), f"{tag}: instance {i}: scaled {k}"
            assert all(same(rec[i][k], snap[i][k]) for k in rec[i] if k.startswith(("result", "trace", "info"))), f"{tag}: instance {i} keeps its last solve"
            assert s.info(i).update_time > 0 and s.info(i).update_time == s.last_update_ms()["wall_ms"] * 1e-3
        unlisted(rec, snap, lst, tag)
        n_solved = s.solve(instances=lst)
        t.solve()
        assert count() == a0 + 1, "no allocation after the first call on a list"
        rec, twin = record(hip, s), record(hip, t)
        assert n_solved == sum(int(twin[i]["info status"]) == SOLVED for i in lst)
        listed(rec, twin, lst, tag + ", solved")
        unlisted(rec, snap, lst, tag + ", solved")
        for i in lst:
            assert s.info(i).run_time == s.info(i).update_time + s.info(i).solve_time
        # the whole solve: an unlisted instance starts from INIT on data, x_b_scaling and P_diag that no call touched, so it ends on the snapshot's bits again
        assert s.solve() == t.solve()
        rec, twin = record(hip, s), record(hip, t)
        listed(rec, twin, lst, tag + ", solved whole")
        unlisted(rec, snap, lst, tag + ", solved whole", times=False)


def test_an_update_by_list_without_arguments_is_an_unscale_and_rescale_of_the_listed_rows(hip):
    shape, kind, lst = (4, 2, 3, 13), LLT, [9, 2, 7, 0]
    qs = feasible_batch(*shape)
    s, t = handle(hip, qs, kind), handle(hip, qs, kind)
    assert s.solve() == 13 and t.solve() == 13
    snap = record(hip, s)
    assert s.update(instances=lst) is True and t.update() is True
    rec, twin = record(hip, s), record(hip, t)
    listed(rec, twin, lst, "update()")
    unlisted(rec, snap, lst, "update()")
    assert any(not same(rec[i]["scaled P_utri"], snap[i]["scaled P_utri"]) for i in lst), "unscaling and rescaling move P by roundings"
    assert s.solve() == 13 and t.solve() == 13
    rec, twin = record(hip, s), record(hip, t)
    listed(rec, twin, lst, "update(), then a whole solve")
    unlisted(rec, snap, lst, "update(), then a whole solve", times=False)


def test_an_unlisted_instance_keeps_its_stale_p_diag(hip):
    """P_diag is taken at an update that carries P and at no other (kkt_system.hpp:134-141).  A whole update(A, b) with preconditioner_reuse_on_update = 0 rescales P
    and leaves P_diag alone, so every instance holds a P_diag that is not its diagonal; an update(P) of some instances by list must take P_diag again for those and
    for no other.  With refinement always on P_diag enters the regularisation of every factorisation (max_diag), and with it x_reg, the factor and the iterates."""
    shape, kind, lst = (4, 2, 3, 13), LLT, [12, 1, 5, 8]
    qs = feasible_batch(*shape)
    settings = dict(preconditioner_reuse_on_update=0, iterative_refinement_always_enabled=1)
    s, r, t = (handle(hip, qs, kind, **settings) for _ in range(3))
    first = stack([update_args(qs, i, "A,b") for i in range(13)])
    assert s.update(**first) is True and r.update(**first) is True and t.update(**first) is True
    new = [update_args(qs, i, "P") for i in lst]
    assert s.update(**stack(new), instances=lst) is True
    assert t.update(**twin_args(qs, lst, new)) is True
    assert s.solve() == r.solve()
    t.solve()
    rec, ref, twin = record(hip, s), record(hip, r), record(hip, t)
    unlisted(rec, ref, lst, "against the handle that got update(A, b) only", times=False)
    listed(rec, twin, lst, "update(P) by list after update(A, b)")


# ---- 4. one oracle anchor
@pytest.mark.parametrize("shape", [(4, 2, 3, 13), (33, 0, 300, 6)], ids=str)
def test_the_listed_rows_are_the_oracles(orc, hip, shape):
    qs = feasible_batch(*shape)
    lst = lists_of(shape)[1]
    s = handle(hip, qs, LLT)
    twins = {i: Twin(orc, hip, qs[i], LLT, {}) for i in lst}

    def check(tag):
        exp = {i: twins[i].solve() for i in lst}
        assert s.solve(instances=lst) == sum(o["status"] == SOLVED for o in exp.values())
        res = {nm: s.result(nm, instances=lst) for nm in NAMES}
        for j, i in enumerate(lst):
            info, o = s.info(i), exp[i]
            for k in info_fields(hip):
                assert same(getattr(info, k), o["info"][k]), f"{tag} instance {i}: info.{k}"
            assert info.status == o["status"] and same(s.trace(i), o["trace"]), f"{tag} instance {i}: status or trace"
            for nm in NAMES:
                assert same(res[nm][j], o["result"][nm]), f"{tag} instance {i}: result {nm}"

    check("first solve")
    new = [update_args(qs, i, "vectors") for i in lst]
    for i, a in zip(lst, new):
        twins[i].update(a, False)
    assert s.update(**stack(new), instances=lst) is True
    for i in lst:
        for k, v in twins[i].expected_scaled().items():
            assert same(s.scaled_data(i, k), v), f"instance {i}: scaled {k}"
    check("after update(vectors)")


# ---- 5. per-instance bound sets
def test_per_instance_sets_follow_an_update_by_list(hip):
    shape = (4, 2, 3, 13)
    n, p, m, B = shape
    qs = mixed_batch(*shape)
    two_sided = [i for i, q in enumerate(qs) if (np.isfinite(q["h_l"]) & np.isfinite(q["h_u"])).any() and (np.isfinite(q["x_l"]) & np.isfinite(q["x_u"])).any()]
    lst = [two_sided[-1], two_sided[0]]
    assert len(two_sided) >= 2 and lst[0] != lst[1]
    s, t = handle(hip, qs, LLT, bounds="per_instance"), handle(hip, qs, LLT, bounds="per_instance")
    assert s.solve() == t.solve()
    snap = record(hip, s)
    keys = ("h_l", "h_u", "x_l", "x_u")
    off = []
    for i in lst:
        q = {k: qs[i][k].copy() for k in keys}
        r = int(np.flatnonzero(np.isfinite(q["h_l"]) & np.isfinite(q["h_u"]))[0])
        v = int(np.flatnonzero(np.isfinite(q["x_l"]) & np.isfinite(q["x_u"]))[0])
        q["h_l"][r], q["x_u"][v] = -np.inf, np.inf  # a row and a box bound switched off
        off.append(q)
    on = [{k: qs[i][k] for k in keys} for i in lst]
    for step, new in (("off", off), ("on again", on)):
        assert s.update(**stack(new), instances=lst) is True
        assert t.update(**twin_args(qs, lst, new)) is True
        rec, twin = record(hip, s), record(hip, t)
        for i in lst:
            for k in ITEMS:
                assert same(rec[i]["scaled " + k], twin[i]["scaled " + k]), f"{step}: instance {i}: scaled {k}"
        for i in set(range(B)) - set(lst):  # (the lists were replaced: the KKT system's hooks wait for the next factorisation)
            assert all(same(rec[i][k], snap[i][k]) for k in rec[i]), f"{step}: unlisted instance {i}"
        n_solved = s.solve(instances=lst)
        t.solve()
        rec, twin = record(hip, s), record(hip, t)
        assert n_solved == sum(int(twin[i]["info status"]) == SOLVED for i in lst)
        listed(rec, twin, lst, step)
        unlisted(rec, snap, lst, step)
    assert s.solve() == t.solve()
    rec, twin = record(hip, s), record(hip, t)
    listed(rec, twin, lst, "the whole solve at the end")
    unlisted(rec, snap, lst, "the whole solve at the end", times=False)


def test_the_kkt_system_waits_for_every_instance_whose_lists_were_replaced(hip):
    shape = (4, 2, 3, 13)
    qs = mixed_batch(*shape)
    s = handle(hip, qs, LLT, bounds="per_instance")
    s.solve()
    keys = ("h_l", "h_u", "x_l", "x_u")
    assert s.update(**stack([{k: qs[i][k] for k in keys} for i in (3, 9)]), instances=[3, 9]) is True
    for others in ([0, 12], [9]):  # a solve that leaves a relisted instance out does not end the wait
        s.solve(instances=others)
        with pytest.raises(RuntimeError, match="before update_scalings_and_factor|no factorisation yet"):
            s.kktsys().x_reg()
    s.solve(instances=[3])
    assert s.kktsys().x_reg().shape == (13, 4)


# ---- 6. shared sets
def test_a_listed_row_that_changes_the_shared_set_is_refused(hip):
    shape, kind = (4, 2, 3, 13), LLT
    qs, twin = solved_twin(hip, shape, kind)
    s = handle(hip, qs, kind)
    assert s.solve() == 13
    snap = record(hip, s)
    name = "x_l" if np.isfinite(qs[0]["x_l"]).any() else "x_u"
    j = int(np.flatnonzero(np.isfinite(qs[0][name]))[0])
    lst = [11, 3, 8]
    v = np.stack([qs[i][name] for i in lst])
    v[1, j] = -np.inf if name == "x_l" else np.inf
    import torch
    for feed in (lambda a: a, lambda a: torch.as_tensor(a).cuda()):
        with pytest.raises(RuntimeError, match=f"the set of finite bounds of variable {j} changes in instance 3 "):
            s.update(**{name: feed(v)}, instances=lst)
        hold(record(hip, s), snap, [(i, i) for i in range(13)], "after the refused update", times=True)
    assert s.solve() == 13
    hold(record(hip, s), twin, [(i, i) for i in range(13)], "the whole solve after the refused update", times=False)


# ---- 7. result by list
@pytest.mark.parametrize("case", [((1, 0, 0, 6), LLT), ((4, 2, 3, 13), LLT), ((33, 0, 300, 6), LLT)], ids=case_id)
def test_result_by_list(hip, case):
    shape, kind = case
    qs, _ = solved_twin(hip, shape, kind)
    B = shape[3]
    s = handle(hip, qs, kind)
    assert s.solve() == B
    rng = np.random.default_rng(5)
    for lst in ([B - 1], [0, 0, B - 1, 0], rng.integers(0, B, 3 * B + 1).tolist(), list(range(B))):  # repeats, count > batch
        for nm in NAMES:
            whole = s.result(nm)
            host, dev = s.result(nm, instances=lst), s.result(nm, device=True, instances=lst)
            assert host.shape == dev.shape == (len(lst), whole.shape[1])
            assert same(host, whole[lst]) and same(dev.cpu().numpy(), whole[lst]), f"result({nm}, {lst})"
    if shape[1] == 0:  # a field of length 0 writes nothing
        o = np.full(4, -7.0)
        idx = np.array([1, 0], dtype=np.intc)
        assert s.L.pq_solver_batch_get_result_select_mem(s.h, idx.ctypes.data, 2, NAMES.index("y"), o.ctypes.data, 0) == 0 and o.tolist() == [-7.0] * 4
        for device in (False, True):  # the refusals hold for the empty field too
            with pytest.raises(RuntimeError, match=f"idx\\[1\\] = {B}"):
                s.result("y", device=device, instances=[0, B])
    a0 = s.L.pq_debug_alloc_count()
    s.result("x", device=True, instances=[B - 1, 0])
    assert s.L.pq_debug_alloc_count() == a0, "the device-memory result allocates nothing"


# ---- 8. refusals on a live handle
def test_refusals_on_a_live_handle_leave_it_as_it_was(hip):
    shape, kind = (4, 2, 3, 13), LLT
    qs, twin = solved_twin(hip, shape, kind)
    L = hip._lib.load()
    text = lambda: L.pq_last_error_string().decode()
    o = np.full(8, -7.0)
    c = np.zeros((3, 4))
    idx = lambda *v: np.array(v, dtype=np.intc)
    calls = lambda h, ix: {"pq_solver_batch_solve_select": lambda: L.pq_solver_batch_solve_select(h, ix.ctypes.data, len(ix)),
                           "pq_solver_batch_update_dense_select": lambda: L.pq_solver_batch_update_dense_select(h, ix.ctypes.data, len(ix), None, c.ctypes.data, *[None] * 7, 0, 1),
                           "pq_solver_batch_get_result_select_mem": lambda: L.pq_solver_batch_get_result_select_mem(h, ix.ctypes.data, len(ix), 0, o.ctypes.data, 0)}
    # a handle never set up
    fresh = hip.BatchDenseSolver()
    for fn, call in calls(fresh.h, idx(0, 1, 2)).items():
        assert call() == -1 and fn in text() and "not set up" in text()
    # a result before any solve
    s = handle(hip, qs, kind)
    s0 = handle(hip, feasible_batch(1, 0, 0, 6), kind)
    a0 = L.pq_debug_alloc_count()
    snap = record(hip, s)
    assert calls(s.h, idx(0, 1, 2))["pq_solver_batch_get_result_select_mem"]() == -1 and "no solve yet" in text()
    assert s.solve(instances=[12, 5]) == 2
    solved = record(hip, s)
    a1 = L.pq_debug_alloc_count()
    # an entry out of range, an instance listed twice
    for ix, words in ((idx(2, 13, 0), ("idx[1] = 13", "[0, 13)")), (idx(2, -1, 0), ("idx[1] = -1",)), (idx(4, 0, 4), ("idx[2] = 4", "listed twice", "idx[0]"))):
        for fn, call in calls(s.h, ix).items():
            if "listed twice" in words and fn == "pq_solver_batch_get_result_select_mem":
                continue  # (a result may repeat)
            assert call() == -1 and fn in text() and all(w in text() for w in words), (fn, text())
    with pytest.raises(RuntimeError, match="idx\\[1\\] = 13"):
        s.solve(instances=[2, 13])
    # the blocks the setup does not have
    buf = np.zeros(8)
    for k in (2, 3, 4, 5, 6):
        ptrs = [buf.ctypes.data if j == k else None for j in range(9)]
        assert L.pq_solver_batch_update_dense_select(s0.h, idx(0, 1).ctypes.data, 2, *ptrs, 0, 1) == -1 and "pq_solver_batch_update_dense_select" in text()
    assert o.tolist() == [-7.0] * 8 and L.pq_debug_alloc_count() == a1 and a1 == a0 + 1
    hold(record(hip, s), solved, [(i, i) for i in range(13)], "after the refusals", times=True)
    assert all(same(solved[i][k], snap[i][k]) for i in set(range(13)) - {12, 5} for k in snap[i])
    assert s.solve() == 13
    hold(record(hip, s), twin, [(i, i) for i in range(13)], "the whole solve after the refusals", times=False)


def test_settings_that_are_refused_mark_the_listed_infos_alone(hip):
    shape, kind = (4, 2, 3, 13), LLT
    qs, twin = solved_twin(hip, shape, kind)
    s = handle(hip, qs, kind)
    assert s.solve() == 13
    tau = s.settings.tau
    s.settings.tau = 2.0
    with pytest.raises(RuntimeError, match="invalid settings"):
        s.solve(instances=[3, 10])
    st = s.statuses()
    assert [st[3], st[10]] == [-10, -10] and all(st[i] == SOLVED for i in range(13) if i not in (3, 10))
    s.settings.tau = tau
    assert s.solve(instances=[10, 3]) == 2
    hold(record(hip, s), twin, [(i, i) for i in range(13)], "after the settings were put right", times=False)


# ---- 9. a clone taken after calls on lists
def test_a_clone_carries_the_mixed_state(hip):
    shape, kind = (31, 7, 5, 9), LLT
    qs = feasible_batch(*shape)
    s = handle(hip, qs, kind)
    assert s.solve(instances=[8, 1, 4]) == 3
    new = [update_args(qs, i, "all") for i in (4, 6)]
    assert s.update(**stack(new), instances=[4, 6]) is True
    assert s.solve(instances=[6]) == 1
    rec = record(hip, s)
    c = s.clone()
    hold(record(hip, c), rec, [(i, i) for i in range(9)], "clone()", times=True)
    part = [6, 0, 8, 4]
    hold(record(hip, s.clone(part)), rec, [(j, i) for j, i in enumerate(part)], "clone(instances)", times=True)
    assert c.solve() == s.solve()
    hold(record(hip, c), record(hip, s), [(i, i) for i in range(9)], "clone and source solved whole", times=False)
