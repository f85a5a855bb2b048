"""The batched DenseSolver (piqp_amd/csrc/dense_solver_batch.hip, pq_solver_batch_*, piqp_amd.BatchDenseSolver; n <= 128): every instance of a batch is compared
with its own CPU oracle, orc.Solver with the same settings and kkt_solver 0 or 16 (oracle/orc_solver.c), on the raw doubles.  There is no tolerance in this file and no
instance is left out: equality is same() of tests/test_dense_exact_gpu.py (the uint64 views).  Compared per instance: status, iter, every trace row, all ten result
vectors at full length, every non-time info field with n_factor and n_solve (n_backend_solve is this library's own counter, the oracle has none), and after setup the
scaled data and the scalings.  The oracle hands out its scaled data but not delta, delta_b and c of its preconditioner: ruiz_numpy (tests/batch_qp.py) is first held to
the oracle's scaled data bit for bit and the device's scalings are then compared with ruiz_numpy's.

Inputs: tests/batch_qp.py, feasible by construction.  What a test needs from the oracle (instances of one batch taking different numbers of iterations, a ladder that
is climbed, the exit statuses) is asserted on the oracle alone before the device is touched.  The oracle's run of a batch is computed once and shared."""
import numpy as np
import pytest

from batch_qp import feasible_batch, ruiz_numpy, stacked
from test_dense_exact_gpu import same

pytestmark = pytest.mark.gpu

LLT, LDLT = 0, 16
KINDS = [pytest.param(LLT, id="llt"), pytest.param(LDLT, id="ldlt")]
NAMES = ("x", "y", "z_l", "z_u", "z_bl", "z_bu", "s_l", "s_u", "s_bl", "s_bu")
SHAPES = [(1, 0, 0, 67), (4, 2, 3, 67), (31, 7, 5, 67), (32, 3, 5, 9), (33, 0, 300, 9), (64, 40, 257, 9), (128, 7, 5, 9)]
TIMES = ("setup_time", "update_time", "solve_time", "kkt_factor_time", "kkt_solve_time", "run_time")
SOLVED, MAX_ITER_REACHED, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE, NUMERICS, UNSOLVED, INVALID_SETTINGS = 1, -1, -2, -3, -8, -9, -10
TRACE_ROWS = 260  # more than max_iter + 1


def info_fields(hip):
    return [k for k, _ in hip._lib.Info._fields_ if k not in TIMES and k != "n_backend_solve"]


def oracle_run(orc, hip, qs, kind, states=False, **kw):
    """every instance through orc.Solver: what the device is compared with"""
    out = []
    for q in qs:
        s = orc.Solver()
        for k, v in kw.items():
            setattr(s.settings, k, v)
        s.settings.kkt_solver = kind
        s.enable_trace(TRACE_ROWS)
        assert s.setup(**q)
        d = s.data()
        scaled = {k: np.array(d.mat(k)) for k in ("P_utri", "AT", "GT")}
        scaled.update({k: np.array(d.vec(k)) for k in ("c", "b", "h_l", "h_u", "x_l", "x_u", "x_b_scaling")})
        rec = s.record_states() if states else None
        status = s.solve()
        out.append(dict(status=status, info={k: getattr(s.info, k) for k in info_fields(hip)}, trace=s.trace(), result=s.result(), scaled=scaled, states=rec, solver=s))
    return out


_oracle = {}


def oracle_of(orc, hip, n, p, m, batch, kind, pattern="random", **kw):
    key = (n, p, m, batch, kind, pattern, tuple(sorted(kw.items())))
    if key not in _oracle:
        qs = feasible_batch(n, p, m, batch, pattern)
        _oracle[key] = (qs, oracle_run(orc, hip, qs, kind, **kw))
    return _oracle[key]


def device(hip, qs, kind, trace=True, **kw):
    s = hip.BatchDenseSolver(kkt_solver=kind)
    for k, v in kw.items():
        setattr(s.settings, k, v)
    if trace:
        s.enable_trace(TRACE_ROWS)
    s.setup(**stacked(qs))
    return s


def check_solve(hip, s, ref, tag=""):
    """status, iter, info, trace and the ten result vectors of every instance against the oracle's"""
    res = {nm: s.result(nm) for nm in NAMES}
    for i, o in enumerate(ref):
        info = s.info(i)
        for k in info_fields(hip):
            assert same(getattr(info, k), o["info"][k]), f"{tag} instance {i}: info.{k} = {getattr(info, k)!r}, the oracle has {o['info'][k]!r}"
        assert info.status == o["status"]
        assert same(s.trace(i), o["trace"]), f"{tag} instance {i}: trace"
        for nm in NAMES:
            assert same(res[nm][i], o["result"][nm]), f"{tag} instance {i}: result {nm}"


def check_setup(orc, s, qs, ref, scale_cost=0, precond_iter=10):
    for i, (q, o) in enumerate(zip(qs, ref)):
        for k, v in o["scaled"].items():
            assert same(s.scaled_data(i, k), v), f"instance {i}: scaled {k}"
        od = orc.Data.dense(**q)
        scaled, (delta, delta_b, c_scale) = ruiz_numpy(od.mat("P_utri"), od.mat("AT"), od.mat("GT"), od.vec("c"), od.vec("x_b_scaling"), precond_iter, scale_cost)
        for k, v in zip(("P_utri", "AT", "GT", "c", "x_b_scaling"), scaled):
            assert same(v, o["scaled"][k]), f"instance {i}: the NumPy restatement of the equilibration misses the oracle's {k}"
        assert same(s.scaled_data(i, "delta"), delta) and same(s.scaled_data(i, "delta_b"), delta_b) and same(s.scaled_data(i, "c_scale"), c_scale), f"instance {i}: scalings"


# ---- 1. shapes: one wave per instance with a ragged last workgroup, both sides of n = 32, m beyond one K block, the full LDS square
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,p,m,batch", SHAPES, ids=lambda v: str(v))
def test_every_instance_is_the_oracle_at_every_launch_shape(orc, hip, n, p, m, batch, kind):
    qs, ref = oracle_of(orc, hip, n, p, m, batch, kind)
    assert all(o["status"] == SOLVED for o in ref)
    iters = {o["info"]["iter"] for o in ref}
    assert len(iters) >= 2, "the instances must not run in lock step: masked rounds have to occur"
    s = device(hip, qs, kind)
    check_setup(orc, s, qs, ref)
    assert s.solve() == batch
    check_solve(hip, s, ref)
    assert np.array_equal(s.statuses(), [o["status"] for o in ref]) and np.array_equal(s.iterations(), [o["info"]["iter"] for o in ref])
    ms = s.last_ms()
    assert 3 * max(iters) <= ms["rounds"] <= s.max_rounds()


# ---- 2. every exit, in one batch each
def nonconvex(n, p, m):
    qs = feasible_batch(n, p, m, 6, "no box")
    for i, shift in ((1, 0.7), (3, 3.0), (4, 30.0)):
        qs[i]["P"] = qs[i]["P"] - shift * np.eye(n)
    return qs


@pytest.mark.parametrize("variant", [dict(), dict(max_factor_retires=2), dict(iterative_refinement_always_enabled=1)], ids=["default", "two retries", "refinement always"])
@pytest.mark.parametrize("n,p,m", [(6, 2, 3), (33, 4, 6)], ids=str)
def test_the_retry_ladder_and_numerics(orc, hip, n, p, m, variant):
    qs = nonconvex(n, p, m)
    ref = oracle_run(orc, hip, qs, LLT, **variant)
    st = [o["status"] for o in ref]
    assert [st[i] for i in (0, 1, 2, 5)] == [SOLVED] * 4
    if "max_factor_retires" in variant:
        assert st[3] == st[4] == NUMERICS and ref[3]["info"]["iter"] == ref[4]["info"]["iter"] == 0
    else:
        assert any(o["info"]["n_factor"] > o["info"]["iter"] + 1 for o in ref), "no instance climbs the ladder"
        assert st[3] != SOLVED and st[4] != SOLVED
    s = device(hip, qs, LLT, **variant)
    assert s.solve() == st.count(SOLVED)
    check_solve(hip, s, ref)


def test_primal_infeasible_instance_among_solved_ones(orc, hip):
    qs = feasible_batch(4, 2, 3, 8)
    q = qs[1]
    assert np.isfinite(q["h_l"][0])
    q["G"], q["h_l"] = q["G"].copy(), q["h_l"].copy()
    q["G"][0] = q["A"][0]
    q["h_l"][0] = q["b"][0] + 100.0  # row 0 of G is row 0 of A: A_0 x = b_0 and A_0 x >= b_0 + 100
    ref = oracle_run(orc, hip, qs, LLT)
    assert [o["status"] for o in ref] == [SOLVED, PRIMAL_INFEASIBLE] + [SOLVED] * 6
    s = device(hip, qs, LLT)
    assert s.solve() == 7
    check_solve(hip, s, ref)


def test_dual_infeasible_instance_among_solved_ones(orc, hip):
    qs = feasible_batch(5, 0, 0, 6, "lower box")
    qs[2]["P"], qs[2]["c"] = np.zeros((5, 5)), -np.ones(5)
    ref = oracle_run(orc, hip, qs, LLT)
    assert [o["status"] for o in ref] == [SOLVED, SOLVED, DUAL_INFEASIBLE, SOLVED, SOLVED, SOLVED]
    s = device(hip, qs, LLT)
    assert s.solve() == 5
    check_solve(hip, s, ref)


def test_max_iter_reached(orc, hip):
    qs, ref = oracle_of(orc, hip, 4, 2, 3, 8, LLT, max_iter=3)
    assert all(o["status"] == MAX_ITER_REACHED and o["info"]["iter"] == 3 for o in ref)
    s = device(hip, qs, LLT, max_iter=3)
    assert s.solve() == 0
    check_solve(hip, s, ref)
    assert all(len(s.trace(i)) == len(o["trace"]) for i, o in enumerate(ref))


def test_invalid_settings_are_refused_without_a_launch(orc, hip):
    qs, ref = oracle_of(orc, hip, 4, 2, 3, 8, LLT, max_factor_retires=0)
    assert all(o["status"] == INVALID_SETTINGS for o in ref)
    s = device(hip, qs, LLT, max_factor_retires=0)
    assert s.L.pq_solver_batch_solve(s.h) == -1
    assert all(st == INVALID_SETTINGS for st in s.statuses())
    assert s.last_ms()["launches"] == 0
    s.settings.max_factor_retires = 10  # the handle goes on
    good = oracle_of(orc, hip, 4, 2, 3, 8, LLT)[1]
    assert s.solve() == 8
    check_solve(hip, s, good)


# ---- 3. settings
@pytest.mark.parametrize("variant", [dict(preconditioner_iter=0), dict(preconditioner_scale_cost=1), dict(check_duality_gap=0),
                                     dict(iterative_refinement_static_regularization_eps=1e-4)], ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()))
@pytest.mark.parametrize("n,p,m,batch", [(4, 2, 3, 67), (33, 0, 300, 9)], ids=lambda v: str(v))
def test_settings(orc, hip, n, p, m, batch, variant):
    qs, ref = oracle_of(orc, hip, n, p, m, batch, LLT, **variant)
    s = device(hip, qs, LLT, **variant)
    check_setup(orc, s, qs, ref, scale_cost=variant.get("preconditioner_scale_cost", 0), precond_iter=variant.get("preconditioner_iter", 10))
    assert s.solve() == sum(o["status"] == SOLVED for o in ref)
    check_solve(hip, s, ref)


# ---- 4. handle behaviour
def test_solve_twice_setup_again_and_no_allocation(orc, hip):
    qs, ref = oracle_of(orc, hip, 31, 7, 5, 67, LLT)
    s = device(hip, qs, LLT)
    a0 = s.L.pq_debug_alloc_count()
    assert s.solve() == 67
    first = {nm: s.result(nm) for nm in NAMES}
    assert s.solve() == 67
    check_solve(hip, s, ref, "second solve")
    assert all(same(first[nm], s.result(nm)) for nm in NAMES)
    dev = {nm: s.result(nm, device=True) for nm in NAMES}
    assert s.L.pq_debug_alloc_count() == a0, "solve and the result calls must not allocate"
    assert all(same(dev[nm].cpu().numpy(), first[nm]) for nm in NAMES)
    qs2, ref2 = oracle_of(orc, hip, 4, 2, 3, 8, LLT)  # other data, another shape, on the same handle
    s.setup(**stacked(qs2))
    assert s.solve() == 8
    check_solve(hip, s, ref2, "second setup")


def test_batch_of_one(orc, hip):
    qs, ref = oracle_of(orc, hip, 33, 4, 6, 1, LDLT)
    s = device(hip, qs, LDLT)
    assert s.solve() == 1
    check_solve(hip, s, ref)


@pytest.mark.parametrize("order", ["row-major", "column-major", "mixed with numpy"])
def test_torch_inputs_give_the_bits_of_the_host_fed_handle(orc, hip, order):
    import torch
    qs, ref = oracle_of(orc, hip, 32, 3, 5, 9, LLT)
    a = stacked(qs)
    t = {k: (None if v is None else torch.as_tensor(v).cuda()) for k, v in a.items()}
    if order == "column-major":
        for k in ("P", "A", "G"):
            t[k] = t[k].transpose(1, 2).contiguous().transpose(1, 2)
            assert not t[k].is_contiguous()
    elif order == "mixed with numpy":
        t["G"], t["c"] = a["G"], a["c"]
    s = hip.BatchDenseSolver(kkt_solver=LLT)
    s.enable_trace(TRACE_ROWS)
    s.setup(**t)
    check_setup(orc, s, qs, ref)
    assert s.solve() == 9
    check_solve(hip, s, ref)


def test_a_differing_bound_pattern_is_refused(hip):
    qs = feasible_batch(4, 2, 3, 8)
    assert np.isfinite(qs[3]["h_l"][0])
    qs[3]["h_l"] = qs[3]["h_l"].copy()
    qs[3]["h_l"][0] = -np.inf
    s = hip.BatchDenseSolver()
    with pytest.raises(RuntimeError, match="finite bounds"):
        s.setup(**stacked(qs))


def test_rows_without_a_finite_bound_are_dropped_as_the_oracle_drops_them(orc, hip):
    qs = feasible_batch(4, 2, 3, 8)
    for q in qs:
        q["h_l"], q["h_u"] = q["h_l"].copy(), q["h_u"].copy()
        q["h_l"][1], q["h_u"][1] = -np.inf, np.inf
    ref = oracle_run(orc, hip, qs, LLT)
    assert all(not o["scaled"]["GT"][:, 1].any() for o in ref)
    s = device(hip, qs, LLT)
    check_setup(orc, s, qs, ref)
    assert s.solve() == sum(o["status"] == SOLVED for o in ref)
    check_solve(hip, s, ref)


# ---- 5. the layers below: the borrowed KKT system is in the state the last factorisation of each instance left
@pytest.mark.parametrize("n,p,m,batch", [(4, 2, 3, 67), (33, 0, 300, 9)], ids=lambda v: str(v))
def test_the_borrowed_kkt_system_holds_each_instances_last_factorisation(orc, hip, n, p, m, batch):
    qs = feasible_batch(n, p, m, batch)
    ref = oracle_run(orc, hip, qs, LLT, states=True)
    s = device(hip, qs, LLT)
    assert s.solve() == batch
    ks = s.kktsys()
    if (n, p, m, batch) == (4, 2, 3, 67):  # the borrowed system knows its dimensions but not the bound lists: calls that take variables say so, before any launch
        assert ks.batch == batch
        with pytest.raises(RuntimeError):
            ks.solve({})
    x_reg, z_reg = ks.x_reg(), ks.z_reg()
    for i, o in enumerate(ref):
        last = [st for st in o["states"] if st["kind"] == 0][-1]
        ko = orc.KKTSystem(o["solver"].data(), orc.Settings(kkt_solver=LLT))
        assert ko.update_scalings_and_factor(last["refine"], last["rho"], last["delta"], last["vars"])
        assert same(x_reg[i], ko.x_reg()) and same(z_reg[i], ko.z_reg()), f"instance {i}"


# ---- the boundary shift (solver.hpp:616-640): a bound a billion away makes its multiplier fall below machine epsilon while the instance still iterates
def far_bounds(kind):
    if kind == "rows":
        qs = feasible_batch(4, 2, 3, 8)
        assert np.isfinite(qs[0]["h_l"][0])
        for q in qs[::2]:
            q["h_l"] = q["h_l"].copy()
            q["h_l"][0] -= 1e9
    else:
        qs = feasible_batch(5, 0, 0, 6, "lower box")
        for q in qs[1::2]:
            q["x_l"] = q["x_l"].copy()
            q["x_l"][0] -= 1e9
    return qs


@pytest.mark.parametrize("kind", ["rows", "box"])
def test_the_boundary_shift(orc, hip, kind):
    """(a copy of the oracle without the shift of z_l gives other bits on instances 0, 2, 4 and 6 of "rows": checked when this test was written)"""
    qs = far_bounds(kind)
    ref = oracle_run(orc, hip, qs, LLT)
    assert all(o["status"] == SOLVED for o in ref)
    far = [o["info"]["iter"] for o in (ref[::2] if kind == "rows" else ref[1::2])]
    near = [o["info"]["iter"] for o in (ref[1::2] if kind == "rows" else ref[::2])]
    assert min(far) > max(near) + 3, "the far bound is to keep its instance iterating while its multiplier vanishes"
    s = device(hip, qs, LLT)
    assert s.solve() == len(qs)
    check_solve(hip, s, ref)
