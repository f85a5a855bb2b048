"""BatchDenseSolver.update (pq_solver_batch_update_dense, piqp_amd/csrc/dense_solver_batch.hip): every instance of a batch has its own CPU oracle, orc.Solver, that
gets the same setup, solve and update calls.  There is no tolerance in this file and no instance is left out: equality is same() of tests/test_dense_exact_gpu.py.
After every update the 13 items of scaled_data are compared, after every solve status, iter, every info field, every trace row and the ten vectors (check_solve of
tests/test_dense_solver_batch_gpu.py).  The assembled KKT matrix is not compared on its own: after an update that leaves A'A alone the oracle's A'A is that of an
earlier A', which no fresh orc.KKTSystem reproduces; the trace covers it (a wrong A'A changes the first factorisation).

The oracle hands out its scaled data but not its scalings.  A Twin carries a NumPy restatement of unscale_data, the assignment and scale_data beside each oracle
(ruiz_numpy of tests/batch_qp.py for the equilibration); after the setup and after every update it is first held to the oracle's scaled P, A', G', c and x_b_scaling bit
for bit, and delta, delta_b and c of the device are then compared with its own.

Where the library recomputes A'A and the reference would not (P or G without A, p > 0, preconditioner_reuse_on_update = 0: include/piqp_amd.h says why), the oracle
gets A = its own unscaled A beside the other arguments, which leaves its data as they are and makes it recompute A'A; that its scaled data are bitwise the same with
and without that argument is asserted first, on two oracle solvers alone.  What a test needs from the oracle (every instance SOLVED, at least two iteration counts in
a batch, lists that stay the setup's) is asserted before the device is touched."""
import numpy as np
import pytest

from batch_qp import KEYS, feasible_batch, ruiz_numpy, stacked
from test_dense_exact_gpu import same
from test_dense_solver_batch_gpu import LDLT, LLT, MAX_ITER_REACHED, NAMES, SOLVED, TRACE_ROWS, check_solve, info_fields

pytestmark = pytest.mark.gpu

SCALED = ("P_utri", "AT", "GT", "c", "b", "h_l", "h_u", "x_l", "x_u", "x_b_scaling")
SHAPES = [(1, 0, 0, 5), (4, 2, 3, 67), (31, 7, 5, 9), (33, 0, 300, 3), (64, 40, 257, 3), (128, 7, 5, 3)]
SETS = ("c", "vectors", "P", "A,b", "G,h", "all", "chain")


# ---- the update sets: instance i takes data from its neighbour (the same bound pattern, feasible by construction)
def update_args(qs, i, name):
    q, nb = qs[i], qs[(i + 1) % len(qs)]
    n = len(q["c"])
    r = np.random.default_rng(424242 + i)
    d = 0.01 * r.standard_normal(n)
    if name == "c":
        return dict(c=nb["c"])
    if name == "vectors":
        a = dict(c=q["c"] + 0.1 * r.standard_normal(n))
        if "A" in q:
            a["b"] = q["b"] + q["A"] @ d
        if "G" in q:
            a["h_l"], a["h_u"] = q["h_l"] + q["G"] @ d - 0.25, q["h_u"] + q["G"] @ d + 0.25
        a["x_l"], a["x_u"] = q["x_l"] + d - 0.25, q["x_u"] + d + 0.25
        return a
    if name == "P":
        return dict(P=nb["P"])
    if name == "A,b":
        S = r.uniform(0.5, 2, len(q["b"]))
        return dict(A=S[:, None] * q["A"], b=S * q["b"])
    if name == "G,h":
        S = r.uniform(0.5, 2, len(q["h_l"]))
        return dict(G=S[:, None] * q["G"], h_l=S * q["h_l"], h_u=S * q["h_u"])
    assert name == "all"
    return {k: nb[k] for k in KEYS if k in nb}


def steps_of(name):
    return ("vectors", "all", "c") if name == "chain" else (name,)


def stack(per_instance):
    return {k: np.stack([a[k] for a in per_instance]) for k in per_instance[0]}


# ---- one oracle and the NumPy restatement of its preconditioner
class Twin:
    def __init__(self, orc, hip, q, kind, settings):
        self.hip = hip
        self.s = orc.Solver()
        for k, v in settings.items():
            setattr(self.s.settings, k, v)
        self.s.settings.kkt_solver = kind
        self.s.enable_trace(TRACE_ROWS)
        assert self.s.setup(**q)
        self.iter, self.cost = self.s.settings.preconditioner_iter, self.s.settings.preconditioner_scale_cost
        self.reuse = self.s.settings.preconditioner_reuse_on_update
        od = orc.Data.dense(**q)
        self.lists = [od.idx(k).tolist() for k in ("h_l", "h_u", "x_l", "x_u")]
        self.data, self.scal = ruiz_numpy(od.mat("P_utri"), od.mat("AT"), od.mat("GT"), od.vec("c"), od.vec("x_b_scaling"), self.iter, self.cost)
        self.hold("setup")

    def oracle_scaled(self, s=None):
        d = (s or self.s).data()
        out = {k: np.array(d.mat(k)) for k in ("P_utri", "AT", "GT")}
        out.update({k: np.array(d.vec(k)) for k in SCALED[3:]})
        return out

    def hold(self, tag):
        o = self.oracle_scaled()
        for k, v in zip(("P_utri", "AT", "GT", "c", "x_b_scaling"), self.data):
            assert same(v, o[k]), f"{tag}: the NumPy restatement of the preconditioner misses the oracle's {k}"
        d = self.s.data()
        assert [d.idx(k).tolist() for k in ("h_l", "h_u", "x_l", "x_u")] == self.lists, f"{tag}: the oracle's lists are no longer the setup's"

    def unscaled(self):
        """orc_solver.c:243-251 on the restatement's copy"""
        P, AT, GT, c, xbs = self.data
        delta, delta_b, rc = self.scal
        n, p = P.shape[0], AT.shape[1]
        di, dib, ci = 1.0 / delta, 1.0 / delta_b, 1.0 / rc[0]
        iu = np.triu(np.ones((n, n), dtype=bool))
        P = np.where(iu, ((P * ci) * di[None, :n]) * di[:n, None], P)
        return P, (di[:n, None] * AT) * di[None, n:n + p], (di[:n, None] * GT) * di[None, n + p:], c * (ci * di[:n]), xbs * (dib * di[:n])

    def update(self, args, trap):
        """the same update on the oracle and on the restatement; trap: the oracle gets its own unscaled A too, so that it recomputes A'A"""
        P, AT, GT, c, xbs = self.unscaled()
        if trap:
            A_un = np.ascontiguousarray(AT.T)
            plain = self.s.clone()
            assert plain.update(**args) and self.s.update(A=A_un, **args)
            a, b = self.oracle_scaled(plain), self.oracle_scaled()
            assert all(same(a[k], b[k]) for k in SCALED), "the oracle's scaled data differ with and without its own unscaled A"
        else:
            assert self.s.update(**args)
        n, p = P.shape[0], AT.shape[1]
        if "P" in args:
            P = np.triu(args["P"])
        if "A" in args:
            AT = np.array(args["A"].T)
        if "G" in args:
            GT = np.array(args["G"].T)
        if "c" in args:
            c = np.array(args["c"])
        if self.reuse or not any(k in args for k in ("P", "A", "G")):  # :229-235
            delta, delta_b, rc = self.scal
            iu = np.triu(np.ones((n, n), dtype=bool))
            P = np.where(iu, ((P * rc[0]) * delta[None, :n]) * delta[:n, None], P)
            self.data = (P, (delta[:n, None] * AT) * delta[None, n:n + p], (delta[:n, None] * GT) * delta[None, n + p:], c * (rc[0] * delta[:n]), xbs * (delta_b * delta[:n]))
        else:
            self.data, self.scal = ruiz_numpy(P, AT, GT, c, xbs, self.iter, self.cost)
        self.hold(f"update({', '.join(args)})")

    def expected_scaled(self):
        out = self.oracle_scaled()
        out.update(delta=self.scal[0].copy(), delta_b=self.scal[1].copy(), c_scale=self.scal[2].copy())
        return out

    def solve(self):
        self.s.enable_trace(TRACE_ROWS)  # (the oracle's table goes on where the last solve ended; the handle's starts at row 0 with every solve)
        status = self.s.solve()
        return dict(status=status, info={k: getattr(self.s.info, k) for k in info_fields(self.hip)}, trace=self.s.trace(), result=self.s.result())


def is_trap(args, p, reuse):
    return p > 0 and not reuse and "A" not in args and any(k in args for k in ("P", "G"))


def oracle_sequence(orc, hip, qs, kind, settings, sequence):
    """sequence: per step None (a solve) or a list of per-instance argument dicts (an update).  Returns the twins and per step the list of what the device must show"""
    p = qs[0]["A"].shape[0] if "A" in qs[0] else 0
    twins = [Twin(orc, hip, q, kind, settings) for q in qs]
    reuse = twins[0].reuse
    out = [[t.expected_scaled() for t in twins]]
    for step in sequence:
        if step is None:
            out.append([t.solve() for t in twins])
        else:
            for t, a in zip(twins, step):
                t.update(a, is_trap(a, p, reuse))
            out.append([t.expected_scaled() for t in twins])
    return twins, out


def check_scaled(s, exp, tag):
    for i, e in enumerate(exp):
        for k, v in e.items():
            assert same(s.scaled_data(i, k), v), f"{tag} instance {i}: scaled {k}"


def new_handle(hip, qs, kind, settings):
    s = hip.BatchDenseSolver(kkt_solver=kind)
    for k, v in settings.items():
        setattr(s.settings, k, v)
    s.enable_trace(TRACE_ROWS)
    s.setup(**stacked(qs))
    return s


def to_torch(a, order):
    import torch
    t = {k: torch.as_tensor(v).cuda() for k, v in a.items()}
    if order == "column-major":
        for k in ("P", "A", "G"):
            if k in t:
                t[k] = t[k].transpose(1, 2).contiguous().transpose(1, 2)
    return t


def device_sequence(hip, s, sequence, exp, feed="numpy"):
    """the same calls on the handle, compared step by step with exp[1:]"""
    for k, (step, e) in enumerate(zip(sequence, exp[1:])):
        if step is None:
            assert s.solve() == sum(o["status"] == SOLVED for o in e)
            check_solve(hip, s, e, f"step {k}")
        else:
            a = stack(step) if step[0] else {}
            assert s.update(**(a if feed == "numpy" else to_torch(a, feed))) is True
            check_scaled(s, e, f"step {k}")


def sequence_of(qs, name):
    seq = [None]  # the oracle and the handle both solve once before the first update
    for st in steps_of(name):
        seq += [[update_args(qs, i, st) for i in range(len(qs))], None]
    return seq


# ---- 1. every set at every shape, both values of preconditioner_reuse_on_update, both factorisations
def cases():
    out = []
    for n, p, m, batch in SHAPES:
        for name in SETS:
            if (name == "A,b" and p == 0) or (name == "G,h" and m == 0):
                continue
            for reuse in (0, 1):
                for kind, kid in ((LLT, "llt"), (LDLT, "ldlt")):
                    out.append(pytest.param(n, p, m, batch, name, reuse, kind, id=f"({n}, {p}, {m}, {batch})-{name}-reuse={reuse}-{kid}"))
    return out


@pytest.mark.parametrize("n,p,m,batch,name,reuse,kind", cases())
def test_update_is_the_oracles_update(orc, hip, n, p, m, batch, name, reuse, kind):
    qs = feasible_batch(n, p, m, batch)
    settings = dict(preconditioner_reuse_on_update=reuse)
    seq = sequence_of(qs, name)
    _, exp = oracle_sequence(orc, hip, qs, kind, settings, seq)
    solves = [e for step, e in zip(seq, exp[1:]) if step is None]
    assert all(o["status"] == SOLVED for e in solves for o in e)
    # (per solve this holds everywhere but after "vectors" at (128, 7, 5, 3), where the three instances all take 8 iterations; the solve before it takes 8, 10, 8)
    assert any(len({o["info"]["iter"] for o in e}) >= 2 for e in solves), "the instances must not run in lock step: masked rounds have to occur"
    s = new_handle(hip, qs, kind, settings)
    check_scaled(s, exp[0], "setup")
    device_sequence(hip, s, seq, exp)


# ---- 2. settings: the c_inv / rc factors of scale_cost, scalings that are all ones
@pytest.mark.parametrize("name", ["all", "c"])
@pytest.mark.parametrize("variant", [dict(preconditioner_scale_cost=1), dict(preconditioner_iter=0)], ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()))
def test_update_under_preconditioner_settings(orc, hip, variant, name):
    qs = feasible_batch(4, 2, 3, 67)
    seq = sequence_of(qs, name)
    twins, exp = oracle_sequence(orc, hip, qs, LLT, variant, seq)
    if "preconditioner_scale_cost" in variant:
        assert any(t.scal[2][0] != 1.0 for t in twins), "no instance has a cost scaling"
    else:
        assert all((t.scal[0] == 1.0).all() and (t.scal[1] == 1.0).all() for t in twins)
    s = new_handle(hip, qs, LLT, variant)
    check_scaled(s, exp[0], "setup")
    device_sequence(hip, s, seq, exp)


# ---- 3. a row dropped at setup
def dropped_row_batch():
    qs = feasible_batch(4, 0, 3, 8)
    for q in qs:
        q["h_l"], q["h_u"] = q["h_l"].copy(), q["h_u"].copy()
        q["h_l"][0], q["h_u"][0] = -np.inf, np.inf
    return qs


def test_a_dropped_row_through_updates_and_the_refusals(orc, hip):
    qs = dropped_row_batch()
    B = len(qs)
    nb = lambda i: qs[(i + 1) % B]
    seq = [None,
           [dict(c=nb(i)["c"]) for i in range(B)], None,
           [dict(h_l=q["h_l"] - 0.25, h_u=q["h_u"] + 0.25) for q in qs], None,  # row 0 is infinite again on both sides
           [dict(G=nb(i)["G"]) for i in range(B)], None]
    twins, exp = oracle_sequence(orc, hip, qs, LLT, {}, seq)  # (every Twin.hold asserts that the oracle's lists stay the setup's)
    assert all(not e["GT"][:, 0].any() for e in exp[4]) and all(e["GT"][:, 0].any() for e in exp[6]), "column 0 of G' is zero until G comes alone"
    assert all(same(e["h_l"][0], -e["delta"][4]) and same(e["h_u"][0], e["delta"][4]) for e in exp[4]), "reset to exactly -1 / 1 before scaling (n + p = 4)"
    assert {o["status"] for o in exp[7]} <= {SOLVED, MAX_ITER_REACHED}
    s = new_handle(hip, qs, LLT, {})
    device_sequence(hip, s, seq, exp)
    # refused, from the host path and from the torch path: -inf on the dropped row with h_u absent (its stored 1 is finite), a finite box bound turned infinite
    import torch
    j = int(np.flatnonzero(np.isfinite(qs[0]["x_l"]))[0])
    h_l = np.stack([q["h_l"] for q in qs])
    x_l = np.stack([q["x_l"] for q in qs])
    x_l[B - 1, j] = -np.inf
    for bad in (dict(h_l=h_l), dict(x_l=x_l)):
        for feed in (lambda v: v, lambda v: torch.as_tensor(v).cuda()):
            with pytest.raises(RuntimeError, match="finite bounds"):
                s.update(**{k: feed(v) for k, v in bad.items()})
            check_scaled(s, exp[6], "after a refused update")
    last = [t.solve() for t in twins]  # the oracle that did not get those calls
    assert s.solve() == sum(o["status"] == SOLVED for o in last)
    check_solve(hip, s, last, "after the refusals")


# ---- 4. the handle
def test_no_allocation_no_argument_and_setup_again(orc, hip):
    qs = feasible_batch(4, 2, 3, 67)
    B = len(qs)
    seq = [None, [update_args(qs, i, "vectors") for i in range(B)], None, [{} for _ in range(B)], None, [update_args(qs, i, "all") for i in range(B)], None]
    _, exp = oracle_sequence(orc, hip, qs, LLT, {}, seq)
    s = new_handle(hip, qs, LLT, {})
    a0 = s.L.pq_debug_alloc_count()
    device_sequence(hip, s, seq, exp)
    assert s.L.pq_debug_alloc_count() == a0, "update and solve must not allocate"
    i0 = s.info(0)
    assert i0.update_time > 0 and i0.run_time == i0.update_time + i0.solve_time
    ms = s.last_update_ms()
    assert 0 < ms["device_ms"] and 0 < ms["wall_ms"] and same(i0.update_time, ms["wall_ms"] * 1e-3)
    # a setup after updates behaves as a first setup
    qs2 = feasible_batch(31, 7, 5, 9)
    _, exp2 = oracle_sequence(orc, hip, qs2, LLT, {}, [None])
    s.setup(**stacked(qs2))
    check_scaled(s, exp2[0], "second setup")
    assert s.solve() == 9
    check_solve(hip, s, exp2[1], "second setup")
    assert s.info(0).run_time == s.info(0).setup_time + s.info(0).solve_time


def test_update_before_setup_and_absent_blocks_are_refused(hip):
    s = hip.BatchDenseSolver()
    with pytest.raises(RuntimeError):
        s.update(c=np.zeros((3, 4)))
    qs = feasible_batch(1, 0, 0, 5)
    s.setup(**stacked(qs))
    buf = np.zeros(64)
    for k in (2, 3, 4, 5, 6):  # A, b, G, h_l, h_u at the C level: p = m = 0
        ptrs = [buf.ctypes.data if j == k else None for j in range(9)]
        assert s.L.pq_solver_batch_update_dense(s.h, *ptrs, 0, 1) == -1


@pytest.mark.parametrize("order", ["row-major", "column-major"])
@pytest.mark.parametrize("name", ["vectors", "all"])
def test_torch_inputs_give_the_bits_of_the_host_fed_handle(orc, hip, name, order):
    qs = feasible_batch(4, 2, 3, 67)
    seq = sequence_of(qs, name)
    _, exp = oracle_sequence(orc, hip, qs, LLT, {}, seq)
    host = new_handle(hip, qs, LLT, {})
    device_sequence(hip, host, seq, exp)
    s = new_handle(hip, qs, LLT, {})
    a0 = s.L.pq_debug_alloc_count()
    device_sequence(hip, s, seq, exp, feed=order)
    assert s.L.pq_debug_alloc_count() == a0
    for k in SCALED + ("delta", "delta_b", "c_scale"):
        assert all(same(s.scaled_data(i, k), host.scaled_data(i, k)) for i in range(len(qs)))
    assert all(same(s.result(nm), host.result(nm)) for nm in NAMES)
