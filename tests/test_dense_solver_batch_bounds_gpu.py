"""The batched DenseSolver with a set of finite bounds per instance (BatchDenseSolver(bounds="per_instance"), pq_solver_batch_set_bound_sets,
piqp_amd/csrc/dense_solver_batch.hip): every instance of a batch of tests/batch_qp_mixed.py is compared with its own CPU oracle, orc.Solver taken through the same
setup, solve and update calls, on the raw doubles.  There is no tolerance in this file, and no instance of a batch is left out but in test 7, which builds its
batch from the instances the library's rule on stored infinite bounds does not touch and says which (on the others the library and the reference differ by rule;
tests/test_dense_solver_batch_bounds_abi.py asserts there what the reference does): equality is same() of
tests/test_dense_exact_gpu.py; check_setup and check_solve are those of tests/test_dense_solver_batch_gpu.py (scaled data and scalings; status, iter, every info
field, every trace row, the ten vectors at full length).

Shapes, the smallest that reach each branch: (1, 0, 0, 9) counts 0 / 1; (4, 2, 3, 67) several instances with different counts in one workgroup of the factor launch and
a ragged last workgroup (both factorisations); (33, 0, 300, 9) n past 32, m past one K block, dropped rows in a wide G; (128, 7, 5, 9) the full LDS square.

Tests: 1 setup and solve; 2 a shared pattern through a per-instance handle; 3 an update that changes the sets (A, G and the four bound vectors); 4 the bound vectors
alone; 5 torch CUDA inputs; 6 the mode belongs to the setup; 7 one bound vector alone.

What a test needs from the oracle is asserted on the oracle before the device is touched; the oracle's runs are computed once and shared."""
import numpy as np
import pytest

from batch_qp import stacked
from batch_qp_mixed import hinges_on_a_rounding, mixed_batch, oracle_of_mixed
from test_dense_exact_gpu import same
from test_dense_solver_batch_gpu import LDLT, LLT, MAX_ITER_REACHED, NAMES, PRIMAL_INFEASIBLE, SOLVED, TRACE_ROWS, check_setup, check_solve, info_fields, oracle_of

pytestmark = pytest.mark.gpu

CASES = [pytest.param(1, 0, 0, 9, LLT, id="(1, 0, 0, 9)-llt"), pytest.param(4, 2, 3, 67, LLT, id="(4, 2, 3, 67)-llt"), pytest.param(4, 2, 3, 67, LDLT, id="(4, 2, 3, 67)-ldlt"),
         pytest.param(33, 0, 300, 9, LLT, id="(33, 0, 300, 9)-llt"), pytest.param(128, 7, 5, 9, LLT, id="(128, 7, 5, 9)-llt")]
SCALED = ("P_utri", "AT", "GT", "c", "b", "h_l", "h_u", "x_b_scaling")
LISTS = ("h_l", "h_u", "x_l", "x_u")
BOUNDS = ("h_l", "h_u", "x_l", "x_u")


def device(hip, qs, kind, bounds="per_instance"):
    s = hip.BatchDenseSolver(kkt_solver=kind, bounds=bounds)
    s.enable_trace(TRACE_ROWS)
    s.setup(**stacked(qs))
    return s


# ---- 1. setup and solve
@pytest.mark.parametrize("n,p,m,batch,kind", CASES)
def test_setup_and_solve_of_a_mixed_batch(orc, hip, n, p, m, batch, kind):
    qs, ref = oracle_of_mixed(orc, hip, n, p, m, batch, kind)
    assert all(o["status"] == SOLVED for o in ref)
    assert len({o["info"]["iter"] for o in ref}) >= 2, "the instances must not run in lock step: masked rounds have to occur"
    assert len({orc.Data.dense(**q).counts() for q in qs}) >= 3, "the instances must hold different sets"
    s = device(hip, qs, kind)
    check_setup(orc, s, qs, ref)
    assert s.solve() == batch
    check_solve(hip, s, ref)


# ---- 2. a batch that does share its pattern
@pytest.mark.parametrize("n,p,m,batch", [(4, 2, 3, 67), (33, 0, 300, 9)], ids=str)
def test_a_shared_pattern_through_a_per_instance_handle(orc, hip, n, p, m, batch):
    qs, ref = oracle_of(orc, hip, n, p, m, batch, LLT)
    one, own = device(hip, qs, LLT, "shared"), device(hip, qs, LLT)
    check_setup(orc, own, qs, ref)
    assert one.solve() == own.solve() == sum(o["status"] == SOLVED for o in ref)
    check_solve(hip, own, ref)
    assert all(same(own.result(nm), one.result(nm)) for nm in NAMES)
    assert all(same(own.trace(i), one.trace(i)) for i in range(batch))


# ---- 3., 4. an update that changes the sets
def update_of(q1, names):
    return {k: q1[k] for k in names if k in q1}


_chains = {}


def oracle_chain(orc, hip, n, p, m, batch, kind, names, keep=None):
    """every instance (keep: only those) through setup(salt 0), solve, update(the arguments `names` of salt 1), solve: per instance the two solves, the counts and
    lists before and after the update and the scaled data after it"""
    key = (n, p, m, batch, kind, names, keep)
    if key in _chains:
        return _chains[key]
    out = []
    for i, (q, q1) in enumerate(zip(mixed_batch(n, p, m, batch), mixed_batch(n, p, m, batch, salt=1))):
        if keep is not None and i not in keep:
            continue
        s = orc.Solver()
        s.settings.kkt_solver = kind
        rec = {}
        for step in ("first", "second"):
            if step == "first":
                assert s.setup(**q)
                rec["counts0"] = s.data().counts()
            else:
                assert s.update(**update_of(q1, names))
                d = s.data()
                rec["counts1"] = d.counts()
                rec["lists1"] = [d.idx(k).tolist() for k in LISTS]
                rec["scaled"] = {k: np.array(d.mat(k)) for k in SCALED[:3]}
                rec["scaled"].update({k: np.array(d.vec(k)) for k in SCALED[3:] + ("x_l", "x_u")})
            s.enable_trace(TRACE_ROWS)  # (the oracle's table goes on where the last solve ended; the handle's starts at row 0 with every solve)
            status = s.solve()
            rec[step] = dict(status=status, info={k: getattr(s.info, k) for k in info_fields(hip)}, trace=s.trace(), result=s.result())
        out.append(rec)
    _chains[key] = out
    return out


def check_updated(s, chain):
    """the scaled data after the update; of the packed box vectors what the instance's own count covers (the rest is unspecified)"""
    for i, rec in enumerate(chain):
        for k in SCALED:
            assert same(s.scaled_data(i, k), rec["scaled"][k]), f"instance {i}: scaled {k} after the update"
        for k, c in (("x_l", rec["counts1"][2]), ("x_u", rec["counts1"][3])):
            assert same(s.scaled_data(i, k)[:c], rec["scaled"][k][:c]), f"instance {i}: scaled {k} after the update"


def run_chain(hip, s, chain, args, feed=lambda v: v):
    batch = len(chain)
    assert s.solve() == sum(rec["first"]["status"] == SOLVED for rec in chain)
    check_solve(hip, s, [rec["first"] for rec in chain], "before the update")
    a0 = s.L.pq_debug_alloc_count()
    assert s.update(**{k: feed(v) for k, v in args.items() if v is not None}) is True
    assert s.solve() == sum(rec["second"]["status"] == SOLVED for rec in chain)
    live = [nm for nm in NAMES if chain[0]["second"]["result"][nm].size]  # (an empty vector has no device pointer to hand over)
    dev = {nm: s.result(nm, device=True) for nm in live}
    assert s.L.pq_debug_alloc_count() == a0, "update, solve and the result calls must not allocate"
    check_updated(s, chain)
    check_solve(hip, s, [rec["second"] for rec in chain], "after the update")
    assert all(same(dev[nm].cpu().numpy(), s.result(nm)) for nm in live) and len(chain) == batch


WITH_MATRICES = ("A", "G") + BOUNDS  # A because of the A'A rule of include/piqp_amd.h: with G alone and new scalings the library recomputes A'A and the reference does not


@pytest.mark.parametrize("n,p,m,batch,kind,least", [pytest.param(4, 2, 3, 67, LLT, 65, id="(4, 2, 3, 67)-llt"), pytest.param(4, 2, 3, 67, LDLT, 65, id="(4, 2, 3, 67)-ldlt"),
                                                    pytest.param(33, 0, 300, 9, LLT, 9, id="(33, 0, 300, 9)-llt")])
def test_an_update_that_changes_the_sets(orc, hip, n, p, m, batch, kind, least):
    chain = oracle_chain(orc, hip, n, p, m, batch, kind, WITH_MATRICES)
    assert sum(rec["counts0"] != rec["counts1"] for rec in chain) >= least, "the update is to change the sets"
    assert all(rec[k]["status"] == SOLVED for rec in chain for k in ("first", "second"))
    s = device(hip, mixed_batch(n, p, m, batch), kind)
    run_chain(hip, s, chain, update_of(stacked(mixed_batch(n, p, m, batch, salt=1)), WITH_MATRICES))


def test_an_update_of_the_bounds_alone(orc, hip):
    """rows that come back without a new G keep their zero row, as in the reference: some instances are then infeasible or run to the iteration limit"""
    n, p, m, batch = 4, 2, 3, 67
    chain = oracle_chain(orc, hip, n, p, m, batch, LLT, BOUNDS)
    after = [rec["second"]["status"] for rec in chain]
    assert SOLVED in after and (PRIMAL_INFEASIBLE in after or MAX_ITER_REACHED in after), after
    assert all(rec["first"]["status"] == SOLVED for rec in chain)
    s = device(hip, mixed_batch(n, p, m, batch), LLT)
    run_chain(hip, s, chain, update_of(stacked(mixed_batch(n, p, m, batch, salt=1)), BOUNDS))
    assert np.array_equal(s.statuses(), after)


# ---- 5. torch CUDA inputs
def test_torch_inputs_give_the_bits_of_the_host_fed_handle(orc, hip):
    import torch
    n, p, m, batch = 4, 2, 3, 67
    qs, ref = oracle_of_mixed(orc, hip, n, p, m, batch, LLT)
    chain = oracle_chain(orc, hip, n, p, m, batch, LLT, WITH_MATRICES)
    args = update_of(stacked(mixed_batch(n, p, m, batch, salt=1)), WITH_MATRICES)
    host = device(hip, qs, LLT)
    run_chain(hip, host, chain, args)
    s = hip.BatchDenseSolver(kkt_solver=LLT, bounds="per_instance")
    s.enable_trace(TRACE_ROWS)
    s.setup(**{k: (None if v is None else torch.as_tensor(v).cuda()) for k, v in stacked(qs).items()})
    check_setup(orc, s, qs, ref)
    run_chain(hip, s, chain, args, feed=lambda v: torch.as_tensor(v).cuda())
    for k in SCALED + ("delta", "delta_b", "c_scale"):
        assert all(same(s.scaled_data(i, k), host.scaled_data(i, k)) for i in range(batch)), k
    assert all(same(s.result(nm), host.result(nm)) for nm in NAMES)


# ---- 6. the mode belongs to the setup
def test_a_handle_set_up_again_in_the_other_mode_is_a_fresh_handle_of_that_mode(orc, hip):
    n, p, m, batch = 4, 2, 3, 67
    mixed, mref = oracle_of_mixed(orc, hip, n, p, m, batch, LLT)
    shared, sref = oracle_of(orc, hip, n, p, m, batch, LLT)
    chain = oracle_chain(orc, hip, n, p, m, batch, LLT, WITH_MATRICES)
    salt1 = update_of(stacked(mixed_batch(n, p, m, batch, salt=1)), WITH_MATRICES)
    s = device(hip, mixed, LLT)
    assert s.L.pq_solver_batch_set_bound_sets(s.h, 0) == 0  # read by the next setup only: the problem that is set up keeps its own sets
    run_chain(hip, s, chain, salt1)
    # per instance -> shared
    s.setup(**stacked(shared))
    check_setup(orc, s, shared, sref)
    assert s.solve() == batch
    check_solve(hip, s, sref, "shared after per instance")
    with pytest.raises(RuntimeError, match="finite bounds"):
        s.update(**update_of(stacked(mixed), BOUNDS))
    with pytest.raises(RuntimeError, match="finite bounds"):
        s.setup(**stacked(mixed))
    # shared -> per instance
    assert s.L.pq_solver_batch_set_bound_sets(s.h, 1) == 0
    s.setup(**stacked(mixed))
    check_setup(orc, s, mixed, mref)
    run_chain(hip, s, chain, salt1)


# ---- 7. one vector alone: the side that is not given keeps what is stored
@pytest.mark.parametrize("name", BOUNDS)
def test_an_update_of_one_bound_vector_alone(orc, hip, name):
    """h_l or h_u alone: the batch is made of the instances whose lists in the reference do not hinge on the rounding of (1e30 d) (1 / d) (hinges_on_a_rounding of
    tests/batch_qp_mixed.py; on the others the library drops a row by its second rule, include/piqp_amd.h, and the reference leaves it in neither list): 61 resp. 62
    of the 67.  Rows dropped through the STORED side are among them."""
    n, p, m, batch = 4, 2, 3, 67
    q0, q1 = mixed_batch(n, p, m, batch), mixed_batch(n, p, m, batch, salt=1)
    keep = tuple(i for i in range(batch) if name[0] == "x" or not hinges_on_a_rounding(orc, q0[i], q1[i], name))
    assert len(keep) >= batch - 6
    chain = oracle_chain(orc, hip, n, p, m, batch, LLT, (name,), keep)
    assert sum(rec["counts0"] != rec["counts1"] for rec in chain) >= batch // 2, "the update is to change the sets"
    if name[0] == "h":
        k, other = LISTS.index(name), "h_u" if name == "h_l" else "h_l"
        # the given bound infinite, the stored other one infinite too (stored as -/+ 1e30: the row was not dropped at the setup, its own side was finite then)
        both_inf = [np.flatnonzero(~np.isfinite(q1[i][name]) & ~np.isfinite(q0[i][other]) & np.isfinite(q0[i][name])) for i in keep]
        assert any(len(r) and set(r) <= set(rec["lists1"][k]) for r, rec in zip(both_inf, chain)), "no instance drops a row through the stored side"
    s = device(hip, [q0[i] for i in keep], LLT)
    run_chain(hip, s, chain, update_of(stacked([q1[i] for i in keep]), (name,)))
    assert np.array_equal(s.statuses(), [rec["second"]["status"] for rec in chain])
