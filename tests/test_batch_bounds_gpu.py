"""The batched sparse solver with a set of finite bounds per instance (BatchSparseSolver(bounds="per_instance"), pq_batch_set_bound_sets; batch_solver.hip).

The yardstick for bits is the shared-mode path: a per-instance handle on a uniform batch is a shared handle bit for bit, and instance i of a mixed batch is, bit for
bit, a shared-mode handle of batch 1 set up from instance i's data alone (test_batch_ldlt_gpu.py::test_instances_do_not_interact shows that a batch of one equals
the member of a larger batch).  Against the CPU oracle the tolerances are those of test_batch_ldlt_gpu.py::_compare_solves.  Both backends (the default
sparse_multistage and sparse_ldlt) unless a test says otherwise.  Inputs: tests/batch_sparse_mixed.py."""
import ctypes as C

import numpy as np
import pytest

from batch_sparse_mixed import LISTS, debug_bound_lists, finite_sparse_batch, instance_args, kinds, mixed_sparse_batch, stored_flags, sub_batch, with_kinds
from qp_gen import mpc_batch
from test_batch_ldlt_gpu import _compare_solves, _random_sparse_qp_batch, _scalings

pytestmark = pytest.mark.gpu

B = 12
BACKENDS = ["multistage", "ldlt"]
FIELDS = ("x", "y", "z_l", "z_u", "z_bl", "z_bu", "s_l", "s_u", "s_bl", "s_bu")
TIMES = ("setup_time", "update_time", "solve_time", "kkt_factor_time", "kkt_solve_time", "run_time")
VECS = ("c", "b", "h_l", "h_u", "x_l", "x_u")
# (test, backend, dim) -> {instance: iterations of the batch} where it ends one iteration away from the oracle.  The rule for an entry: at most one per case, at most
# one iteration away, the instance SOLVED within the tolerances.  None so far.
PINNED = {}


def _ks(hip, orc, backend):
    return (hip.SPARSE_MULTISTAGE, orc.SPARSE_MULTISTAGE) if backend == "multistage" else (hip.SPARSE_LDLT, orc.SPARSE_LDLT)


def _handle(hip, bt, ks, bounds, **settings):
    bs = hip.BatchSparseSolver(kkt_solver=ks, bounds=bounds)
    for k, v in settings.items():
        setattr(bs.settings, k, v)
    assert bs.setup(bt["P"], bt["Pv"], bt["c"], bt["A"], bt["Av"], bt["b"], bt["G"], bt["Gv"], bt["h_l"], bt["h_u"], bt["x_l"], bt["x_u"])
    return bs


def _solved(bs):
    """everything a solve leaves: the ten result vectors and every info field that is not a time, per instance"""
    bs.solve()
    names = [f for f, _ in type(bs.info(0))._fields_ if f not in TIMES]
    info = np.array([[getattr(bs.info(i), f) for f in names] for i in range(bs.batch)], dtype=np.float64)
    return {**{k: bs.result(k) for k in FIELDS}, "info": info}


def _assert_same(a, b, ia=None, ib=None, what=""):
    """bitwise; ia / ib: instance lists (None: every instance of both)"""
    for k in a:
        x = a[k] if ia is None else a[k][ia]
        y = b[k] if ib is None else b[k][ib]
        assert np.array_equal(x, y, equal_nan=True), (what, k, np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1)).tolist()[:8])


def _vectors(bt):
    return {k: bt[k] for k in VECS if bt.get(k) is not None}


def _mpc_as_batch(nb):
    mb = mpc_batch(nb)
    return dict(P=mb["P_pattern"], Pv=mb["P_values"], c=mb["c"], A=mb["A_pattern"], Av=mb["A_values"], b=mb["b"], G=None, Gv=None, h_l=None, h_u=None, x_l=mb["x_l"], x_u=mb["x_u"], B=nb)


def _moved(bt, seed):
    """other values, the same set of finite bounds (an infinity stays where it is)"""
    rng = np.random.default_rng(seed)
    out = dict(bt)
    out["c"] = bt["c"] + 0.1 * rng.standard_normal(bt["c"].shape)
    out["Pv"] = bt["Pv"] * (1.0 + 0.5 * rng.random(bt["Pv"].shape[0]))[:, None]
    out["Av"] = bt["Av"] * (1 + 0.05 * rng.uniform(-1, 1, bt["Av"].shape))
    if bt["G"] is not None:
        out["Gv"] = bt["Gv"] * (1 + 0.05 * rng.uniform(-1, 1, bt["Gv"].shape))
        out["h_l"], out["h_u"] = bt["h_l"] - 0.05, bt["h_u"] + 0.05
    out["x_l"], out["x_u"] = bt["x_l"] - 0.05, bt["x_u"] + 0.05
    return out


def _held_lists(bs, i):
    got = bs.bound_lists(i)
    return {k: got[k + "_idx"].tolist() for k in LISTS}, got["dropped"]


def _oracle_lists(od):
    return {k: od.idx(k).tolist() for k in LISTS}


def _check_lists_after_update(bs, before, given, oracles=None):
    """every instance's lists after an update with the vectors `given` ({name: [B, len]}): the host statement of the rules on the lists held before, the oracle's
    Data where a Solver that got the same update is at hand, and `dropped` = the rows the call dropped (unchanged by a call without h_l and h_u)"""
    for i in range(bs.batch):
        lists, dropped = _held_lists(bs, i)
        exp, dead = debug_bound_lists(bs.L, bs.m, bs.n, {k: v[i] for k, v in given.items()}, stored_flags(before[i][0], bs.n, bs.m))
        assert lists == exp, i
        assert np.array_equal(dropped, dead if ("h_l" in given or "h_u" in given) else before[i][1]), i
        if oracles is not None:
            assert lists == _oracle_lists(oracles[i].data()), i


def _oracle_solver(orc, oks, bt, i, **settings):
    s = orc.Solver()
    s.settings.kkt_solver = oks
    for k, v in settings.items():
        setattr(s.settings, k, v)
    assert s.setup(**instance_args(bt, i), sparse=True)
    return s


def _compare_with(bs, oracles, key):
    """_compare_solves of test_batch_ldlt_gpu.py -- status, iteration count, x / y / z with its tolerances -- against oracle Solvers that are already solved"""
    res = {k: bs.result(k) for k in ("x", "y", "z_l", "z_u", "z_bl", "z_bu")}
    pinned = PINNED.get(key, {})
    assert len(pinned) <= 1
    off = {}
    for i, s in enumerate(oracles):
        info = bs.info(i)
        print(f"{key} instance {i}: status {info.status} / {s.info.status}, iterations {info.iter} / {s.info.iter}")
        assert info.status == s.info.status, (i, info.status, s.info.status)
        if i in pinned:
            assert abs(pinned[i] - s.info.iter) <= 1 and info.status == 1
        if info.iter != pinned.get(i, s.info.iter):
            off[i] = (info.iter, s.info.iter)
        if s.info.status != 1:
            continue
        ref = s.result()
        assert np.abs(res["x"][i] - ref["x"]).max(initial=0) <= 1e-7 * (1 + np.abs(ref["x"]).max(initial=0)), i
        for k in ("y", "z_l", "z_u", "z_bl", "z_bu"):
            r = np.nan_to_num(ref[k], posinf=0, neginf=0)
            assert np.abs(res[k][i] - r).max(initial=0) <= 1e-6 * (1 + np.abs(r).max(initial=0)), (i, k)
    assert not off, ("instance: (batch, oracle) iterations", off)


# ---- 1. a uniform batch: the shared path, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("data", ["mpc24", "dim16", "dim64"])
def test_uniform_batch_is_bitwise_a_shared_handle(hip, orc, backend, data):
    ks, _ = _ks(hip, orc, backend)
    bt = _mpc_as_batch(24) if data == "mpc24" else _random_sparse_qp_batch(int(data[3:]), B, seed=int(data[3:]))
    sh, pi = _handle(hip, bt, ks, "shared"), _handle(hip, bt, ks, "per_instance")
    assert sh.last_kernel_ms()[1] == pi.last_kernel_ms()[1]
    _assert_same(_solved(sh), _solved(pi), what="setup")
    assert sh.last_kernel_ms()[1] == pi.last_kernel_ms()[1], "threads per QP"
    b1 = _moved(bt, 1)
    for s in (sh, pi):
        assert s.update(**_vectors(b1))
    _assert_same(_solved(sh), _solved(pi), what="update")
    b2 = _moved(b1, 2)
    for s in (sh, pi):
        assert s.update_data(P_values=b2["Pv"], A_values=b2["Av"], G_values=b2["Gv"], **_vectors(b2))
    _assert_same(_solved(sh), _solved(pi), what="update_data")
    for i in (0, bt["B"] - 1):
        a, b = sh.bound_lists(i), pi.bound_lists(i)
        assert all(np.array_equal(a[k], b[k]) for k in a), i


# ---- 2. + 3. a mixed batch at setup --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dim", [16, 64])
def test_mixed_batch_at_setup(hip, orc, backend, dim):
    ks, oks = _ks(hip, orc, backend)
    bt = mixed_sparse_batch(dim, B)
    pi = _handle(hip, bt, ks, "per_instance")
    got = _solved(pi)
    for i in range(B):
        one = _handle(hip, sub_batch(bt, [i]), ks, "shared")
        _assert_same(_solved(one), got, None, [i], what=f"instance {i} against a shared handle of batch 1")
        assert one.last_kernel_ms()[1] == pi.last_kernel_ms()[1], "threads per QP"
        lists, dropped = _held_lists(pi, i)
        q = instance_args(bt, i)
        exp, dead = debug_bound_lists(pi.L, pi.m, pi.n, q)
        assert lists == exp == _oracle_lists(orc.Data.sparse(**q)) == _held_lists(one, 0)[0], i
        assert np.array_equal(dropped, dead) and np.array_equal(dropped, _held_lists(one, 0)[1]), i
    # (a pin would be an instance whose shared handle of batch 1 shows the same count: the bitwise equality above asserts that)
    _compare_solves(pi, orc, bt, pinned=PINNED.get(("setup", backend, dim)), kkt_solver=oks)


def test_shared_mode_still_refuses_and_a_handle_keeps_its_mode(hip, orc):
    bt, b1 = mixed_sparse_batch(16, B), mixed_sparse_batch(16, B, 1)
    L = hip._lib.load()
    sh = hip.BatchSparseSolver()
    for bad in (2, -1, 7):
        assert L.pq_batch_set_bound_sets(sh.h, bad) == -1 and L.pq_last_error_string().decode()
    with pytest.raises(Exception, match="batch setup: instances differ in which bounds are finite"):
        sh.setup(bt["P"], bt["Pv"], bt["c"], bt["A"], bt["Av"], bt["b"], bt["G"], bt["Gv"], bt["h_l"], bt["h_u"], bt["x_l"], bt["x_u"])
    fin = finite_sparse_batch(16, B)
    sh = _handle(hip, fin, hip.SPARSE_MULTISTAGE, "shared")
    assert L.pq_batch_set_bound_sets(sh.h, 1) == 0  # read by the next setup only
    for call in (lambda: sh.update(h_l=b1["h_l"]), lambda: sh.update_data(G_values=b1["Gv"], x_u=b1["x_u"])):
        with pytest.raises(Exception, match="batch update: the set of finite bounds differs from the one given at setup"):
            call()
    pi = _handle(hip, bt, hip.SPARSE_MULTISTAGE, "per_instance")
    assert L.pq_batch_set_bound_sets(pi.h, 0) == 0
    assert pi.update(h_l=b1["h_l"], h_u=b1["h_u"]) and pi.update_data(G_values=b1["Gv"], x_u=b1["x_u"])
    with pytest.raises(Exception, match="out of range"):
        pi.bound_lists(B)


# ---- 4. update_data(G, h_l, h_u, x_l, x_u): from the sets of salt 0 to those of salt 1 ----------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dim", [16, 64])
def test_update_data_to_other_sets_matches_the_oracle(hip, orc, backend, dim):
    ks, oks = _ks(hip, orc, backend)
    b0, b1 = mixed_sparse_batch(dim, B), mixed_sparse_batch(dim, B, 1)
    pi = _handle(hip, b0, ks, "per_instance")
    pi.solve()
    before = [_held_lists(pi, i) for i in range(B)]
    given = {k: b1[k] for k in LISTS}
    assert pi.update_data(G_values=b1["Gv"], **given)
    oracles = []
    for i in range(B):
        s = _oracle_solver(orc, oks, b0, i)
        s.solve()
        a = instance_args(b1, i)
        assert s.update(G=a["G"], h_l=a["h_l"], h_u=a["h_u"], x_l=a["x_l"], x_u=a["x_u"])
        oracles.append(s)
    _check_lists_after_update(pi, before, given, oracles)
    pi.solve()
    for s in oracles:
        s.solve()
    _compare_with(pi, oracles, ("update_data", backend, dim))


# ---- 5. what an update_data of everything leaves does not depend on what was there ------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_update_data_of_everything_forgets_the_history(hip, orc, backend):
    """Two per-instance handles with preconditioner_reuse_on_update = 0, one set up with the sets of salt 0 and one with every bound finite, get every matrix and
    vector of salt 1: every stored value is overwritten, every list rebuilt and the equilibration starts afresh.  The lists, statuses and iteration counts are
    equal; the results are compared within the tolerances of _compare_solves, not bitwise, because shared-mode handles already carry one trace of their history
    through such an update: x_b_scaling is multiplied by the old scalings' inverses and by the new scalings, it is not set again.  Two SHARED handles set up with
    different matrix values and given the same update_data(everything) end with equal iteration counts and x that differs by 1.1e-11 (sparse_multistage) and
    5.8e-12 (sparse_ldlt) at dim 16, 12 instances."""
    ks, _ = _ks(hip, orc, backend)
    dim = 16
    b1 = mixed_sparse_batch(dim, B, 1)
    out = []
    for start in (mixed_sparse_batch(dim, B), finite_sparse_batch(dim, B)):
        s = _handle(hip, start, ks, "per_instance", preconditioner_reuse_on_update=0)
        s.solve()
        assert s.update_data(P_values=b1["Pv"], A_values=b1["Av"], G_values=b1["Gv"], **_vectors(b1))
        out.append((_solved(s), [_held_lists(s, i) for i in range(B)]))
    assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(out[0][1], out[1][1]))
    a, b = out[0][0], out[1][0]
    assert np.array_equal(a["info"][:, :2], b["info"][:, :2]), "statuses and iteration counts"
    assert (a["info"][:, 0] == 1).all()
    for k, tol in (("x", 1e-7), ("y", 1e-6), ("z_l", 1e-6), ("z_u", 1e-6), ("z_bl", 1e-6), ("z_bu", 1e-6)):
        for i in range(B):
            print(f"history, {backend}, {k}, instance {i}: max difference {np.abs(a[k][i] - b[k][i]).max(initial=0):.3e}")
            assert np.abs(a[k][i] - b[k][i]).max(initial=0) <= tol * (1 + np.abs(b[k][i]).max(initial=0)), (k, i)


# ---- 6. updates of vectors only ----------------------------------------------------------------------------------------------------------------------------------
def _vector_update_case(dim, drop):
    """salt 0, then bounds whose row kinds (a) permute both / lower / upper on the rows that are alive and keep the dropped rows dropped, (b) are those of salt 1
    except on the rows dropped before, which stay dropped: rows go, none comes back.  The boxes are those of salt 1."""
    ks0 = [kinds(dim, B, i, 0) for i in range(B)]
    ks1 = [kinds(dim, B, i, 1) for i in range(B)]
    row0, row1, var1 = np.array([k[0] for k in ks0]), np.array([k[0] for k in ks1]), np.array([k[1] for k in ks1])
    row = np.where(row0 == 3, 3, row1 if drop else (row0 + 1) % 3)
    return mixed_sparse_batch(dim, B), with_kinds(finite_sparse_batch(dim, B), row, var1)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("drop", [False, True], ids=["alive", "drop"])
@pytest.mark.parametrize("dim", [16, 64])
def test_vector_updates_match_the_oracle(hip, orc, backend, dim, drop):
    """(a) `alive`: against the oracle's update of the same vectors.  (b) `drop`: a row that loses its last bound has its entries of G' zeroed in the one copy the
    KKT matrix is assembled from (include/piqp_amd.h at pq_batch_set_bound_sets); the reference in that state is the oracle after update(G = its own G, the
    vectors) with preconditioner_reuse_on_update = 1."""
    ks, oks = _ks(hip, orc, backend)
    b0, b1 = _vector_update_case(dim, drop)
    pi = _handle(hip, b0, ks, "per_instance")
    pi.solve()
    before = [_held_lists(pi, i) for i in range(B)]
    given = {k: b1[k] for k in LISTS}
    assert pi.update(**given)
    oracles = []
    for i in range(B):
        s = _oracle_solver(orc, oks, b0, i, preconditioner_reuse_on_update=int(drop))
        s.solve()
        a = instance_args(b1, i)
        assert s.update(G=a["G"] if drop else None, h_l=a["h_l"], h_u=a["h_u"], x_l=a["x_l"], x_u=a["x_u"])
        oracles.append(s)
    _check_lists_after_update(pi, before, given, oracles)
    if drop:
        assert sum(int(_held_lists(pi, i)[1].sum() - before[i][1].sum()) for i in range(B)) > 0, "the case is to drop rows"
    pi.solve()
    for s in oracles:
        s.solve()
    _compare_with(pi, oracles, ("update_drop" if drop else "update_alive", backend, dim))


@pytest.mark.parametrize("backend", BACKENDS)
def test_lists_after_vector_updates_that_bring_rows_back(hip, orc, backend):
    """the lists only (a row that comes back keeps its zero entries of G' until G values are given): all four vectors, then each alone"""
    ks, oks = _ks(hip, orc, backend)
    b0, b1 = mixed_sparse_batch(16, B), mixed_sparse_batch(16, B, 1)
    pi = _handle(hip, b0, ks, "per_instance")
    before = [_held_lists(pi, i) for i in range(B)]
    oracles = [_oracle_solver(orc, oks, b0, i) for i in range(B)]
    assert pi.update(**{k: b1[k] for k in LISTS})
    for i, s in enumerate(oracles):
        assert s.update(**{k: b1[k][i] for k in LISTS})
    _check_lists_after_update(pi, before, {k: b1[k] for k in LISTS}, oracles)
    assert any((before[i][1] & ~_held_lists(pi, i)[1]).any() for i in range(B)), "the case is to bring rows back"
    for k in LISTS:  # one vector alone, back to salt 0 (h_l or h_u alone: the rules as stated, see pq_solver_batch_update_dense for the reference's rounding)
        before = [_held_lists(pi, i) for i in range(B)]
        assert pi.update(**{k: b0[k]})
        _check_lists_after_update(pi, before, {k: b0[k]})


# ---- 7. vectors and values in device memory ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_device_memory_updates_are_bitwise_the_host_fed_ones(hip, orc, backend):
    import torch
    ks, _ = _ks(hip, orc, backend)
    b0, b1 = mixed_sparse_batch(16, B), mixed_sparse_batch(16, B, 1)
    host, dev = _handle(hip, b0, ks, "per_instance"), _handle(hip, b0, ks, "per_instance")
    t = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    vec1, vec0 = {k: t(v) for k, v in _vectors(b1).items()}, {k: t(v) for k, v in _vectors(b0).items()}
    G0, P0 = t(b0["Gv"]), t(b0["Pv"])
    torch.cuda.synchronize()
    count = host.L.pq_debug_alloc_count
    assert host.update(**_vectors(b1))
    a0 = count()
    assert dev.update(**vec1)
    dev.solve()
    xs = [dev.result(k, device=True) for k in FIELDS]
    assert count() == a0, "update, solve and the result calls must not allocate"
    _assert_same(_solved(host), _solved(dev), what="update")
    assert all(np.array_equal(x.cpu().numpy(), dev.result(k)) for k, x in zip(FIELDS, xs))
    assert host.update_data(P_values=b0["Pv"], G_values=b0["Gv"], **_vectors(b0))
    a0 = count()
    assert dev.update_data(P_values=P0, G_values=G0, **vec0)
    dev.solve()
    assert count() == a0, "update_data and solve must not allocate"
    _assert_same(_solved(host), _solved(dev), what="update_data")
    for i in range(B):
        assert _held_lists(host, i)[0] == _held_lists(dev, i)[0]


# ---- 8. the backend's hooks on a mixed batch ----------------------------------------------------------------------------------------------------------------------
def test_ldlt_factor_and_solve_bitwise_equal_the_oracle_on_a_mixed_batch(hip, orc):
    bt = mixed_sparse_batch(16, B)
    bs = _handle(hip, bt, hip.SPARSE_LDLT, "per_instance", preconditioner_iter=0)
    n, p, m = bs.n, bs.p, bs.m
    rng = np.random.default_rng(5)
    for late in (False, True):
        sc = [_scalings(n, m, rng, late) for _ in range(B)]
        ok = bs.kkt_factor(np.array([s[0] for s in sc]), np.array([s[1] for s in sc]).reshape(B, n), np.array([s[2] for s in sc]).reshape(B, m))
        rx, ry, rz = rng.standard_normal((B, n)), rng.standard_normal((B, p)), rng.standard_normal((B, m))
        lx, ly, lz = bs.kkt_solve(rx, ry, rz)
        for i in range(B):
            ko = orc.KKT(orc.Data.sparse(**instance_args(bt, i)), kind="sparse", mode=0)
            assert bool(ok[i]) and ko.update_scalings_and_factor(*sc[i]), (late, i)
            fh, fo = bs.ldlt_factor(i), ko.sparse_factor()
            for k in ("perm", "L_cols", "L_ind", "PKPt_val", "L_vals", "D", "D_inv"):
                assert np.array_equal(fh[k], fo[k]), (late, i, k)
            lo = ko.solve(rx[i], ry[i], rz[i])
            for a, b, nm in zip((lx[i], ly[i], lz[i]), lo, "xyz"):
                assert np.array_equal(a, np.asarray(b)), (late, i, nm)


# ---- 9. more instances than the device holds at once -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_full_chip_mixed_batch_is_bitwise_four_shared_handles(hip, orc, backend):
    """2048 instances at dim 16, the kinds of the forced patterns f = 0 .. 3 cycling over them: several rounds of workgroups, the start order (the second solve
    starts the instances that took longest first) and the stride of the table.  The values are 128 distinct instances repeated, each under all four patterns."""
    ks, _ = _ks(hip, orc, backend)
    dim, nb, base = 16, 2048, 128
    fin = finite_sparse_batch(dim, base)
    bt = sub_batch(fin, np.arange(nb) % base)
    kind = (np.arange(nb) // base + np.arange(nb)) % 4
    from batch_sparse_mixed import FORCED
    row = np.array([[FORCED[k][0]] * (dim // 2) for k in kind])
    var = np.array([[FORCED[k][1]] * dim for k in kind])
    bt = with_kinds(bt, row, var)
    pi = _handle(hip, bt, ks, "per_instance")
    first = _solved(pi)
    second = _solved(pi)
    _assert_same(first, second, what="the start order")
    assert (first["info"][:, 0] == 1).all()
    for k in range(4):
        idx = np.flatnonzero(kind == k)
        assert len(idx) == 512
        sh = _handle(hip, sub_batch(bt, idx), ks, "shared")
        _assert_same(_solved(sh), first, None, idx, what=f"pattern {k}")
