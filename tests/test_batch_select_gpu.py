"""The batched sparse solver acting on a list of instances in place (BatchSparseSolver.solve / update / update_data / result with instances=..., arena_row;
pq_batch_solve_select, pq_batch_update_select_mem, pq_batch_update_data_select_mem, pq_batch_get_result_select_mem, pq_batch_arena_row; batch_solver.hip).

The yardstick is the whole-batch path, bit for bit: a LISTED instance ends as the same instance of a twin handle that got the whole-batch call with the same row --
the ten result vectors and every info field that is not a time (_assert_same of tests/test_batch_bounds_gpu.py), after an update its whole row of the arena --, and of
an UNLISTED instance nothing changes against a snapshot taken before the call: the ten vectors, every info field with the times, the profile row, the arena row and,
with lists per instance, its lists.  The whole-batch path is held to the CPU oracle by the existing suite; one test here repeats _compare_solves of
tests/test_batch_ldlt_gpu.py on instances the clone tests already pass under it, so no tolerance is introduced.  Both backends (sparse_multistage, sparse_ldlt),
batches of 12.  Inputs: mpc_batch(12) (wave-per-QP kernel mode, p > 0, m = 0, boxes), _random_sparse_qp_batch(16, 12) (A, G, boxes, shared infinities),
mixed_sparse_batch(16, 12) (lists per instance), an MPC batch of n = 540 (the 256-thread kernel)."""

import numpy as np
import pytest

from batch_sparse_mixed import finite_sparse_batch, mixed_sparse_batch
from qp_gen import mpc_batch
from test_batch_bounds_gpu import FIELDS, TIMES, _assert_same, _handle, _moved, _mpc_as_batch, _solved, _vectors
from test_batch_ldlt_gpu import _compare_solves, _random_sparse_qp_batch, _scalings

pytestmark = pytest.mark.gpu

B = 12
BACKENDS = ["multistage", "ldlt"]
DATA = ["mpc", "dim16"]
COMBOS = [("multistage", "mpc"), ("multistage", "dim16"), ("ldlt", "dim16")]
PERM = [5, 0, 11, 3, 8, 1, 10, 2, 7, 4, 9, 6]  # (of tests/test_batch_sparse_clone_gpu.py)
LISTS = {"single": [7], "descending": [10, 7, 4, 1], "ends": [0, 11], "permutation": PERM, "all": list(range(B))}
SOLVED, MAX_ITER_REACHED, INVALID_SETTINGS = 1, -1, -10
REFUSED = "batch update: the set of finite bounds differs from the one given at setup"

_batches = {}


def _batch(data):
    """computed once per key; nobody changes it"""
    if data not in _batches:
        _batches[data] = _mpc_as_batch(B) if data == "mpc" else _random_sparse_qp_batch(16, B, seed=16)
    return _batches[data]


def _ks(hip, backend):
    return hip.SPARSE_MULTISTAGE if backend == "multistage" else hip.SPARSE_LDLT


def _oks(orc, backend):
    return orc.SPARSE_MULTISTAGE if backend == "multistage" else orc.SPARSE_LDLT


def _rest(lst, batch=B):
    return [i for i in range(batch) if i not in set(lst)]


def _torch(d):
    import torch
    out = {k: torch.tensor(v, dtype=torch.float64, device="cuda:0") for k, v in d.items() if v is not None}
    torch.cuda.synchronize()
    return out


def _feed(mem):
    return _torch if mem == "device" else (lambda d: {k: v for k, v in d.items() if v is not None})


def _info(bs, times):
    names = [f for f, _ in type(bs.info(0))._fields_ if times or f not in TIMES]
    return np.array([[getattr(bs.info(i), f) for f in names] for i in range(bs.batch)], dtype=np.float64)


def _held(bs):
    """what _solved returns, of the handle as it stands (no solve): what a listed instance is compared in"""
    return {**{k: bs.result(k) for k in FIELDS}, "info": _info(bs, False)}


def _arena(bs):
    return np.array([bs.arena_row(i) for i in range(bs.batch)])


def _state(bs):
    """everything the handle holds per instance: what an unlisted instance is compared in"""
    prof = np.zeros((bs.batch, 8))
    for i in range(bs.batch):
        assert bs.L.pq_batch_get_profile(bs.h, i, prof[i].ctypes.data) == 0
    out = {**{k: bs.result(k) for k in FIELDS}, "info": _info(bs, True), "profile": prof, "arena": _arena(bs)}
    if bs.bounds == "per_instance":
        lists = [bs.bound_lists(i) for i in range(bs.batch)]
        for k in ("h_l_idx", "h_u_idx", "x_l_idx", "x_u_idx", "dropped"):
            out[k] = np.array([np.pad(np.asarray(l[k], dtype=np.int64), (0, max(bs.n, bs.m) + 1 - len(l[k])), constant_values=-1) for l in lists])
    return out


def _rows(new, old, lst, keys):
    """(the listed rows of `new`, the whole-batch stacks that are `new` at lst and `old` elsewhere) for the keys that exist"""
    lst = np.asarray(lst)
    sel, mix = {}, {}
    for k in keys:
        if new.get(k) is None:
            continue
        sel[k] = new[k][lst]
        mix[k] = old[k].copy()
        mix[k][lst] = new[k][lst]
    return sel, mix


# ---- 1. a fresh handle: solve by list, the others untouched, the next whole solve sound ------------------------------------------------------------------------
@pytest.mark.parametrize("lpt", [True, False], ids=["longest_first", "list_order"])
@pytest.mark.parametrize("lst", list(LISTS))
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("backend", BACKENDS)
def test_solve_by_list_on_a_fresh_handle(hip, backend, data, lst, lpt):
    bt, lst = _batch(data), LISTS[lst]
    bs, twin = _handle(hip, bt, _ks(hip, backend), "shared"), _handle(hip, bt, _ks(hip, backend), "shared")
    bs.set_start_order(lpt); twin.set_start_order(lpt)
    want = _solved(twin)
    before = _state(bs)
    assert (bs.iterations() == 0).all()
    a0 = bs.L.pq_debug_alloc_count()
    assert bs.solve(instances=lst) == int((twin.statuses()[lst] == SOLVED).sum())
    assert bs.L.pq_debug_alloc_count() - a0 == 1, "the first call by list makes the one list buffer"
    assert bs.last_kernel_ms()[0] > 0
    _assert_same(_held(bs), want, lst, lst, what="listed against the twin's whole solve")
    _assert_same(_state(bs), before, _rest(lst), _rest(lst), what="unlisted against the snapshot")
    # the stored order of the whole launch is a permutation of the batch still: the whole solve is the twin's, and so are a solve by list after it (its start order
    # now from real iteration counts) and the whole solve after that
    _assert_same(_solved(bs), want, what="whole solve after a solve by list")
    mid = _state(bs)
    bs.solve(instances=lst)
    assert bs.L.pq_debug_alloc_count() - a0 == 1
    _assert_same(_held(bs), want, what="a second solve by list")
    _assert_same(_state(bs), mid, _rest(lst), _rest(lst), what="unlisted against the snapshot, second time")
    _assert_same(_solved(bs), want, what="whole solve again")


@pytest.mark.parametrize("lpt", [True, False], ids=["longest_first", "list_order"])
def test_start_order_with_more_instances_than_the_device_holds(hip, lpt):
    """600 MPC QPs, iteration counts that differ: a list of 200 in descending index order, solved between whole solves"""
    bt = _mpc_as_batch(600)
    bs, twin = _handle(hip, bt, hip.SPARSE_MULTISTAGE, "shared"), _handle(hip, bt, hip.SPARSE_MULTISTAGE, "shared")
    bs.set_start_order(lpt); twin.set_start_order(lpt)
    want = _solved(twin)
    assert len(set(twin.iterations().tolist())) > 1
    lst = list(range(599, -1, -3))
    bs.solve(instances=lst)
    _assert_same(_held(bs), want, lst, lst, what="fresh")
    _assert_same(_solved(bs), want, what="whole")
    x0 = bs.result("x")
    bs.solve(instances=lst)
    assert np.array_equal(bs.result("x"), x0)
    _assert_same(_solved(bs), want, what="whole again")
    _assert_same(_solved(bs), want, what="and once more")


# ---- 2. the oracle anchor ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("backend", BACKENDS)
def test_solve_by_list_against_the_oracle(hip, orc, backend, data):
    bt = _batch(data)
    bs = _handle(hip, bt, _ks(hip, backend), "shared")
    fresh = bs.statuses()
    bs.solve(instances=[10, 5, 0])
    _compare_solves(bs, orc, bt, idx=[0, 5, 10], kkt_solver=_oks(orc, backend))
    rest = _rest([10, 5, 0])
    assert np.array_equal(bs.statuses()[rest], fresh[rest]) and (bs.iterations()[rest] == 0).all(), "the others were not solved"


# ---- 3. update by list after a whole solve ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("lst", list(LISTS))
@pytest.mark.parametrize("backend,data", COMBOS)
def test_update_by_list_then_solve_by_list(hip, backend, data, lst, mem):
    """(the cost is scaled, so the stored cost scaling the update multiplies c with is not 1)"""
    bt, lst = _batch(data), LISTS[lst]
    bs, twin = (_handle(hip, bt, _ks(hip, backend), "shared", preconditioner_scale_cost=1) for _ in range(2))
    bs.solve(); twin.solve()
    before = _state(bs)
    sel, mix = _rows(_moved(bt, 1), bt, lst, ("b", "c"))
    assert bs.update(instances=lst, **_feed(mem)(sel)) and twin.update(**_feed(mem)(mix))
    after = _state(bs)
    _assert_same(after, before, _rest(lst), _rest(lst), what="update: unlisted against the snapshot")
    _assert_same({k: after[k] for k in (*FIELDS, "info", "profile")}, before, what="update: results and infos stay until the next solve")
    assert np.array_equal(after["arena"][lst], _arena(twin)[lst]), "update: the listed rows of the arena against the twin's"
    assert not np.array_equal(after["arena"][lst], before["arena"][lst]), "the case is to change them"
    want = _solved(twin)
    assert bs.solve(instances=lst) == int((twin.statuses()[lst] == SOLVED).sum())
    _assert_same(_held(bs), want, lst, lst, what="solve: listed against the twin")
    _assert_same(_state(bs), before, _rest(lst), _rest(lst), what="solve: unlisted against the snapshot")


# ---- 4. update_data by list -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("reuse", [0, 1])
@pytest.mark.parametrize("what", ["matrices", "matrices_and_vectors"])
@pytest.mark.parametrize("lst", ["descending", "permutation"])
@pytest.mark.parametrize("backend,data", COMBOS)
def test_update_data_by_list(hip, backend, data, lst, what, reuse, mem):
    bt, lst = _batch(data), LISTS[lst]
    bs, twin = (_handle(hip, bt, _ks(hip, backend), "shared", preconditioner_reuse_on_update=reuse, preconditioner_scale_cost=reuse) for _ in range(2))
    bs.solve(); twin.solve()
    before = _state(bs)
    keys = ("Pv", "Av", "Gv") + (("c", "b", "h_l", "h_u", "x_l", "x_u") if what == "matrices_and_vectors" else ())
    sel, mix = _rows(_moved(bt, 2), bt, lst, keys)
    name = lambda d: {dict(Pv="P_values", Av="A_values", Gv="G_values").get(k, k): v for k, v in d.items()}
    assert bs.update_data(instances=lst, **_feed(mem)(name(sel))) and twin.update_data(**_feed(mem)(name(mix)))
    after = _state(bs)
    _assert_same(after, before, _rest(lst), _rest(lst), what="update_data: unlisted against the snapshot")
    assert np.array_equal(after["arena"][lst], _arena(twin)[lst]), "update_data: the listed rows of the arena against the twin's"
    assert not np.array_equal(after["arena"][lst], before["arena"][lst])
    if backend == "ldlt":
        rng = np.random.default_rng(5)
        sc = [_scalings(bs.n, bs.m, rng, False) for _ in range(B)]
        args = (np.array([s[0] for s in sc]), np.array([s[1] for s in sc]).reshape(B, bs.n), np.array([s[2] for s in sc]).reshape(B, bs.m))
        assert bs.kkt_factor(*args).all() and twin.kkt_factor(*args).all()
        for i in lst:
            fa, fb = bs.ldlt_factor(i), twin.ldlt_factor(i)
            assert sorted(fa) == sorted(fb) and all(np.array_equal(fa[k], fb[k]) for k in fb), i
        return  # (the solve after such an update: the next test, with both backends)
    want = _solved(twin)
    bs.solve(instances=lst)
    _assert_same(_held(bs), want, lst, lst, what="solve: listed against the twin")
    _assert_same(_state(bs), before, _rest(lst), _rest(lst), what="solve: unlisted against the snapshot")


@pytest.mark.parametrize("backend,data", COMBOS)
def test_update_data_by_list_solves_to_the_twins_bits_with_both_backends(hip, backend, data):
    """the solve the ldlt cases of the test above leave out (their factor hook comes first)"""
    bt, lst = _batch(data), LISTS["descending"]
    bs, twin = (_handle(hip, bt, _ks(hip, backend), "shared") for _ in range(2))
    bs.solve(); twin.solve()
    before = _state(bs)
    sel, mix = _rows(_moved(bt, 2), bt, lst, ("Pv", "Av", "Gv", "c", "x_l"))
    name = lambda d: {dict(Pv="P_values", Av="A_values", Gv="G_values").get(k, k): v for k, v in d.items()}
    assert bs.update_data(instances=lst, **name(sel)) and twin.update_data(**name(mix))
    want = _solved(twin)
    bs.solve(instances=lst)
    _assert_same(_held(bs), want, lst, lst, what="listed against the twin")
    _assert_same(_state(bs), before, _rest(lst), _rest(lst), what="unlisted against the snapshot")


def test_the_256_thread_kernel_shape(hip):
    """n = 540 > 512: 256 threads per QP in the equilibration, the prepare kernel and the solve"""
    mb = mpc_batch(B, T=180, nx=2, nu=1, seed=77)
    bt = dict(P=mb["P_pattern"], Pv=mb["P_values"], c=mb["c"], A=mb["A_pattern"], Av=mb["A_values"], b=mb["b"], G=None, Gv=None, h_l=None, h_u=None, x_l=mb["x_l"],
              x_u=mb["x_u"], B=B)
    bs, twin = _handle(hip, bt, hip.SPARSE_MULTISTAGE, "shared"), _handle(hip, bt, hip.SPARSE_MULTISTAGE, "shared")
    assert bs.last_kernel_ms()[1] == 256
    lst = LISTS["descending"]
    want = _solved(twin)
    before = _state(bs)
    bs.solve(instances=lst)
    assert bs.last_kernel_ms()[1] == 256
    _assert_same(_held(bs), want, lst, lst, what="fresh: listed")
    _assert_same(_state(bs), before, _rest(lst), _rest(lst), what="fresh: unlisted")
    _assert_same(_solved(bs), want, what="whole")
    before = _state(bs)
    sel, mix = _rows(_moved(bt, 1), bt, lst, ("Pv", "Av", "c", "b", "x_l", "x_u"))
    name = lambda d: {dict(Pv="P_values", Av="A_values").get(k, k): v for k, v in d.items()}
    assert bs.update_data(instances=lst, **name(sel)) and twin.update_data(**name(mix))
    assert np.array_equal(_arena(bs)[lst], _arena(twin)[lst])
    want = _solved(twin)
    bs.solve(instances=lst)
    _assert_same(_held(bs), want, lst, lst, what="update_data: listed")
    _assert_same(_state(bs), before, _rest(lst), _rest(lst), what="update_data: unlisted")
    assert all(np.array_equal(bs.result(k, instances=PERM), bs.result(k)[PERM]) for k in FIELDS)


# ---- 5. sets of finite bounds per instance ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_per_instance_lists_follow_an_update_by_list(hip, backend, mem):
    """instance 0 of the mixed batch has every bound, instance 3 every row of G dropped, instance 4 no finite bound.  Listed: 0, 3, 4, 7, 10.  Step 1 (vectors) switches
    row 1 of G and the box of variable 2 off in them; step 2 (update_data with G_values) gives them the bounds of salt 1 -- rows come back --; the twin gets the whole
    batch with the old rows elsewhere."""
    b0, b1 = mixed_sparse_batch(16, B), mixed_sparse_batch(16, B, 1)
    lst = [10, 7, 4, 3, 0]
    bs, twin = _handle(hip, b0, _ks(hip, backend), "per_instance"), _handle(hip, b0, _ks(hip, backend), "per_instance")
    bs.solve(); twin.solve()
    lists = ("h_l_idx", "h_u_idx", "x_l_idx", "x_u_idx", "dropped")
    off = {k: b0[k].copy() for k in ("h_l", "h_u", "x_l", "x_u")}
    off["h_l"][:, 1], off["h_u"][:, 1], off["x_l"][:, 2], off["x_u"][:, 2] = -np.inf, np.inf, -np.inf, np.inf
    assert not bs.bound_lists(0)["dropped"][1]
    cur = {"Gv": b0["Gv"], **{k: b0[k] for k in ("h_l", "h_u", "x_l", "x_u")}}  # what every instance holds
    name = lambda d: {dict(Gv="G_values").get(k, k): v for k, v in d.items()}
    for step, new, keys in (("off", off, ("h_l", "h_u", "x_l", "x_u")), ("back", b1, ("Gv", "h_l", "h_u", "x_l", "x_u"))):
        before = _state(bs)
        sel, mix = _rows(new, cur, lst, keys)
        cur = {**cur, **mix}
        if step == "off":
            assert bs.update(instances=lst, **_feed(mem)(sel)) and twin.update(**_feed(mem)(mix))
            assert bs.bound_lists(0)["dropped"][1] and 2 not in bs.bound_lists(0)["x_l_idx"].tolist()
        else:
            assert bs.update_data(instances=lst, **_feed(mem)(name(sel))) and twin.update_data(**_feed(mem)(name(mix)))
        after = _state(bs)
        assert not all(np.array_equal(after[k][lst], before[k][lst]) for k in lists), "the case is to change the listed lists"
        for i in lst:
            la, lb = bs.bound_lists(i), twin.bound_lists(i)
            assert all(np.array_equal(la[k], lb[k]) for k in lb), (step, i)
        _assert_same(after, before, _rest(lst), _rest(lst), what=f"{step}: unlisted against the snapshot, lists included")
        assert np.array_equal(after["arena"][lst], _arena(twin)[lst]), step
        want = _solved(twin)
        bs.solve(instances=lst)
        _assert_same(_held(bs), want, lst, lst, what=f"{step}: listed against the twin")
        _assert_same(_state(bs), before, _rest(lst), _rest(lst), what=f"{step}: unlisted after the solve")


# ---- 6. shared sets: a change of finiteness in a listed row is refused ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_shared_sets_refuse_a_listed_row_that_changes_finiteness(hip, backend):
    fin, b1 = finite_sparse_batch(16, B), mixed_sparse_batch(16, B, 1)
    bs = _handle(hip, fin, _ks(hip, backend), "shared")
    bs.solve()
    lst = [2, 5]
    assert not np.isfinite(b1["h_l"][lst]).all() and not np.isfinite(b1["x_u"][lst]).all() and not np.isfinite(b1["x_l"][lst]).all()
    assert bs.update(instances=lst, c=fin["c"][lst])  # (the list buffer exists from here on)
    bs.solve(instances=lst)
    before = _state(bs)
    a0 = bs.L.pq_debug_alloc_count()
    bad_h, bad_d = {"h_l": b1["h_l"][lst]}, _torch({"h_l": b1["h_l"][lst]})
    for call in (lambda: bs.update(instances=lst, **bad_h), lambda: bs.update(instances=lst, **bad_d),
                 lambda: bs.update_data(instances=lst, G_values=b1["Gv"][lst], x_u=b1["x_u"][lst]),
                 lambda: bs.update_data(instances=lst, **_torch(dict(P_values=fin["Pv"][lst], x_l=b1["x_l"][lst])))):
        with pytest.raises(Exception, match=REFUSED):
            call()
        _assert_same(_state(bs), before, what="a refused update leaves every instance")
    assert bs.L.pq_debug_alloc_count() == a0
    # the check runs over the rows given: good rows pass whatever the other instances' rows would have been, from host and device memory
    assert bs.update(instances=lst, h_l=fin["h_l"][lst] - 0.01) and bs.update(instances=lst, **_torch({"h_u": fin["h_u"][lst] + 0.01}))
    _assert_same(_state(bs), before, _rest(lst), _rest(lst))


# ---- 7. results by list -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,data", COMBOS)
def test_result_by_list(hip, backend, data):
    bt = _batch(data)
    bs = _handle(hip, bt, _ks(hip, backend), "shared")
    bs.solve()
    whole = {k: bs.result(k) for k in FIELDS}
    # (30 entries of a batch of 12: more than the list buffer holds at once)
    for lst in (*LISTS.values(), [3, 3, 3], [0] * 20 + PERM[:10], np.array([11, 0, 11], dtype=np.int64)):
        for k in FIELDS:
            want = whole[k][np.asarray(lst)]
            got = bs.result(k, instances=lst)
            assert got.shape == want.shape and np.array_equal(got, want), (k, lst)
            dev = bs.result(k, device=True, instances=lst)
            assert tuple(dev.shape) == want.shape and np.array_equal(dev.cpu().numpy(), want), (k, lst)
    if data == "mpc":
        # m = 0: a field of length 0 writes nothing and returns 0
        assert bs.m == 0 and bs.result("z_l", instances=[7, 7]).shape == (2, 0) and tuple(bs.result("s_u", device=True, instances=[7]).shape) == (1, 0)
        idx, out = np.array([7, 1], dtype=np.intc), np.full(4, -7.0)
        for mem in (0, 1):
            assert bs.L.pq_batch_get_result_select_mem(bs.h, idx.ctypes.data, 2, 2, out.ctypes.data, mem) == 0
        assert out.tolist() == [-7.0] * 4


# ---- 8. refusals on a live handle --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle(hip):
    L = hip._lib.load()
    bt = _batch("dim16")
    bs = _handle(hip, bt, hip.SPARSE_LDLT, "per_instance")
    bs.solve()
    before = _state(bs)
    out = np.full(2 * bs.n, -7.0)
    vec = np.zeros((3, bs.n))

    def calls(idx, count):
        p = idx.ctypes.data if idx.size else None
        return {"pq_batch_solve_select": lambda: L.pq_batch_solve_select(bs.h, p, count),
                "pq_batch_update_select_mem": lambda: L.pq_batch_update_select_mem(bs.h, p, count, vec.ctypes.data, *[None] * 5, 0),
                "pq_batch_update_data_select_mem": lambda: L.pq_batch_update_data_select_mem(bs.h, p, count, *[None] * 3, vec.ctypes.data, *[None] * 5, 0),
                "pq_batch_get_result_select_mem": lambda: L.pq_batch_get_result_select_mem(bs.h, p, count, 0, out.ctypes.data, 0)}

    def refused(idx, count, *words, only=None):
        a0 = L.pq_debug_alloc_count()
        for fn, call in calls(np.asarray(idx, dtype=np.intc), count).items():
            if only and fn not in only:
                continue
            assert call() == -1, fn
            text = L.pq_last_error_string().decode()
            assert fn in text and all(w in text for w in words), text
        assert L.pq_debug_alloc_count() == a0 and (out == -7.0).all()

    refused([0, 1, -1], 3, "idx[2]", "-1")
    refused([0, B, 1], 3, "idx[1]", str(B))
    refused([0, 1], 0, "count", "0")
    refused([0, 1], -3, "count", "-3")
    refused([], 2, "idx")
    refused([4, 1, 4], 3, "idx[2]", "4", "twice", only=("pq_batch_solve_select", "pq_batch_update_select_mem", "pq_batch_update_data_select_mem"))
    assert L.pq_batch_arena_row(bs.h, B, out.ctypes.data) == -1 and str(B) in L.pq_last_error_string().decode()
    assert L.pq_batch_arena_row(bs.h, -1, out.ctypes.data) == -1
    with pytest.raises(RuntimeError, match=r"idx\[1\] = 12"):
        bs.solve(instances=[0, B])
    with pytest.raises(RuntimeError, match=r"idx\[0\] = -1"):
        bs.result("x", instances=[-1])
    with pytest.raises(ValueError, match="twice"):
        bs.update(instances=[1, 1], c=np.zeros((2, bs.n)))
    with pytest.raises(ValueError, match="shape"):
        bs.update(instances=[1, 2], c=_torch({"c": np.zeros((3, bs.n))})["c"])
    _assert_same(_state(bs), before, what="a refused call leaves every instance")
    # a handle that was never set up
    fresh = hip.BatchSparseSolver(kkt_solver=hip.SPARSE_LDLT)
    a0 = L.pq_debug_alloc_count()
    idx = np.array([0], dtype=np.intc)
    for rc in (L.pq_batch_solve_select(fresh.h, idx.ctypes.data, 1), L.pq_batch_update_select_mem(fresh.h, idx.ctypes.data, 1, *[None] * 6, 0),
               L.pq_batch_update_data_select_mem(fresh.h, idx.ctypes.data, 1, *[None] * 9, 0), L.pq_batch_get_result_select_mem(fresh.h, idx.ctypes.data, 1, 0, out.ctypes.data, 0),
               L.pq_batch_arena_row(fresh.h, 0, out.ctypes.data)):
        assert rc == -1 and "setup" in L.pq_last_error_string().decode()
    assert L.pq_debug_alloc_count() == a0 and (out == -7.0).all()


def test_invalid_settings_mark_the_listed_infos_alone(hip):
    bt = _batch("mpc")
    bs = _handle(hip, bt, hip.SPARSE_MULTISTAGE, "shared")
    bs.solve()
    before = _state(bs)
    lst = [10, 7, 4, 1]
    max_iter = bs.settings.max_iter
    bs.settings.max_iter = 0
    assert bs.solve(instances=lst) == 0
    assert (bs.statuses()[lst] == INVALID_SETTINGS).all() and (bs.iterations()[lst] == 0).all()
    after = _state(bs)
    _assert_same(after, before, _rest(lst), _rest(lst), what="unlisted")
    _assert_same({k: after[k] for k in (*FIELDS, "profile", "arena")}, before, what="no launch: the device holds what it held")
    bs.settings.max_iter = max_iter
    assert bs.solve(instances=lst) == len(lst)
    _assert_same({k: before[k] for k in FIELDS}, _held(bs), what="solved again in place")
    assert (bs.statuses() == SOLVED).all()


# ---- 9. allocation --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", ["shared", "per_instance"])
@pytest.mark.parametrize("backend,data", COMBOS)
def test_calls_by_list_allocate_nothing_after_the_first(hip, backend, data, bounds):
    bt = _batch(data)
    L = hip._lib.load()

    def allocs(make):
        a = L.pq_debug_alloc_count()
        h = make()
        return L.pq_debug_alloc_count() - a, h

    _, bs = allocs(lambda: _handle(hip, bt, _ks(hip, backend), bounds))
    per_setup, _ = allocs(lambda: _handle(hip, bt, _ks(hip, backend), bounds))
    per_clone, _ = allocs(bs.clone)
    bs.solve()
    lst = LISTS["descending"]
    b1 = _moved(bt, 3)
    vec = _torch({k: v[lst] for k, v in _vectors(b1).items()})
    mats = _torch({k: b1[s][lst] for k, s in (("P_values", "Pv"), ("A_values", "Av"), ("G_values", "Gv")) if b1.get(s) is not None})
    a0 = bs.L.pq_debug_alloc_count()
    bs.solve(instances=lst)
    assert bs.L.pq_debug_alloc_count() - a0 == 1, "one int buffer, made by the first call by list"
    assert bs.update(instances=lst, **vec) and bs.update_data(instances=lst, **mats, **vec)
    xs = [bs.result(k, device=True, instances=lst) for k in FIELDS]
    a0 = bs.L.pq_debug_alloc_count()
    for _ in range(3):
        assert bs.update(instances=lst, **vec)
        assert bs.update_data(instances=lst, **mats, **vec)
        bs.solve(instances=lst)
        xs = [bs.result(k, device=True, instances=lst) for k in FIELDS]
        bs.info(lst[0]), bs.profile(lst[0])
    assert bs.L.pq_debug_alloc_count() == a0, "update, update_data, solve and device results by list must not allocate"
    assert all(np.array_equal(x.cpu().numpy(), bs.result(k)[lst]) for k, x in zip(FIELDS, xs))
    # setup() and clone() allocate what they allocated before the handle had its list buffer: it is not made there, and a clone makes its own when it needs one
    assert allocs(lambda: _handle(hip, bt, _ks(hip, backend), bounds))[0] == per_setup
    n_clone, cl = allocs(bs.clone)
    assert n_clone == per_clone
    assert allocs(lambda: cl.solve(instances=lst))[0] == 1 and allocs(lambda: cl.solve(instances=lst))[0] == 0


# ---- 10. stragglers, in place -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,data", COMBOS)
def test_stragglers_are_solved_again_in_place(hip, backend, data):
    bt = _batch(data)
    ks = _ks(hip, backend)
    hi = _handle(hip, bt, ks, "shared")
    want = _solved(hi)
    its = hi.iterations()
    assert (hi.statuses() == SOLVED).all()
    low = _handle(hip, bt, ks, "shared", max_iter=int(its.max()) - 1)
    low.solve()
    late = np.flatnonzero(low.statuses() != SOLVED)
    assert len(late) >= 1 and (low.statuses()[late] == MAX_ITER_REACHED).all()
    before = _state(low)
    low.settings.max_iter = hi.settings.max_iter
    assert low.solve(instances=late) == len(late)
    assert (low.statuses() == SOLVED).all()
    _assert_same(_held(low), want, late, late, what="stragglers against a handle with the high limit")
    _assert_same(_state(low), before, _rest(late), _rest(late), what="the others keep their first solve")
    _assert_same(_held(low), want, what="one handle, one set of results")
    # ---- 11. a clone taken now carries the mixed state
    cl = low.clone()
    _assert_same(_state(cl), _state(low), what="a clone after a solve by list")
    sub = low.clone(late)
    _assert_same(_state(sub), _state(low), None, late, what="a clone of the stragglers")
    _assert_same(_solved(cl), want, what="the clone's whole solve")
    _assert_same(_solved(low), want, what="the handle's whole solve")
