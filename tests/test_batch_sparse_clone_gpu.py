"""Clones of the batched sparse solver (BatchSparseSolver.clone(instances); pq_batch_clone, pq_batch_clone_select, pq_batch_clone_ms; batch_solver.hip).

The yardstick: instance j of the clone IS instance idx[j] of the source, bit for bit, and after the same later calls on both handles they stay equal -- the ten result
vectors and every info field that is not a time (_solved / _assert_same of tests/test_batch_bounds_gpu.py).  The source is in turn held to the CPU oracle by
_compare_solves of tests/test_batch_ldlt_gpu.py with its tolerances; no tolerance is introduced here.  Both backends (sparse_multistage, sparse_ldlt) unless a test says
otherwise, batches of 12.  Inputs: mpc_batch(12) (the wave-per-QP kernel mode, p > 0, m = 0, boxes), _random_sparse_qp_batch(16, 12) (A, G, boxes, shared
infinities), mixed_sparse_batch(16, 12) (lists per instance), an MPC batch of n = 540 (the 256-thread kernel).  The arena's stride is even at every shape (every slot
is padded to an even count), so 16-byte words are the gather every test here takes; the 8-byte words of an odd stride are held in a worker process
(tests/workers/batch_clone_words.py) through PIQP_AMD_DEBUG=batch_clone_words=8."""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

from batch_sparse_mixed import finite_sparse_batch, mixed_sparse_batch, sub_batch
from qp_gen import mpc_batch
from test_batch_bounds_gpu import FIELDS, _assert_same, _handle, _moved, _mpc_as_batch, _solved, _vectors
from test_batch_ldlt_gpu import _compare_solves, _random_sparse_qp_batch, _scalings

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 12
BACKENDS = ["multistage", "ldlt"]
DATA = ["mpc", "dim16"]
PERM = [5, 0, 11, 3, 8, 1, 10, 2, 7, 4, 9, 6]
LISTS = {"identity": None, "permutation": PERM, "fanout": [0] * 20, "single": [7], "subset_descending": [10, 7, 4, 1]}
SOLVED, MAX_ITER_REACHED = 1, -1
SENTINEL = 0x5A5A

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


def _idx(lst, batch=B):
    return np.arange(batch) if lst is None else np.asarray(lst)


def _torch(d):
    import torch
    out = {k: torch.tensor(v, dtype=torch.float64, device="cuda:0") for k, v in d.items() if v is not None}
    torch.cuda.synchronize()
    return out


def _all_info(bs):
    """every field of every pq_info, the times included (a clone copies them)"""
    names = [f for f, _ in type(bs.info(0))._fields_]
    return np.array([[getattr(bs.info(i), f) for f in names] for i in range(bs.batch)], dtype=np.float64)


# ---- 1. a clone of a handle that has not solved -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lst", list(LISTS))
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("backend", BACKENDS)
def test_clone_of_an_unsolved_handle_solves_to_the_sources_bits(hip, orc, backend, data, lst):
    bt = _batch(data)
    src, twin = _handle(hip, bt, _ks(hip, backend), "shared"), _handle(hip, bt, _ks(hip, backend), "shared")
    cl = src.clone(LISTS[lst])
    idx = _idx(LISTS[lst])
    assert (cl.batch, cl.n, cl.p, cl.m, cl._nnz, cl.bounds, cl.device) == (len(idx), src.n, src.p, src.m, src._nnz, src.bounds, src.device)
    assert cl.arena_stride() == src.arena_stride() > 0 and src.arena_stride() % 2 == 0, "rows of the arena are 16-byte aligned: the gather's wide words"
    assert all(cl.info(j).status == src.info(0).status and cl.info(j).iter == 0 for j in range(cl.batch))
    ms = cl.clone_ms()
    assert ms["wall_ms"] > 0 and ms["device_ms"] > 0 and src.clone_ms() == dict(wall_ms=0.0, device_ms=0.0)
    got, ref = _solved(cl), _solved(src)
    _assert_same(got, ref, None, idx, what="clone against its source")
    _assert_same(ref, _solved(twin), what="the source against an untouched twin")
    if lst == "identity":
        _compare_solves(src, orc, bt, idx=range(0, B, 5), kkt_solver=_oks(orc, backend))


def test_clone_of_the_256_thread_kernel_shape(hip):
    """n = 540 > 512: 256 threads per QP (the staged / global-memory chain modes), rows of the arena of several chunks"""
    mb = mpc_batch(B, T=180, nx=2, nu=1, seed=77)
    bt = dict(P=mb["P_pattern"], Pv=mb["P_values"], c=mb["c"], A=mb["A_pattern"], Av=mb["A_values"], b=mb["b"], G=None, Gv=None, h_l=None, h_u=None, x_l=mb["x_l"],
              x_u=mb["x_u"], B=B)
    src = _handle(hip, bt, hip.SPARSE_MULTISTAGE, "shared")
    assert src.last_kernel_ms()[1] == 256
    ref = _solved(src)
    cl = src.clone(PERM)
    assert cl.last_kernel_ms()[1] == 256
    assert all(np.array_equal(cl.result(k), ref[k][PERM]) for k in FIELDS)
    _assert_same(_solved(cl), ref, None, PERM)
    b1 = _moved(bt, 1)
    assert cl.update_data(P_values=b1["Pv"][PERM], A_values=b1["Av"][PERM], **_vectors(sub_batch(b1, PERM))) and src.update_data(P_values=b1["Pv"], A_values=b1["Av"], **_vectors(b1))
    _assert_same(_solved(cl), _solved(src), None, PERM, what="update_data")


# ---- 2. a clone after a solve answers without solving -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lst", list(LISTS))
@pytest.mark.parametrize("backend,data", [("multistage", "mpc"), ("multistage", "dim16"), ("ldlt", "dim16")])
def test_clone_after_a_solve_answers_without_solving_and_allocates_nothing_later(hip, backend, data, lst):
    bt = _batch(data)
    src = _handle(hip, bt, _ks(hip, backend), "shared")
    src.solve()
    cl = src.clone(LISTS[lst])
    idx = _idx(LISTS[lst])
    assert np.array_equal(_all_info(cl), _all_info(src)[idx], equal_nan=True)
    assert np.array_equal(cl.iterations(), src.iterations()[idx]) and np.array_equal(cl.statuses(), src.statuses()[idx])
    for k in FIELDS:
        want = src.result(k)[idx]
        assert np.array_equal(cl.result(k), want), k
        assert np.array_equal(cl.result(k, device=True).cpu().numpy(), want), k
    for j, i in enumerate(idx):
        assert cl.profile(j) == src.profile(int(i)), j
    # later calls allocate nothing: vectors from device memory (a host-fed update stages its vectors in fresh buffers on every handle, a clone or not)
    sub = _torch(_vectors(sub_batch(_moved(bt, 3), idx)))
    a0 = cl.L.pq_debug_alloc_count()
    assert cl.update(**sub)
    cl.solve()
    xs = [cl.result(k, device=True) for k in FIELDS]
    for j in (0, cl.batch - 1):
        cl.info(j), cl.profile(j)
    assert cl.L.pq_debug_alloc_count() == a0, "update, solve and the getters of a clone must not allocate"
    assert all(np.array_equal(x.cpu().numpy(), cl.result(k)) for k, x in zip(FIELDS, xs))


# ---- 3. updates on a clone --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("reuse", [0, 1])
@pytest.mark.parametrize("backend,data", [("multistage", "mpc"), ("multistage", "dim16"), ("ldlt", "dim16")])
def test_updates_on_a_clone_are_the_sources_updates(hip, backend, data, reuse, mem):
    """update(vectors), then update_data(matrices + vectors): the clone fed sub_batch(new, idx), the source and its twin fed new.  The clones are updated FIRST, and
    the source's solve in between equals the twin's: nothing an update of a clone does reaches the source."""
    bt = _batch(data)
    ks = _ks(hip, backend)
    # (reuse = 1 also scales the cost, so the stored cost scaling an update unscales with is not 1)
    src, twin = (_handle(hip, bt, ks, "shared", preconditioner_reuse_on_update=reuse, preconditioner_scale_cost=reuse) for _ in range(2))
    src.solve(); twin.solve()
    clones = {name: src.clone(LISTS[name]) for name in ("permutation", "fanout", "subset_descending")}
    feed = (lambda d: _torch(d)) if mem == "device" else (lambda d: {k: v for k, v in d.items() if v is not None})
    b1 = _moved(bt, 1)
    b2 = _moved(b1, 2)

    def vec_args(b):
        return feed(_vectors(b))

    def data_args(b):
        return feed(dict(P_values=b["Pv"], A_values=b["Av"], G_values=b["Gv"], **_vectors(b)))

    for step, b, args in (("update", b1, vec_args), ("update_data", b2, data_args)):
        call = (lambda s, a: s.update(**a)) if step == "update" else (lambda s, a: s.update_data(**a))
        for name, cl in clones.items():
            assert call(cl, args(sub_batch(b, _idx(LISTS[name]))))
        _assert_same(_solved(src), _solved(twin), what=f"{step}: the source after its clones were updated")
        assert call(src, args(b)) and call(twin, args(b))
        ref = _solved(src)
        _assert_same(ref, _solved(twin), what=f"{step}: source against twin")
        for name, cl in clones.items():
            _assert_same(_solved(cl), ref, None, _idx(LISTS[name]), what=f"{step}: clone {name}")


# ---- 4. sets of finite bounds per instance ------------------------------------------------------------------------------------------------------------------------
def _same_lists(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("lst", [PERM, [3, 0, 3, 4, 0], [0] * 20], ids=["permutation", "dropped_next_to_kept", "fanout"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_per_instance_lists_go_with_their_instances(hip, backend, lst):
    """instance 3 of the mixed batch has every row of G dropped, instance 4 no finite bound at all, instance 0 every bound: a clone takes each instance's row of the
    table, `dropped` included, and the update that brings the rows back (bounds of salt 1 with G values) is bitwise the source's"""
    b0, b1 = mixed_sparse_batch(16, B), mixed_sparse_batch(16, B, 1)
    src = _handle(hip, b0, _ks(hip, backend), "per_instance")
    assert src.bound_lists(3)["dropped"].all() and not src.bound_lists(0)["dropped"].any()
    ref = _solved(src)
    cl = src.clone(lst)
    assert cl.bounds == "per_instance"
    for j, i in enumerate(lst):
        assert _same_lists(cl.bound_lists(j), src.bound_lists(i)), j
    _assert_same(_solved(cl), ref, None, lst, what="setup")
    given = dict(G_values=b1["Gv"], h_l=b1["h_l"], h_u=b1["h_u"], x_l=b1["x_l"], x_u=b1["x_u"])
    before = [src.bound_lists(i) for i in range(B)]
    assert cl.update_data(**{k: v[lst] for k, v in given.items()})
    assert all(_same_lists(src.bound_lists(i), before[i]) for i in range(B)), "the source's table is its own"
    assert not all(_same_lists(cl.bound_lists(j), before[i]) for j, i in enumerate(lst)), "the case is to change the clone's lists"
    assert src.update_data(**given)
    for j, i in enumerate(lst):
        assert _same_lists(cl.bound_lists(j), src.bound_lists(i)), j
    _assert_same(_solved(cl), _solved(src), None, lst, what="update_data that brings rows back")
    # vectors only, on the clone alone, then the source: the tables stay apart
    assert cl.update(h_l=b0["h_l"][lst], h_u=b0["h_u"][lst])
    got = _solved(cl)
    assert src.update(h_l=b0["h_l"], h_u=b0["h_u"])
    _assert_same(got, _solved(src), None, lst, what="update of the row bounds")


@pytest.mark.parametrize("backend", BACKENDS)
def test_shared_mode_clone_refuses_a_change_of_finiteness_with_its_own_flag_word(hip, backend):
    fin, b1 = finite_sparse_batch(16, B), mixed_sparse_batch(16, B, 1)
    src = _handle(hip, fin, _ks(hip, backend), "shared")
    cl = src.clone(PERM)
    text = "batch update: the set of finite bounds differs from the one given at setup"
    bad_h, bad_d = {"h_l": b1["h_l"][PERM]}, _torch({"h_l": b1["h_l"][PERM]})
    ok_d = _torch({"h_l": fin["h_l"][PERM] - 0.01})
    for call in (lambda: cl.update(**bad_h), lambda: cl.update(**bad_d), lambda: cl.update_data(G_values=b1["Gv"][PERM], x_u=b1["x_u"][PERM])):
        with pytest.raises(Exception, match=text):
            call()
    # the flag the clone's device check raised is the clone's: the source's device check of good vectors passes, and so does the clone's next one
    assert src.update(**_torch({"h_l": fin["h_l"] - 0.01}))
    assert cl.update(**ok_d)
    _assert_same(_solved(cl), _solved(src), None, PERM)
    del src
    gc.collect()
    with pytest.raises(Exception, match=text):
        cl.update(**bad_d)
    assert cl.update(**ok_d)


# ---- 5. the factor of the sparse_ldlt backend ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lst", ["permutation", "fanout", "single"])
def test_ldlt_factor_goes_with_the_clone(hip, lst):
    bt = _batch("dim16")
    src = _handle(hip, bt, hip.SPARSE_LDLT, "shared")
    n, p, m = src.n, src.p, src.m
    rng = np.random.default_rng(5)
    sc = [_scalings(n, m, rng, False) for _ in range(B)]
    assert src.kkt_factor(np.array([s[0] for s in sc]), np.array([s[1] for s in sc]).reshape(B, n), np.array([s[2] for s in sc]).reshape(B, m)).all()
    idx = _idx(LISTS[lst])
    cl = src.clone(LISTS[lst])
    for j, i in enumerate(idx):
        fc, fs = cl.ldlt_factor(j), src.ldlt_factor(int(i))
        assert sorted(fc) == sorted(fs) and all(np.array_equal(fc[k], fs[k]) for k in fs), j
    rx, ry, rz = rng.standard_normal((B, n)), rng.standard_normal((B, p)), rng.standard_normal((B, m))
    want = src.kkt_solve(rx, ry, rz)
    got = cl.kkt_solve(rx[idx], ry[idx], rz[idx])
    assert all(np.array_equal(g, w[idx]) for g, w in zip(got, want))


# ---- 6. lifetimes -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,data", [("multistage", "mpc"), ("ldlt", "dim16")])
def test_a_clone_outlives_its_source_and_a_new_setup_of_it(hip, backend, data):
    bt = _batch(data)
    ks = _ks(hip, backend)
    twin = _handle(hip, bt, ks, "shared")
    b1 = _moved(bt, 1)
    # (a) the source is destroyed first
    src = _handle(hip, bt, ks, "shared")
    src.solve()
    cl = src.clone(PERM)
    del src
    gc.collect()
    _assert_same(_solved(cl), _solved(twin), None, PERM, what="after the source went")
    assert cl.update(**_vectors(sub_batch(b1, PERM))) and twin.update(**_vectors(b1))
    _assert_same(_solved(cl), _solved(twin), None, PERM, what="update after the source went")
    # (b) the source is set up again with a problem of another size, and the reverse: a clone's source set up again, then the clone goes
    src = _handle(hip, bt, ks, "shared")
    cl = src.clone([0] * 20)
    other = _random_sparse_qp_batch(64, 5, seed=64) if data == "dim16" else _mpc_as_batch(5)
    if data == "mpc":
        mb = mpc_batch(5, T=12, nx=3, nu=2, seed=77)
        other = dict(P=mb["P_pattern"], Pv=mb["P_values"], c=mb["c"], A=mb["A_pattern"], Av=mb["A_values"], b=mb["b"], G=None, Gv=None, h_l=None, h_u=None,
                     x_l=mb["x_l"], x_u=mb["x_u"], B=5)
    assert src.setup(other["P"], other["Pv"], other["c"], other["A"], other["Av"], other["b"], other["G"], other["Gv"], other["h_l"], other["h_u"], other["x_l"], other["x_u"])
    assert src.n != cl.n
    fresh = _handle(hip, other, ks, "shared")
    twin0 = _handle(hip, bt, ks, "shared")
    _assert_same(_solved(cl), _solved(twin0), None, [0] * 20, what="the clone after a new setup of its source")
    _assert_same(_solved(src), _solved(fresh), what="the source after its new setup")
    del cl
    gc.collect()
    _assert_same(_solved(src), _solved(fresh), what="the source after its clone went")


@pytest.mark.parametrize("backend,data", [("multistage", "mpc"), ("ldlt", "dim16")])
def test_a_clone_of_a_clone_and_two_clones_interleaved(hip, backend, data):
    bt = _batch(data)
    ks = _ks(hip, backend)
    src = _handle(hip, bt, ks, "shared")
    ref = _solved(src)
    first = src.clone(PERM)
    second = first.clone([3, 3, 0])
    both = np.asarray(PERM)[[3, 3, 0]]
    del first
    gc.collect()
    assert all(np.array_equal(second.result(k), ref[k][both]) for k in FIELDS)
    _assert_same(_solved(second), ref, None, both, what="a clone of a clone")
    # two clones, calls interleaved: each is updated with other data, then both solve, then both are read
    a, b = src.clone([1, 2, 3]), src.clone([3, 2, 1, 0])
    ba, bb = _moved(bt, 4), _moved(bt, 5)
    assert a.update(**_vectors(sub_batch(ba, [1, 2, 3])))
    assert b.update_data(P_values=bb["Pv"][[3, 2, 1, 0]], **_vectors(sub_batch(bb, [3, 2, 1, 0])))
    a.solve(); b.solve()
    ra, rb = {k: a.result(k) for k in FIELDS}, {k: b.result(k) for k in FIELDS}
    ta, tb = _handle(hip, bt, ks, "shared"), _handle(hip, bt, ks, "shared")
    ta.solve(); tb.solve()
    assert ta.update(**_vectors(ba)) and tb.update_data(P_values=bb["Pv"], **_vectors(bb))
    wa, wb = _solved(ta), _solved(tb)
    assert all(np.array_equal(ra[k], wa[k][[1, 2, 3]]) and np.array_equal(rb[k], wb[k][[3, 2, 1, 0]]) for k in FIELDS)
    _assert_same(_solved(src), ref, what="the source after all of it")


# ---- 7. stragglers ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,data", [("multistage", "mpc"), ("multistage", "dim16"), ("ldlt", "dim16")])
def test_stragglers_are_solved_again_on_a_clone(hip, backend, data):
    """a solve starts from the data, not from the last iterate (k_batch_ipm runs the reference's solve_impl from its start), so a straggler solved again with a higher
    limit is the instance of a handle that had the high limit from the start"""
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
    done = {k: low.result(k) for k in FIELDS}
    cl = low.clone(late)
    assert cl.settings.max_iter == int(its.max()) - 1
    cl.settings.max_iter = hi.settings.max_iter
    got = _solved(cl)
    assert (cl.statuses() == SOLVED).all()
    _assert_same(got, want, None, late, what="stragglers against a handle with the high limit")
    assert low.settings.max_iter == int(its.max()) - 1 and all(np.array_equal(low.result(k), done[k]) for k in FIELDS), "the source is as it was"


# ---- 8. scenario fan-out ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,data", [("multistage", "mpc"), ("multistage", "dim16"), ("ldlt", "dim16")])
def test_fan_out_equals_a_handle_set_up_from_the_nominal_instance(hip, backend, data):
    """clone([0] * 20) and 20 right-hand sides b: bitwise a 20-instance handle set up from instance 0's data and given the same update (an instance does not depend on
    the batch it is in: test_batch_ldlt_gpu.py::test_instances_do_not_interact, test_batch_gpu.py::test_chain_shapes_match_the_oracle_in_both_kernel_variants) -- with
    both backends"""
    bt = _batch(data)
    ks = _ks(hip, backend)
    S = 20
    src = _handle(hip, bt, ks, "shared")
    cl = src.clone([0] * S)
    rng = np.random.default_rng(8)
    b_new = bt["b"][0][None, :] * (1 + 0.01 * rng.uniform(-1, 1, (S, bt["b"].shape[1])))
    ref = _handle(hip, sub_batch(bt, [0] * S), ks, "shared")
    assert cl.update(b=b_new) and ref.update(b=b_new)
    got = _solved(cl)
    _assert_same(got, _solved(ref), what="fan-out")
    assert len({got["x"][j].tobytes() for j in range(S)}) == S, "20 scenarios, 20 answers"


# ---- 9. start order -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_start_order_of_a_clone_changes_no_bit(hip, backend):
    """600 MPC QPs: more than one workgroup per compute unit, iteration counts that differ.  The whole clone of a solved handle starts its longest instances first
    (the order is computed from its gathered infos); index order and longest-first again leave every bit"""
    bt = _mpc_as_batch(600)
    src = _handle(hip, bt, _ks(hip, backend), "shared")
    ref = _solved(src)
    assert len(set(src.iterations().tolist())) > 1
    cl = src.clone()
    _assert_same(_solved(cl), ref, what="longest first, from the gathered infos")
    cl.set_start_order(False)
    _assert_same(_solved(cl), ref, what="index order")
    cl.set_start_order(True)
    _assert_same(_solved(cl), ref, what="longest first again: the order of the solve before")
    _assert_same(_solved(cl), ref, what="and once more")
    off = src.clone(np.arange(599, -1, -1))
    _assert_same(_solved(off), ref, None, np.arange(599, -1, -1), what="a reversed clone")


# ---- 10. refusals on a live handle, and what is copied ------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle_and_the_copied_scalars(hip):
    L = hip._lib.load()
    bt = _batch("dim16")
    src = _handle(hip, bt, hip.SPARSE_LDLT, "per_instance", max_iter=77, eps_abs=3.5e-7)
    out = C.c_void_p(SENTINEL)

    def refused(idx, count, *words):
        a = np.asarray(idx, dtype=np.intc)
        a0 = L.pq_debug_alloc_count()
        assert L.pq_batch_clone_select(src.h, a.ctypes.data if a.size else None, count, C.byref(out)) == -1
        text = L.pq_last_error_string().decode()
        assert all(w in text for w in words), text
        assert out.value == SENTINEL and L.pq_debug_alloc_count() == a0

    refused([0, 1, -1], 3, "idx[2]", "-1")
    refused([0, B, 1], 3, "idx[1]", str(B))
    refused([0, 1], 0, "count", "0")
    refused([0, 1], -3, "count", "-3")
    refused([], 2, "idx")
    with pytest.raises(RuntimeError, match=r"idx\[1\] = 12"):
        src.clone([0, B])
    with pytest.raises(ValueError):
        src.clone([])
    # a handle that was never set up: _clone gives the scalars and no problem, _clone_select is refused
    fresh = hip.BatchSparseSolver(kkt_solver=hip.SPARSE_LDLT, bounds="per_instance")
    fresh.settings.max_iter = 55
    a = np.array([0], dtype=np.intc)
    assert L.pq_batch_clone_select(fresh.h, a.ctypes.data, 1, C.byref(out)) == -1 and "setup" in L.pq_last_error_string().decode() and out.value == SENTINEL
    empty = fresh.clone()
    assert (empty.settings.max_iter, empty.settings.kkt_solver, empty.batch) == (55, hip.SPARSE_LDLT, 0)
    assert empty.clone_ms() == dict(wall_ms=0.0, device_ms=0.0)
    with pytest.raises(RuntimeError, match="not set up"):
        empty.solve()
    mixed = mixed_sparse_batch(16, B)
    assert empty.setup(mixed["P"], mixed["Pv"], mixed["c"], mixed["A"], mixed["Av"], mixed["b"], mixed["G"], mixed["Gv"], mixed["h_l"], mixed["h_u"], mixed["x_l"], mixed["x_u"]), \
        "the bound-set mode went along: a shared-mode handle refuses this batch"
    # the copied scalars of a live handle
    cl = src.clone([2, 1])
    dims = [C.c_int() for _ in range(4)]
    assert L.pq_batch_dims(cl.h, *[C.byref(d) for d in dims]) == 0 and [d.value for d in dims] == [2, src.n, src.p, src.m]
    assert (cl.settings.max_iter, cl.settings.eps_abs, cl.settings.kkt_solver, cl.bounds) == (77, 3.5e-7, hip.SPARSE_LDLT, "per_instance")
    cl.settings.max_iter = 5
    src.settings.eps_abs = 1e-6
    assert src.settings.max_iter == 77 and cl.settings.eps_abs == 3.5e-7
    assert cl.update(h_l=np.full((2, src.m), -np.inf)), "lists per instance: the clone takes a change of finiteness"


# ---- the two word widths of the arena gather ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", [16, 8])
def test_arena_gather_in_both_word_widths(tmp_path, words):
    """one process per width (PIQP_AMD_DEBUG is parsed once per process): the worker clones, compares bit for bit and reports the width the library took"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PIQP_AMD_")}
    env["PIQP_AMD_DEBUG"] = "batch_clone_info" + (",batch_clone_words=8" if words == 8 else "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "workers", "batch_clone_words.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stderr.splitlines() if "batch clone:" in ln]
    assert len(lines) == 6 and all(f"in {words}-byte words" in ln for ln in lines), lines
