"""CPU-only checks of the clones of the batched dense stack (include/piqp_amd.h: pq_kkt_batch_clone_select, pq_kktsys_batch_clone_select, pq_solver_batch_clone,
pq_solver_batch_clone_select; piqp_amd.BatchDenseKKT / BatchKKTSystem / BatchDenseSolver .clone(instances)).  Every refusal is made before the device is touched, so on
a machine without a GPU it comes back as PQ_ERR_INVALID with a text and never as a HIP error, and *out is left as it was.  The only handle that exists without a device
is a pq_solver_batch that was never set up: the refusals that need a batch to compare with (an index out of range, and every refusal of the two lower layers beyond the
NULL handle and the NULL out) are in tests/test_batch_clone_gpu.py."""
import ctypes as C

import numpy as np
import pytest

PQ_ERR_INVALID = -1
PQ_UNSOLVED = -9
SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


@pytest.fixture()
def fresh(L):
    h = C.c_void_p()
    assert L.pq_solver_batch_create(C.byref(h), 0) == 0
    yield h
    L.pq_solver_batch_destroy(h)


def refused(L, rc, out):
    assert rc == PQ_ERR_INVALID
    assert L.pq_last_error_string().decode() != ""
    assert out.value == SENTINEL, "*out must be left untouched"


IDX = np.array([0, 0], dtype=np.intc)


@pytest.mark.parametrize("fn", ["pq_kkt_batch_clone_select", "pq_kktsys_batch_clone_select", "pq_solver_batch_clone_select"])
def test_a_null_handle_or_a_null_out_is_refused_in_every_layer(L, fresh, fn):
    out = C.c_void_p(SENTINEL)
    refused(L, getattr(L, fn)(None, IDX.ctypes.data, 2, C.byref(out)), out)
    if fn == "pq_solver_batch_clone_select":
        assert getattr(L, fn)(fresh, IDX.ctypes.data, 2, None) == PQ_ERR_INVALID and L.pq_last_error_string().decode() != ""


def test_clone_of_a_null_handle_or_into_a_null_out(L, fresh):
    out = C.c_void_p(SENTINEL)
    refused(L, L.pq_solver_batch_clone(None, C.byref(out)), out)
    assert L.pq_solver_batch_clone(fresh, None) == PQ_ERR_INVALID and L.pq_last_error_string().decode() != ""


def test_a_null_list_and_a_count_below_one_are_refused_with_their_own_texts(L, fresh):
    out = C.c_void_p(SENTINEL)
    refused(L, L.pq_solver_batch_clone_select(fresh, None, 2, C.byref(out)), out)
    assert "idx" in L.pq_last_error_string().decode()
    for count in (0, -1):
        refused(L, L.pq_solver_batch_clone_select(fresh, IDX.ctypes.data, count, C.byref(out)), out)
        assert "count" in L.pq_last_error_string().decode() and str(count) in L.pq_last_error_string().decode()


def test_clone_select_of_a_handle_that_was_never_set_up_is_refused(L, fresh):
    out = C.c_void_p(SENTINEL)
    refused(L, L.pq_solver_batch_clone_select(fresh, IDX.ctypes.data, 2, C.byref(out)), out)
    assert "setup" in L.pq_last_error_string().decode()


def test_clone_of_a_handle_that_was_never_set_up_copies_its_scalars(L, fresh):
    s = L.pq_solver_batch_settings(fresh).contents
    s.max_iter, s.eps_abs, s.kkt_solver = 77, 3.5e-7, 16
    assert L.pq_solver_batch_set_trace(fresh, 19) == 0
    assert L.pq_solver_batch_set_bound_sets(fresh, 1) == 0
    a0 = L.pq_debug_alloc_count()
    c = C.c_void_p()
    assert L.pq_solver_batch_clone(fresh, C.byref(c)) == 0 and c.value
    try:
        assert L.pq_debug_alloc_count() == a0, "no device is touched"
        cs = L.pq_solver_batch_settings(c).contents
        assert (cs.max_iter, cs.eps_abs, cs.kkt_solver) == (77, 3.5e-7, 16)
        # there is no problem in it: it answers as a fresh handle does
        assert L.pq_solver_batch_dims(c, None, None, None, None) == PQ_ERR_INVALID
        assert L.pq_solver_batch_info(c, 0).contents.status == PQ_UNSOLVED
        assert L.pq_solver_batch_solve(c) == PQ_ERR_INVALID and "before setup" in L.pq_last_error_string().decode()
        out = C.c_void_p(SENTINEL)
        refused(L, L.pq_solver_batch_clone_select(c, IDX.ctypes.data, 2, C.byref(out)), out)
        # the two settings structs are independent
        cs.max_iter = 5
        s.eps_abs = 1.0
        assert L.pq_solver_batch_settings(fresh).contents.max_iter == 77 and L.pq_solver_batch_settings(c).contents.eps_abs == 3.5e-7
        # trace rows and bound-set mode have no getter: a clone of the clone, made through the Python wrapper's eyes, is checked on the GPU (a setup reads them);
        # here: the calls that set them still work on the clone and leave the source alone
        assert L.pq_solver_batch_set_trace(c, 4) == 0 and L.pq_solver_batch_set_bound_sets(c, 0) == 0
    finally:
        L.pq_solver_batch_destroy(c)
    # the source survives its clone
    assert L.pq_solver_batch_settings(fresh).contents.max_iter == 77


def test_the_python_wrappers_refuse_a_bad_list_before_any_library_call():
    import piqp_amd
    from piqp_amd.batch_kkt import select_list

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"library call {name}")

    bad = ([], np.zeros((2, 2), dtype=np.intc), [[0, 1], [1, 0]], [0.5, 1.0], np.array([1.0]), ["a"], 3, [True, False], [[0], [1, 2]])
    for cls in (piqp_amd.BatchDenseKKT, piqp_amd.BatchKKTSystem, piqp_amd.BatchDenseSolver):
        k = cls.__new__(cls)
        k._owned = False
        k.L, k.h, k.device, k.kkt_solver, k.lists, k.per_inst, k.bounds = NoLibrary(), C.c_void_p(1), 0, 0, None, False, "shared"
        for inst in bad:
            with pytest.raises(ValueError):
                k.clone(inst)
    for good in ([3, 0, 0], (1,), np.array([2, 1], dtype=np.int64), range(4)):
        a = select_list(good)
        assert a.dtype == np.intc and a.ndim == 1 and a.flags.c_contiguous and a.tolist() == list(good)
