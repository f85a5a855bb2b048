"""CPU-only checks of the clones of the batched sparse solver (include/piqp_amd.h: pq_batch_clone, pq_batch_clone_select, pq_batch_clone_ms;
piqp_amd.BatchSparseSolver.clone(instances)).  A pq_batch cannot exist without a device (pq_batch_create refuses), so what can be asked here is what is refused
before the handle is looked at -- a NULL handle, a NULL out -- and what the Python wrapper refuses before it calls the library.  The refusals that need a live handle
(idx, count, a handle that was never set up) are in tests/test_batch_sparse_clone_gpu.py."""
import ctypes as C

import numpy as np
import pytest

PQ_ERR_INVALID = -1
SENTINEL = 0x5A5A
IDX = np.array([0, 0], dtype=np.intc)


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


def refused(L, rc, out=None):
    assert rc == PQ_ERR_INVALID
    assert L.pq_last_error_string().decode() != ""
    if out is not None:
        assert out.value == SENTINEL, "*out must be left untouched"


def test_a_null_handle_is_refused_by_both_clones_and_out_is_left_alone(L):
    out = C.c_void_p(SENTINEL)
    refused(L, L.pq_batch_clone(None, C.byref(out)), out)
    refused(L, L.pq_batch_clone_select(None, IDX.ctypes.data, 2, C.byref(out)), out)


def test_a_null_out_is_refused_by_both_clones(L):
    # (the handle is not looked at before out is: any non-NULL value stands for it)
    fake = C.c_void_p(SENTINEL)
    refused(L, L.pq_batch_clone(fake, None))
    refused(L, L.pq_batch_clone_select(fake, IDX.ctypes.data, 2, None))


def test_clone_ms_of_a_null_handle_is_refused(L):
    o = np.full(2, -7.0)
    refused(L, L.pq_batch_clone_ms(None, o.ctypes.data))
    assert o.tolist() == [-7.0, -7.0]
    refused(L, L.pq_batch_arena_stride(None))


def test_the_python_wrapper_refuses_a_bad_list_before_any_library_call():
    """the lists of tests/test_batch_clone_abi.py::test_the_python_wrappers_refuse_a_bad_list_before_any_library_call, on that test's object with a stub library"""
    import piqp_amd

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"library call {name}")

    bad = ([], np.zeros((2, 2), dtype=np.intc), [[0, 1], [1, 0]], [0.5, 1.0], np.array([1.0]), ["a"], 3, [True, False], [[0], [1, 2]])
    k = piqp_amd.BatchSparseSolver.__new__(piqp_amd.BatchSparseSolver)
    k._owned = False
    k.L, k.h, k.device, k.bounds = NoLibrary(), C.c_void_p(1), 0, "shared"
    k.batch, k.n, k.p, k.m, k._nnz = 4, 3, 1, 0, (3, 3, 0)
    for inst in bad:
        with pytest.raises(ValueError):
            k.clone(inst)
