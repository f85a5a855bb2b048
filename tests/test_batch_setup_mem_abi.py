"""CPU-only checks of pq_batch_setup_sparse_mem, pq_batch_last_ingest and pq_batch_setup_ms (include/piqp_amd.h) and of the argument handling of
piqp_amd.BatchSparseSolver.setup() for data in GPU memory.  No pq_batch exists without a device, so what can be held here is what is refused before the device is
touched: a NULL handle, a NULL out -- with out left as it was -- and a tensor the wrapper must not hand to the library.  The rest is in
tests/test_batch_setup_mem_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

PQ_ERR_INVALID = -1
MEM_HOST, MEM_DEVICE = 0, 1


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


def test_the_three_symbols_are_exported_and_declared(L):
    import os
    import piqp_amd
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(piqp_amd.__file__))), "include", "piqp_amd.h")).read()
    for name in ("pq_batch_setup_sparse_mem", "pq_batch_last_ingest", "pq_batch_setup_ms"):
        assert getattr(L, name) is not None
        assert name in piqp_amd._lib.SYMBOLS and f"int {name}(" in header


def test_a_null_handle_is_refused_by_setup_in_either_memory(L):
    Pp, Pi = np.array([0, 1], dtype=np.intc), np.array([0], dtype=np.intc)
    Px, c = np.ones((1, 1)), np.ones((1, 1))
    a0 = L.pq_debug_alloc_count()
    for mem in (MEM_HOST, MEM_DEVICE, 7):
        rc = L.pq_batch_setup_sparse_mem(None, 1, 1, 0, 0, Pp.ctypes.data, Pi.ctypes.data, Px.ctypes.data, c.ctypes.data, *([None] * 11), mem)
        assert rc == PQ_ERR_INVALID and L.pq_last_error_string().decode() != ""
    assert L.pq_debug_alloc_count() == a0, "a refusal comes before the device is touched"


def test_the_read_outs_refuse_null_and_leave_out_alone(L):
    ingest = np.array([-5, -6], dtype=np.int64)
    ms = np.array([-1.5, -2.5, -3.5])
    assert L.pq_batch_last_ingest(None, ingest.ctypes.data) == PQ_ERR_INVALID and "pq_batch_last_ingest" in L.pq_last_error_string().decode()
    assert L.pq_batch_setup_ms(None, ms.ctypes.data) == PQ_ERR_INVALID and "pq_batch_setup_ms" in L.pq_last_error_string().decode()
    assert ingest.tolist() == [-5, -6] and ms.tolist() == [-1.5, -2.5, -3.5]
    # a NULL out beside a handle: any non-NULL address stands for the handle, the call must refuse before it looks at it
    fake = C.c_void_p(1)
    assert L.pq_batch_last_ingest(fake, None) == PQ_ERR_INVALID
    assert L.pq_batch_setup_ms(fake, None) == PQ_ERR_INVALID


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name}")


def test_the_wrapper_refuses_bad_tensors_before_any_library_call(monkeypatch):
    """There is no CUDA tensor on a machine without a GPU: device_call is made to answer as it does when one is among the arguments, and every tensor below is one
    that must not reach the library beside it -- float32, a wrong shape, and float64 of the right shape in CPU memory."""
    import torch
    import piqp_amd
    from piqp_amd import batch as batch_mod
    monkeypatch.setattr(batch_mod, "device_call", lambda args: True)
    s = piqp_amd.BatchSparseSolver.__new__(piqp_amd.BatchSparseSolver)
    s._owned = False
    s.L, s.h, s.device, s.bounds = NoLibrary(), C.c_void_p(1), 0, "shared"
    s.batch = s.n = s.p = s.m = 0
    B, n = 3, 4
    P = sp.identity(n, format="csc")
    c = np.ones((B, n))
    with pytest.raises(TypeError, match="float64"):
        s.setup(P, torch.ones(B, n, dtype=torch.float32), c)
    with pytest.raises(ValueError, match="shape"):
        s.setup(P, torch.ones(B, n + 1, dtype=torch.float64), c)
    with pytest.raises(ValueError, match="shape"):
        s.setup(P, torch.ones(B - 1, n, dtype=torch.float64), c)
    with pytest.raises(TypeError, match="CPU torch tensor"):
        s.setup(P, torch.ones(B, n, dtype=torch.float64), c)
    assert (s.batch, s.n) == (0, 0)


def test_a_host_call_is_still_a_host_call():
    """numpy arguments alone go to pq_batch_setup_sparse, as before: device_call decides"""
    from piqp_amd.kkt import device_call
    assert not device_call((np.ones((2, 2)), None, np.ones(3)))
