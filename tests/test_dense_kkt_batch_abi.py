"""CPU-only checks of pq_kkt_batch_create_dense (include/piqp_amd.h): every argument is validated before the device is touched, so on a machine without a GPU a
bad argument is reported as such (PQ_ERR_INVALID / PQ_ERR_UNSUPPORTED), never as a HIP error."""
import ctypes as C
import os

import numpy as np
import pytest

PQ_ERR_INVALID, PQ_ERR_HIP, PQ_ERR_UNSUPPORTED = -1, -2, -3
DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT = 0, 16
MEM_HOST, MEM_DEVICE = 0, 1


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


BUF = np.zeros(4 * 8 * 8)  # enough for P (4 x 8 x 8), AT (4 x 8 x 3) and GT (4 x 8 x 5) of the default arguments


def create(L, batch=4, n=8, p=3, m=5, kind=DENSE_CHOLESKY, P=True, AT=True, GT=True, mem=MEM_HOST):
    h = C.c_void_p()
    ptr = lambda have: BUF.ctypes.data if have else None
    rc = L.pq_kkt_batch_create_dense(C.byref(h), 0, batch, n, p, m, kind, ptr(P), ptr(AT), ptr(GT), mem)
    if rc == 0:
        L.pq_kkt_batch_destroy(h)
    return rc


def test_the_limit_is_in_the_header_and_in_the_package():
    import piqp_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "PQ_KKT_BATCH_DENSE_MAX_N = 128" in open(os.path.join(root, "include", "piqp_amd.h")).read()
    assert piqp_amd.KKT_BATCH_DENSE_MAX_N == 128 == piqp_amd.batch_kkt.KKT_BATCH_DENSE_MAX_N


@pytest.mark.parametrize("kind", [DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT])
def test_n_above_the_limit_is_unsupported_and_the_message_names_n_and_the_limit(L, kind):
    assert create(L, n=129, kind=kind) == PQ_ERR_UNSUPPORTED
    msg = L.pq_last_error_string().decode()
    assert "129" in msg and "128" in msg
    assert create(L, n=100000, kind=kind, p=0, m=0) == PQ_ERR_UNSUPPORTED


@pytest.mark.parametrize("bad", [dict(batch=0), dict(batch=-3), dict(n=0), dict(n=-1), dict(p=-1), dict(m=-1), dict(kind=1), dict(kind=19), dict(kind=-1),
                                 dict(mem=2), dict(mem=-1), dict(P=False), dict(AT=False), dict(GT=False), dict(P=False, p=0, m=0)])
def test_bad_arguments_are_invalid(L, bad):
    assert create(L, **bad) == PQ_ERR_INVALID
    assert L.pq_last_error_string().decode() != ""


def test_null_out_is_invalid(L):
    p = BUF.ctypes.data
    assert L.pq_kkt_batch_create_dense(None, 0, 4, 8, 3, 5, DENSE_CHOLESKY, p, p, p, MEM_HOST) == PQ_ERR_INVALID


def test_null_handles_are_invalid(L):
    p = BUF.ctypes.data
    h = C.c_void_p()
    three = (C.c_double * 3)()
    dims = [C.c_int() for _ in range(4)]
    assert L.pq_kkt_batch_clone(None, C.byref(h)) == PQ_ERR_INVALID
    assert L.pq_kkt_batch_dims(None, *[C.byref(d) for d in dims]) == PQ_ERR_INVALID
    assert L.pq_kkt_batch_update_data_dense(None, p, p, p, 7, MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_kkt_batch_update_scalings_and_factor(None, p, p, p, MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_kkt_batch_info(None, p, p) == PQ_ERR_INVALID
    assert L.pq_kkt_batch_solve(None, p, p, p, p, p, p, MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_kkt_batch_eval_P_x(None, p, p, p, MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_kkt_batch_eval_A_xn_and_AT_xt(None, p, p, p, p, p, p, MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_kkt_batch_eval_G_xn_and_GT_xt(None, p, p, p, p, p, p, MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_kkt_batch_internal_kkt_mat(None, 0, p) == PQ_ERR_INVALID
    assert L.pq_kkt_batch_internal_factor(None, 0, p) == PQ_ERR_INVALID
    assert L.pq_kkt_batch_last_ms(None, three) == PQ_ERR_INVALID
    L.pq_kkt_batch_destroy(None)


def test_the_wrapper_refuses_bad_arguments_before_any_library_call():
    import piqp_amd
    P = np.zeros((4, 8, 8))
    with pytest.raises(TypeError):
        piqp_amd.BatchDenseKKT(P.astype(np.float32))
    with pytest.raises(ValueError):
        piqp_amd.BatchDenseKKT(np.zeros((4, 8, 7)))
    with pytest.raises(ValueError):
        piqp_amd.BatchDenseKKT(P, A=np.zeros((4, 3, 9)))
    with pytest.raises(ValueError):
        piqp_amd.BatchDenseKKT(P, G=np.zeros((3, 5, 8)))
    with pytest.raises(ValueError):
        piqp_amd.BatchDenseKKT(P, kkt_solver=piqp_amd.DENSE_CHOLESKY_EXACT)
