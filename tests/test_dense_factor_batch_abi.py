"""CPU-only checks of pq_dense_factor_batch_create (include/piqp_amd.h): every argument is validated before the device is touched, so on a machine without a GPU a
bad argument is reported as such (PQ_ERR_INVALID / PQ_ERR_UNSUPPORTED), never as a HIP error."""
import ctypes as C

import pytest

PQ_ERR_INVALID, PQ_ERR_HIP, PQ_ERR_UNSUPPORTED = -1, -2, -3
DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT = 0, 16
LOWER, UPPER = 1, 2


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


def create(L, batch=4, n=8, kind=DENSE_CHOLESKY, uplo=LOWER, max_nrhs=1):
    h = C.c_void_p()
    rc = L.pq_dense_factor_batch_create(C.byref(h), 0, batch, n, kind, uplo, max_nrhs)
    if rc == 0:
        L.pq_dense_factor_batch_destroy(h)
    return rc


def test_the_limit_is_in_the_header_and_in_the_package():
    import os
    import piqp_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "PQ_DENSE_FACTOR_BATCH_MAX_N = 128" in open(os.path.join(root, "include", "piqp_amd.h")).read()
    assert piqp_amd.BatchLLT._kind == DENSE_CHOLESKY and piqp_amd.BatchLDLTNoPivot._kind == DENSE_LDLT_NO_PIVOT


@pytest.mark.parametrize("kind", [DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT])
def test_n_above_the_limit_is_unsupported_and_the_message_names_the_limit(L, kind):
    assert create(L, n=129, kind=kind) == PQ_ERR_UNSUPPORTED
    msg = L.pq_last_error_string().decode()
    assert "129" in msg and "128" in msg
    assert create(L, n=100000, kind=kind, uplo=UPPER) == PQ_ERR_UNSUPPORTED


@pytest.mark.parametrize("bad", [dict(batch=0), dict(batch=-3), dict(n=0), dict(n=-1), dict(max_nrhs=0), dict(kind=1), dict(kind=19), dict(uplo=0), dict(uplo=3)])
def test_bad_arguments_are_invalid(L, bad):
    assert create(L, **bad) == PQ_ERR_INVALID
    assert L.pq_last_error_string().decode() != ""


def test_null_out_is_invalid(L):
    assert L.pq_dense_factor_batch_create(None, 0, 4, 8, DENSE_CHOLESKY, LOWER, 1) == PQ_ERR_INVALID


def test_null_handles_are_invalid(L):
    assert L.pq_dense_factor_batch_compute(None, None, 8, 64, 0) == PQ_ERR_INVALID
    assert L.pq_dense_factor_batch_info(None, None, None) == PQ_ERR_INVALID
    assert L.pq_dense_factor_batch_solve_in_place(None, None, 8, 1, 8, 0) == PQ_ERR_INVALID
    assert L.pq_dense_factor_batch_matrix(None, 0, None, 8) == PQ_ERR_INVALID
    assert L.pq_dense_factor_batch_last_ms(None, None) == PQ_ERR_INVALID
    L.pq_dense_factor_batch_destroy(None)
