"""CPU-only checks of pq_solver_batch_* (include/piqp_amd.h) and piqp_amd.BatchDenseSolver: every argument is validated before the device is touched, so on a
machine without a GPU a bad argument is reported as such (PQ_ERR_INVALID / PQ_ERR_UNSUPPORTED with a text), never as a HIP error; null handles are invalid in every
entry point; the Python wrapper refuses wrong shapes before any library call.  (Settings that verify_settings refuses need a set-up handle: that refusal is in
tests/test_dense_solver_batch_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

PQ_ERR_INVALID, PQ_ERR_HIP, PQ_ERR_UNSUPPORTED = -1, -2, -3
PQ_UNSOLVED = -9
DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT = 0, 16
MEM_HOST, MEM_DEVICE = 0, 1
COL_MAJOR, ROW_MAJOR = 0, 1

BUF = np.zeros(4 * 8 * 8)  # enough for every array of the default arguments


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


def setup(L, batch=4, n=8, p=3, m=5, kind=DENSE_CHOLESKY, mem=MEM_HOST, order=COL_MAJOR, null=(), **skw):
    """the code of pq_solver_batch_setup_dense on a fresh handle; null: names of the nine arrays passed as NULL"""
    h = C.c_void_p()
    assert L.pq_solver_batch_create(C.byref(h), 0) == 0
    s = L.pq_solver_batch_settings(h).contents
    s.kkt_solver = kind
    for k, v in skw.items():
        setattr(s, k, v)
    ptrs = [None if k in null else BUF.ctypes.data for k in ("P", "c", "A", "b", "G", "h_l", "h_u", "x_l", "x_u")]
    rc = L.pq_solver_batch_setup_dense(h, batch, n, p, m, *ptrs, mem, order)
    L.pq_solver_batch_destroy(h)
    return rc


@pytest.mark.parametrize("kind", [DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT])
def test_n_above_the_limit_is_unsupported_and_the_message_names_n_and_the_limit(L, kind):
    assert setup(L, n=129, kind=kind) == PQ_ERR_UNSUPPORTED
    msg = L.pq_last_error_string().decode()
    assert "129" in msg and "128" in msg


@pytest.mark.parametrize("bad", [dict(batch=0), dict(batch=-3), dict(n=0), dict(n=-1), dict(p=-1), dict(m=-1), dict(kind=1), dict(kind=5), dict(kind=19), dict(kind=-1),
                                 dict(null=("P",)), dict(null=("c",)), dict(null=("A",)), dict(null=("G",)), dict(iterative_refinement_max_iter=-1),
                                 dict(iterative_refinement_max_iter=65), dict(mem=2), dict(mem=-1), dict(order=2), dict(order=-1)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_a_bad_argument_of_setup_is_invalid_before_the_device_is_touched(L, bad):
    assert setup(L, **bad) == PQ_ERR_INVALID
    assert L.pq_last_error_string().decode() != ""


def test_null_optionals_are_not_refused_as_arguments(L):
    """NULL b, bounds and absent matrices with a zero count pass the argument checks: without a device the call then ends as a HIP error, with one it sets up"""
    assert setup(L, null=("b", "h_l", "h_u", "x_l", "x_u")) in (PQ_ERR_HIP, 1)
    assert setup(L, p=0, m=0, null=("A", "b", "G", "h_l", "h_u")) in (PQ_ERR_HIP, 1)


def test_solve_and_queries_before_setup(L):
    h = C.c_void_p()
    assert L.pq_solver_batch_create(C.byref(h), 0) == 0
    assert L.pq_solver_batch_solve(h) == PQ_ERR_INVALID
    assert "before setup" in L.pq_last_error_string().decode()
    assert L.pq_solver_batch_info(h, 0).contents.status == PQ_UNSOLVED  # as the single solver: "Solver not setup yet"
    out = np.zeros(8)
    rows = C.c_int(0)
    assert L.pq_solver_batch_get_result_mem(h, 0, out.ctypes.data, MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_solver_batch_get_trace(h, 0, out.ctypes.data, C.byref(rows)) == PQ_ERR_INVALID
    assert L.pq_solver_batch_dims(h, None, None, None, None) == PQ_ERR_INVALID
    assert L.pq_solver_batch_scaled_data(h, 0, 0, out.ctypes.data) == PQ_ERR_INVALID
    assert not L.pq_solver_batch_kktsys(h)
    assert L.pq_solver_batch_set_trace(h, -1) == PQ_ERR_INVALID
    assert L.pq_solver_batch_set_trace(h, 16) == 0
    o6 = np.ones(6)
    assert L.pq_solver_batch_last_ms(h, o6.ctypes.data) == 0 and not o6.any()
    L.pq_solver_batch_destroy(h)


def test_null_handles_and_null_outputs(L):
    out = np.zeros(8)
    rows = C.c_int(0)
    assert L.pq_solver_batch_create(None, 0) == PQ_ERR_INVALID
    assert L.pq_solver_batch_create(C.byref(C.c_void_p()), -1) == PQ_ERR_INVALID
    L.pq_solver_batch_destroy(None)
    assert not L.pq_solver_batch_settings(None)
    assert L.pq_solver_batch_setup_dense(None, 1, 1, 0, 0, BUF.ctypes.data, BUF.ctypes.data, None, None, None, None, None, None, None, MEM_HOST, COL_MAJOR) == PQ_ERR_INVALID
    assert L.pq_solver_batch_solve(None) == PQ_ERR_INVALID
    assert not L.pq_solver_batch_info(None, 0)
    assert L.pq_solver_batch_get_result_mem(None, 0, out.ctypes.data, MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_solver_batch_set_trace(None, 4) == PQ_ERR_INVALID
    assert L.pq_solver_batch_get_trace(None, 0, out.ctypes.data, C.byref(rows)) == PQ_ERR_INVALID
    assert L.pq_solver_batch_dims(None, None, None, None, None) == PQ_ERR_INVALID
    assert L.pq_solver_batch_last_ms(None, out.ctypes.data) == PQ_ERR_INVALID
    assert L.pq_solver_batch_scaled_data(None, 0, 0, out.ctypes.data) == PQ_ERR_INVALID
    assert not L.pq_solver_batch_kktsys(None)
    h = C.c_void_p()
    assert L.pq_solver_batch_create(C.byref(h), 0) == 0
    assert L.pq_solver_batch_get_result_mem(h, 0, None, MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_solver_batch_get_result_mem(h, 10, out.ctypes.data, MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_solver_batch_get_result_mem(h, 0, out.ctypes.data, 2) == PQ_ERR_INVALID
    assert L.pq_solver_batch_last_ms(h, None) == PQ_ERR_INVALID
    L.pq_solver_batch_destroy(h)


def test_the_python_wrapper_checks_shapes_before_any_library_call():
    import piqp_amd
    with pytest.raises(ValueError):
        piqp_amd.BatchDenseSolver(kkt_solver=1)
    s = piqp_amd.BatchDenseSolver(kkt_solver=DENSE_LDLT_NO_PIVOT)
    assert s.settings.kkt_solver == DENSE_LDLT_NO_PIVOT
    b, n, p, m = 3, 4, 2, 5
    good = dict(P=np.zeros((b, n, n)), c=np.zeros((b, n)), A=np.zeros((b, p, n)), b=np.zeros((b, p)), G=np.zeros((b, m, n)), h_l=np.zeros((b, m)), h_u=np.zeros((b, m)),
                x_l=np.zeros((b, n)), x_u=np.zeros((b, n)))
    args = lambda **kw: tuple(dict(good, **kw)[k] for k in ("P", "c", "A", "b", "G", "h_l", "h_u", "x_l", "x_u"))
    dims, mem, order, arrs = s._prepare(args())
    assert dims == (b, n, p, m) and mem == MEM_HOST and order == ROW_MAJOR and all(a.flags.c_contiguous for a in arrs)
    dims, _, _, arrs = s._prepare(args(A=None, b=None, G=None, h_l=None, h_u=None, x_l=None))
    assert dims == (b, n, 0, 0) and arrs[2] is None and arrs[7] is None
    for bad in (dict(P=np.zeros((n, n))), dict(P=np.zeros((b, n, n + 1))), dict(P=np.zeros((b, 129, 129))), dict(P=None), dict(c=None), dict(c=np.zeros((b, n + 1))),
                dict(A=np.zeros((b, p, n + 1))), dict(A=np.zeros((b + 1, p, n))), dict(A=np.zeros((p, n))), dict(G=np.zeros((b, m))), dict(b=np.zeros((b, p + 1))),
                dict(h_l=np.zeros((b, m + 1))), dict(h_u=np.zeros(m)), dict(x_l=np.zeros((b, n, 1))), dict(x_u=np.zeros((b + 1, n))), dict(A=None), dict(G=None)):
        with pytest.raises(ValueError):
            s._prepare(args(**bad))
