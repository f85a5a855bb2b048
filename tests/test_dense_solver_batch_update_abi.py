"""CPU-only checks of pq_solver_batch_update_dense (include/piqp_amd.h) and piqp_amd.BatchDenseSolver.update: the refusals that need no set-up handle come back as
PQ_ERR_INVALID with a text before the device is touched (a NULL handle, a bad mem or order, a call before a setup), and the Python wrapper refuses wrong shapes and
matrices the setup had none of with ValueError before any library call.  (A or b with p = 0 and G, h_l or h_u with m = 0 at the C level need a set-up handle:
tests/test_dense_solver_batch_update_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

PQ_ERR_INVALID = -1
MEM_HOST, MEM_DEVICE = 0, 1
COL_MAJOR, ROW_MAJOR = 0, 1
NAMES = ("P", "c", "A", "b", "G", "h_l", "h_u", "x_l", "x_u")

BUF = np.zeros(4 * 8 * 8)


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


def update(L, h, mem=MEM_HOST, order=ROW_MAJOR, given=NAMES):
    return L.pq_solver_batch_update_dense(h, *[BUF.ctypes.data if k in given else None for k in NAMES], mem, order)


def test_a_null_handle_is_invalid(L):
    assert update(L, None) == PQ_ERR_INVALID
    assert update(L, None, given=()) == PQ_ERR_INVALID
    out = np.zeros(2)
    assert L.pq_solver_batch_last_update_ms(None, out.ctypes.data) == PQ_ERR_INVALID


@pytest.mark.parametrize("given", [NAMES, ("c",), ()], ids=["all", "c", "none"])
def test_an_update_before_a_setup_is_invalid(L, given):
    h = C.c_void_p()
    assert L.pq_solver_batch_create(C.byref(h), 0) == 0
    assert update(L, h, given=given) == PQ_ERR_INVALID
    assert "before setup" in L.pq_last_error_string().decode()
    out = np.ones(2)
    assert L.pq_solver_batch_last_update_ms(h, out.ctypes.data) == 0 and not out.any()
    assert L.pq_solver_batch_last_update_ms(h, None) == PQ_ERR_INVALID
    L.pq_solver_batch_destroy(h)


@pytest.mark.parametrize("bad", [dict(mem=2), dict(mem=-1), dict(order=2), dict(order=-1)], ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_a_bad_mem_or_order_is_invalid_and_named(L, bad):
    h = C.c_void_p()
    assert L.pq_solver_batch_create(C.byref(h), 0) == 0
    assert update(L, h, **bad) == PQ_ERR_INVALID
    assert ("mem" if "mem" in bad else "order") in L.pq_last_error_string().decode()
    L.pq_solver_batch_destroy(h)


def test_the_python_wrapper_refuses_before_any_library_call():
    import piqp_amd
    s = piqp_amd.BatchDenseSolver()
    with pytest.raises(RuntimeError, match="before setup"):
        s.update(c=np.zeros((3, 4)))
    b, n, p, m = 3, 4, 2, 5
    dims = (b, n, p, m)
    good = dict(P=np.zeros((b, n, n)), c=np.zeros((b, n)), A=np.zeros((b, p, n)), b=np.zeros((b, p)), G=np.zeros((b, m, n)), h_l=np.zeros((b, m)), h_u=np.zeros((b, m)),
                x_l=np.zeros((b, n)), x_u=np.zeros((b, n)))
    args = lambda **kw: tuple(kw.get(k) for k in NAMES)
    got, mem, order, arrs = s._prepare(args(**good), dims)
    assert got == dims and mem == MEM_HOST and order == ROW_MAJOR and all(a.flags.c_contiguous for a in arrs)
    _, _, _, arrs = s._prepare(args(), dims)  # nothing given is legal
    assert all(a is None for a in arrs)
    _, _, _, arrs = s._prepare(args(b=good["b"], h_u=good["h_u"]), dims)  # vectors without their matrices, P and c absent
    assert [a is not None for a in arrs] == [k in ("b", "h_u") for k in NAMES]
    for bad in (dict(P=np.zeros((n, n))), dict(P=np.zeros((b, n, n + 1))), dict(P=np.zeros((b + 1, n, n))), dict(c=np.zeros((b, n + 1))), dict(c=np.zeros(n)),
                dict(A=np.zeros((b, p + 1, n))), dict(A=np.zeros((b, p, n + 1))), dict(A=np.zeros((p, n))), dict(b=np.zeros((b, p + 1))), dict(G=np.zeros((b, m))),
                dict(G=np.zeros((b, m + 1, n))), dict(h_l=np.zeros((b, m + 1))), dict(h_u=np.zeros(m)), dict(x_l=np.zeros((b, n, 1))), dict(x_u=np.zeros((b + 1, n)))):
        with pytest.raises(ValueError):
            s._prepare(args(**bad), dims)
    # update() itself, on a handle that only believes it is set up: the ValueError comes before the library could say "before setup"
    s.batch, s.n, s.p, s.m = b, n, 0, 0
    for bad in (dict(A=np.zeros((b, 0, n))), dict(b=np.zeros((b, 0))), dict(G=np.zeros((b, 0, n))), dict(h_l=np.zeros((b, 0))), dict(h_u=np.zeros((b, 0))),
                dict(c=np.zeros((b, n + 1)))):
        with pytest.raises(ValueError):
            s.update(**bad)
