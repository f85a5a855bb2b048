"""CPU-only checks of pq_kktsys_batch_* (include/piqp_amd.h): every argument of pq_kktsys_batch_create_dense is validated before the device is touched, so on a
machine without a GPU a bad argument is reported as such (PQ_ERR_INVALID / PQ_ERR_UNSUPPORTED with a text), never as a HIP error; null handles are invalid in
every entry point."""
import ctypes as C

import numpy as np
import pytest

PQ_ERR_INVALID, PQ_ERR_HIP, PQ_ERR_UNSUPPORTED = -1, -2, -3
DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT = 0, 16
MEM_HOST, MEM_DEVICE = 0, 1


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


BUF = np.zeros(4 * 8 * 8)  # enough for P (4 x 8 x 8), AT (4 x 8 x 3), GT (4 x 8 x 5) and x_b_scaling (4 x 8) of the default arguments
GOOD = dict(h_l=[0, 1, 3], h_u=[1, 2, 4], x_l=[0, 7], x_u=[])  # m = 5: every row is in one of the two lists; n = 8


def settings(L, **kw):
    import piqp_amd
    s = piqp_amd._lib.Settings()
    L.pq_settings_default(C.byref(s))
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def create(L, batch=4, n=8, p=3, m=5, kind=DENSE_CHOLESKY, P=True, AT=True, GT=True, xbs=True, mem=MEM_HOST, lists=None, counts=None, null_list=None, have_settings=True,
           out=True, **skw):
    """returns the code of pq_kktsys_batch_create_dense; lists: overrides of GOOD; counts: overrides of the four counts; null_list: names passed as NULL"""
    h = C.c_void_p()
    ptr = lambda have: BUF.ctypes.data if have else None
    ls = dict(GOOD, **(lists or {}))
    arrs = {k: np.asarray(v, dtype=np.int32) for k, v in ls.items()}
    cnt = {k: len(v) for k, v in arrs.items()}
    cnt.update(counts or {})
    lp = {k: (None if k in (null_list or ()) else a.ctypes.data) for k, a in arrs.items()}
    s = settings(L, kkt_solver=kind, **skw)
    rc = L.pq_kktsys_batch_create_dense(C.byref(h) if out else None, 0, batch, n, p, m, ptr(P), ptr(AT), ptr(GT), cnt["h_l"], cnt["h_u"], cnt["x_l"], cnt["x_u"],
                                        lp["h_l"], lp["h_u"], lp["x_l"], lp["x_u"], ptr(xbs), C.byref(s) if have_settings else None, mem)
    if rc == 0:
        L.pq_kktsys_batch_destroy(h)
    return rc


@pytest.mark.parametrize("kind", [DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT])
def test_n_above_the_limit_is_unsupported_and_the_message_names_n_and_the_limit(L, kind):
    assert create(L, n=129, kind=kind) == PQ_ERR_UNSUPPORTED
    msg = L.pq_last_error_string().decode()
    assert "129" in msg and "128" in msg
    assert create(L, n=100000, kind=kind, p=0, m=0, lists=dict(h_l=[], h_u=[])) == PQ_ERR_UNSUPPORTED


# what pq_kkt_batch_create_dense refuses
@pytest.mark.parametrize("bad", [dict(batch=0), dict(batch=-3), dict(n=0), dict(n=-1), dict(p=-1), dict(m=-1), dict(kind=1), dict(kind=19), dict(kind=-1),
                                 dict(mem=2), dict(mem=-1), dict(P=False), dict(AT=False), dict(GT=False), dict(out=False)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_what_the_backend_refuses_is_invalid(L, bad):
    assert create(L, **bad) == PQ_ERR_INVALID
    assert L.pq_last_error_string().decode() != ""


# what the KKTSystem layer refuses on top of that
@pytest.mark.parametrize("bad", [
    dict(have_settings=False),
    dict(iterative_refinement_max_iter=-1), dict(iterative_refinement_max_iter=65),
    dict(counts=dict(h_l=-1)), dict(counts=dict(h_u=-2)), dict(counts=dict(x_l=-1)), dict(counts=dict(x_u=-1)),                     # a negative count
    dict(counts=dict(h_l=6)), dict(counts=dict(h_u=6)), dict(counts=dict(x_l=9)), dict(counts=dict(x_u=9)),                         # above its vector's length
    dict(null_list=("h_l",)), dict(null_list=("h_u",)), dict(null_list=("x_l",)), dict(null_list=("x_u",), counts=dict(x_u=1)),    # a NULL list with a positive count
    dict(lists=dict(h_l=[0, 3, 1])), dict(lists=dict(h_u=[1, 1, 2, 4])), dict(lists=dict(x_l=[7, 0])), dict(lists=dict(x_u=[2, 2])),  # not strictly ascending
    dict(lists=dict(h_l=[0, 1, 5])), dict(lists=dict(h_u=[-1, 1, 2, 4])), dict(lists=dict(x_l=[0, 8])), dict(lists=dict(x_u=[-3])),   # an index out of range
    dict(lists=dict(h_l=[0, 1], h_u=[1, 2, 4])), dict(lists=dict(h_l=[], h_u=[])),                                                # a row of G in neither list
], ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_bad_lists_counts_and_settings_are_invalid(L, bad):
    assert create(L, **bad) == PQ_ERR_INVALID
    assert L.pq_last_error_string().decode() != ""


def test_good_arguments_get_past_the_checks(L):
    """with the default arguments of this file the only thing that can fail is the device itself"""
    rc = create(L)
    assert rc in (0, PQ_ERR_HIP), (rc, L.pq_last_error_string().decode())
    assert create(L, iterative_refinement_max_iter=0) in (0, PQ_ERR_HIP)
    assert create(L, iterative_refinement_max_iter=64, xbs=False, p=0, AT=False) in (0, PQ_ERR_HIP)


def test_null_handles_are_invalid(L):
    import piqp_amd
    p = BUF.ctypes.data
    h = C.c_void_p()
    three = (C.c_double * 3)()
    dims = [C.c_int() for _ in range(4)]
    v = piqp_amd._lib.Vars(*([p] * 10))
    s = settings(L)
    assert L.pq_kktsys_batch_clone(None, C.byref(h)) == PQ_ERR_INVALID
    assert L.pq_kktsys_batch_dims(None, *[C.byref(d) for d in dims]) == PQ_ERR_INVALID
    assert L.pq_kktsys_batch_backend(None) is None
    assert L.pq_last_error_string().decode() != ""
    assert L.pq_kktsys_batch_update_data_dense(None, p, p, p, p, 7, MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_kktsys_batch_set_settings(None, C.byref(s)) == PQ_ERR_INVALID
    assert L.pq_kktsys_batch_update_scalings_and_factor(None, p, p, p, C.byref(v), MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_kktsys_batch_solve(None, C.byref(v), C.byref(v), MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_kktsys_batch_mul(None, C.byref(v), C.byref(v), MEM_HOST) == PQ_ERR_INVALID
    assert L.pq_kktsys_batch_info(None, p, p, p, p, p) == PQ_ERR_INVALID
    assert L.pq_kktsys_batch_state(None, 0, p) == PQ_ERR_INVALID
    assert L.pq_kktsys_batch_last_ms(None, three) == PQ_ERR_INVALID
    L.pq_kktsys_batch_destroy(None)


def test_the_wrapper_refuses_bad_arguments_before_any_library_call():
    import piqp_amd
    P, G = np.zeros((4, 8, 8)), np.zeros((4, 5, 8))
    with pytest.raises(TypeError):
        piqp_amd.BatchKKTSystem(P.astype(np.float32))
    with pytest.raises(ValueError):
        piqp_amd.BatchKKTSystem(np.zeros((4, 8, 7)))
    with pytest.raises(ValueError):
        piqp_amd.BatchKKTSystem(P, G=np.zeros((3, 5, 8)))
    with pytest.raises(ValueError):
        piqp_amd.BatchKKTSystem(P, kkt_solver=piqp_amd.DENSE_CHOLESKY_EXACT)
    with pytest.raises(ValueError):
        piqp_amd.BatchKKTSystem(P, G=G, h_l_idx=[0, 1], h_u_idx=[1, 2, 3])  # row 4 has no bound
    with pytest.raises(ValueError):
        piqp_amd.BatchKKTSystem(P, G=G, x_l_idx=[3, 2])
    with pytest.raises(ValueError):
        piqp_amd.BatchKKTSystem(P, G=G, x_u_idx=[8])
    with pytest.raises(TypeError):
        piqp_amd.BatchKKTSystem(P, G=G, x_u_idx=[0.5])
    with pytest.raises(ValueError):
        piqp_amd.BatchKKTSystem(P, G=G, x_b_scaling=np.ones((4, 7)))
    with pytest.raises(ValueError):
        piqp_amd.BatchKKTSystem(P, G=G, settings=piqp_amd.default_settings(iterative_refinement_max_iter=65))
