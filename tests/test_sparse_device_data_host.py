"""Sparse problem data whose values live in GPU memory, the part that needs no GPU: the gather maps a device-mode setup builds from the sparsity patterns alone
(pq_debug_sparse_ingest_maps, host-only) against scipy, and what SparseSolver refuses before the library is called."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import piqp_amd
from piqp_amd import kkt


def _csc(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return M


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _maps(P, A, G):
    """(mapP, mapA, mapG, nnz_out) of the hook for sorted-CSC patterns P (n x n), A (p x n) / None, G (m x n) / None"""
    L = piqp_amd._lib.load()
    n = P.shape[0]
    keep, args, outs = [], [], []
    for M in (P, A, G):
        if M is None:
            args += [None, None]
            outs.append(None)
            continue
        ip, ii = _i32(M.indptr), _i32(M.indices)
        keep += [ip, ii]
        args += [ip.ctypes.data, ii.ctypes.data]
        outs.append(np.full(max(M.nnz, 1), -7, dtype=np.int32))
    nnz = (C.c_int * 3)()
    rc = L.pq_debug_sparse_ingest_maps(n, 0 if A is None else A.shape[0], 0 if G is None else G.shape[0], *args, *[None if o is None else o.ctypes.data for o in outs], C.byref(nnz))
    assert rc == 0, L.pq_last_error_string()
    return [None if o is None else o[: M.nnz] for o, M in zip(outs, (P, A, G))] + [tuple(nnz)]


def _labelled(M):
    """M with its k-th stored value replaced by k + 1: wherever scipy moves the entry, the label says where it came from"""
    L = M.copy()
    L.data = np.arange(1, M.nnz + 1, dtype=np.float64)
    return L


def _check_P(P):
    P = _csc(P)
    mapP, _, _, nnz = _maps(P, None, None)
    U = _csc(sp.triu(_labelled(P), format="csc"))
    assert nnz == (U.nnz, 0, 0)
    rows = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))  # column of every stored entry
    upper = P.indices <= rows
    assert np.array_equal(mapP >= 0, upper)  # exactly the entries on or above the diagonal are read
    src = (U.data - 1).astype(np.int64)  # stored entry t of triu(P) is the caller's entry src[t]
    assert np.array_equal(mapP[src], np.arange(U.nnz))
    assert sorted(mapP[upper]) == list(range(U.nnz))


def _check_T(A, which):
    A = _csc(A)
    P = _csc(sp.identity(A.shape[1]))
    out = _maps(P, A if which == "A" else None, A if which == "G" else None)
    m = out[1] if which == "A" else out[2]
    T = _csc(_labelled(A).T)
    assert out[3] == (P.nnz, A.nnz if which == "A" else 0, A.nnz if which == "G" else 0)
    src = (T.data - 1).astype(np.int64)
    assert np.array_equal(m[src], np.arange(T.nnz))
    assert sorted(m) == list(range(A.nnz))


def _random(rows, cols, density, seed):
    return sp.random(rows, cols, density=density, random_state=np.random.default_rng(seed), format="csc")


@pytest.mark.parametrize("n, density, seed", [(1, 1.0, 0), (7, 0.4, 1), (40, 0.15, 2), (65, 0.05, 3)])
def test_map_of_a_full_P_sends_every_upper_entry_where_triu_puts_it(n, density, seed):
    R = _random(n, n, density, seed)
    _check_P(R + R.T + sp.identity(n))


@pytest.mark.parametrize("n, density, seed", [(1, 1.0, 0), (9, 0.5, 4), (40, 0.1, 5)])
def test_map_of_an_upper_P_is_the_identity(n, density, seed):
    U = _csc(sp.triu(_random(n, n, density, seed) + sp.identity(n), format="csc"))
    _check_P(U)
    assert np.array_equal(_maps(U, None, None)[0], np.arange(U.nnz))


def test_map_of_P_with_empty_columns_and_without_a_diagonal():
    P = sp.lil_matrix((6, 6))
    P[0, 2] = 1.0; P[2, 0] = 1.0; P[1, 5] = 2.0; P[5, 1] = 2.0; P[5, 5] = 3.0  # columns 3 and 4 empty, most diagonals absent
    _check_P(P)
    _check_P(sp.csc_matrix((4, 4)))  # no entry at all


@pytest.mark.parametrize("which", ["A", "G"])
@pytest.mark.parametrize("rows, cols, density, seed", [(1, 1, 1.0, 0), (3, 9, 0.5, 6), (20, 7, 0.3, 7), (33, 70, 0.05, 8)])
def test_map_of_a_rectangular_matrix_is_the_transposition(which, rows, cols, density, seed):
    _check_T(_random(rows, cols, density, seed), which)


@pytest.mark.parametrize("which", ["A", "G"])
def test_map_of_an_empty_matrix_and_of_empty_columns(which):
    _check_T(sp.csc_matrix((4, 6)), which)
    A = sp.lil_matrix((3, 8))
    A[2, 0] = 1.0; A[0, 0] = 2.0; A[1, 7] = 3.0; A[2, 7] = 4.0  # columns 1 .. 6 empty, row order reversed by the transposition
    _check_T(A, which)


def test_all_three_maps_in_one_call():
    R = _random(12, 12, 0.3, 9)
    P, A, G = _csc(R + R.T + sp.identity(12)), _csc(_random(5, 12, 0.4, 10)), _csc(_random(8, 12, 0.3, 11))
    mapP, mapA, mapG, nnz = _maps(P, A, G)
    assert nnz == (sp.triu(P).nnz, A.nnz, G.nnz)
    assert np.array_equal(mapA, _maps(_csc(sp.identity(12)), A, None)[1]) and np.array_equal(mapG, _maps(_csc(sp.identity(12)), None, G)[2])
    assert np.array_equal(mapP, _maps(P, None, None)[0])


def test_bad_arguments_of_the_hook():
    L = piqp_amd._lib.load()
    assert L.pq_debug_sparse_ingest_maps(0, 0, 0, *[None] * 9, None) == -1
    assert L.pq_debug_sparse_ingest_maps(3, 0, 0, *[None] * 9, None) == -1  # no pattern of P


# ---------------------------------------------------------------------------------------------- the binding refuses before any library call
class _NoLibrary:
    """stands where the loaded library would: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def _solver():
    s = object.__new__(piqp_amd.SparseSolver)  # no handle: no GPU needed
    s.L = _NoLibrary()
    s.h = None
    s.device = 0
    s._trace = None
    s._owned = False
    return s


def _qp():
    P = _csc(sp.identity(4) * 2.0)
    A = _csc(sp.csc_matrix(np.array([[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0]])))
    return P, np.zeros(4), A, np.zeros(2)


@pytest.fixture
def device_path(monkeypatch):
    """No GPU here, so no CUDA tensor can select the device path: force it.  The checks then meet CPU tensors, and refuse them in the order dtype, shape, device."""
    monkeypatch.setattr(kkt, "device_call", lambda args: True)


def test_float32_values_are_refused(device_path):
    P, c, A, b = _qp()
    with pytest.raises(TypeError, match="float64"):
        _solver().setup((P, torch.ones(P.nnz, dtype=torch.float32)), c, A, b)
    with pytest.raises(TypeError, match="float64"):
        _solver().setup(P, torch.zeros(4, dtype=torch.float32), A, b)


def test_pair_with_the_wrong_number_of_values_is_refused(device_path):
    P, c, A, b = _qp()
    with pytest.raises(ValueError, match=r"A: shape \(5,\), expected \(4,\)"):
        _solver().setup(P, c, (A, torch.ones(A.nnz + 1, dtype=torch.float64)), b)
    with pytest.raises(ValueError, match="shape"):
        _solver().setup((P, np.ones(P.nnz + 1)), c, A, b)  # numpy values beside device data: checked before they are moved
    with pytest.raises(ValueError, match="shape"):
        _solver().setup((P, torch.ones(2, P.nnz, dtype=torch.float64)), c, A, b)  # 2-D where the CSC values are meant


def test_pair_with_the_wrong_number_of_values_is_refused_on_the_host_path_too():
    P, c, A, b = _qp()
    with pytest.raises(ValueError, match="shape"):
        _solver().setup((P, np.ones(P.nnz + 1)), c, A, b)
    with pytest.raises(ValueError, match="shape"):
        _solver().update(A=(A, np.ones(A.nnz - 1)))


def test_vector_of_the_wrong_shape_is_refused(device_path):
    P, c, A, b = _qp()
    with pytest.raises(ValueError, match=r"c: shape \(5,\), expected \(4,\)"):
        _solver().setup(P, np.zeros(5), A, b)
    with pytest.raises(ValueError, match="shape"):
        _solver().setup(P, c, A, torch.zeros(2, 1, dtype=torch.float64))


def test_cpu_tensor_is_refused(device_path):
    P, c, A, b = _qp()
    with pytest.raises(TypeError, match="CPU torch tensor"):
        _solver().setup((P, torch.ones(P.nnz, dtype=torch.float64)), c, A, b)
    s = _solver()
    s._dims = lambda: (4, 2, 0)
    s._nnz = dict(P=P.nnz, A=A.nnz, G=0)
    with pytest.raises(TypeError, match="CPU torch tensor"):
        s.update(A=torch.ones(A.nnz, dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):
        s.update(P=torch.ones(P.nnz + 2, dtype=torch.float64))


def test_cpu_tensor_alone_is_refused_on_the_host_path_too():
    """no CUDA argument, so the call would take the host path: a bare tensor of values, or the values of a pair, must not reach scipy as if they were a matrix"""
    P, c, A, b = _qp()
    with pytest.raises(TypeError, match="CPU torch tensor"):
        _solver().update(A=torch.ones(A.nnz, dtype=torch.float64))
    with pytest.raises(TypeError, match="CPU torch tensor"):
        _solver().setup((P, torch.ones(P.nnz, dtype=torch.float64)), c, A, b)
    with pytest.raises(TypeError, match="scipy sparse pattern"):
        _solver().setup(torch.eye(4, dtype=torch.float64), c, A, b)


def test_a_pair_must_be_a_pair():
    P, c, A, b = _qp()
    with pytest.raises(TypeError, match="pair"):
        _solver().setup((P, np.ones(P.nnz), 3), c, A, b)


def test_device_update_needs_the_lengths_of_the_setup(device_path):
    s = _solver()
    s._dims = lambda: (4, 2, 0)
    assert s._nnz is None
    with pytest.raises(RuntimeError, match="never saw the setup"):
        s.update(P=torch.ones(4, dtype=torch.float64))
