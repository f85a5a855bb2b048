"""Host-side mirror of the reference's dense factorisation classes as stand-alone objects: piqp::dense::LDLTNoPivot<Mat, UpLo>
(/root/reference/include/piqp/dense/ldlt_no_pivot.hpp:87-262) and the Eigen::LLT<Mat, UpLo> that dense/kkt.hpp:82 uses -- same member names, same meaning of
info(); the work is done by the HIP kernels behind pq_dense_factor_* (include/piqp_amd.h).  What tests/src/dense/ldlt_test.cpp and
benchmarks/src/dense_cholesky_factorization_benchmark.cpp use."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .kkt import DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT, MEM_DEVICE, MEM_HOST, _Handle, _is_torch, _ptr, sync_current_stream

LOWER, UPPER = 1, 2       # Eigen::Lower, Eigen::Upper
SUCCESS, NUMERICAL_ISSUE = 0, 1  # Eigen::ComputationInfo


class _DenseFactor(_Handle):
    _destroy = "pq_dense_factor_destroy"
    _kind = DENSE_LDLT_NO_PIVOT

    def __init__(self, n, uplo=LOWER, device=0):
        self.L = _lib.load()
        self.n, self.uplo = int(n), int(uplo)
        h = C.c_void_p()
        check(self.L.pq_dense_factor_create(C.byref(h), device, self.n, self._kind, self.uplo), "pq_dense_factor_create")
        self.h = h

    def compute(self, A):
        """A: n x n numpy array (any layout; only the `uplo` triangle is read).  Device-resident matrices: compute_colmajor"""
        Af = np.asfortranarray(A, dtype=np.float64)
        assert Af.shape == (self.n, self.n)
        self._info = check(self.L.pq_dense_factor_compute(self.h, Af.ctypes.data, self.n, MEM_HOST), "pq_dense_factor_compute")
        return self

    def compute_colmajor(self, ptr_or_tensor, lda=None, on_device=True):
        """the column-major matrix at a raw address / in a torch tensor's storage, leading dimension lda (default n); no copy through the host"""
        p = ptr_or_tensor if isinstance(ptr_or_tensor, int) else _ptr(ptr_or_tensor)
        self._keep = ptr_or_tensor
        self._info = check(self.L.pq_dense_factor_compute(self.h, p, self.n if lda is None else int(lda), MEM_DEVICE if on_device else MEM_HOST), "pq_dense_factor_compute")
        return self

    def info(self):
        return check(self.L.pq_dense_factor_info(self.h), "pq_dense_factor_info")

    def solveInPlace(self, x):
        if _is_torch(x):
            check(self.L.pq_dense_factor_solve_in_place(self.h, x.data_ptr(), MEM_DEVICE), "pq_dense_factor_solve_in_place")
            return x
        assert x.dtype == np.float64 and x.flags.c_contiguous and x.shape == (self.n,)
        check(self.L.pq_dense_factor_solve_in_place(self.h, x.ctypes.data, MEM_HOST), "pq_dense_factor_solve_in_place")
        return x

    def solve(self, b):
        x = np.array(b, dtype=np.float64)
        return self.solveInPlace(x)

    def _matrix(self):
        out = np.zeros((self.n, self.n), order="F")
        check(self.L.pq_dense_factor_matrix(self.h, out.ctypes.data, self.n), "pq_dense_factor_matrix")
        return out

    def last_ms(self):
        """(device time of the factorisation launches, wall time of the whole compute()) of the last compute(), ms"""
        o = np.zeros(2)
        check(self.L.pq_dense_factor_last_ms(self.h, o.ctypes.data), "pq_dense_factor_last_ms")
        return float(o[0]), float(o[1])


class LDLTNoPivot(_DenseFactor):
    """piqp::dense::LDLTNoPivot<Mat, UpLo>: A = L D L^T = U^T D U without pivoting"""
    _kind = DENSE_LDLT_NO_PIVOT

    def matrixLDLT(self):
        """ldlt_no_pivot.hpp:217: the `uplo` triangle holds the strictly triangular part of the unit factor and D on the diagonal (the other triangle: zeros here)"""
        return self._matrix()

    def vectorD(self):
        return np.diag(self._matrix()).copy()

    def matrixL(self):
        m = self._matrix()
        m = m if self.uplo == LOWER else m.T
        return np.tril(m, -1) + np.eye(self.n)

    def matrixU(self):
        return self.matrixL().T

    def reconstructedMatrix(self):
        Lm = self.matrixL()
        return (Lm * self.vectorD()[None, :]) @ Lm.T


class LLT(_DenseFactor):
    """Eigen::LLT<Mat, UpLo> as dense/kkt.hpp:82 uses it: A = L L^T = U^T U"""
    _kind = DENSE_CHOLESKY

    def matrixLLT(self):
        return self._matrix()

    def matrixL(self):
        m = self._matrix()
        return np.tril(m if self.uplo == LOWER else m.T)

    def matrixU(self):
        return self.matrixL().T

    def reconstructedMatrix(self):
        Lm = self.matrixL()
        return Lm @ Lm.T


class _DenseFactorBatch(_Handle):
    """`batch` matrices of order n <= 128, each factored by one workgroup (one wave below n = 32) in one launch: pq_dense_factor_batch_* (include/piqp_amd.h).
    Per matrix the factor, info() and every solve are the reference-order ones of csrc/dense_factor_batch.hip: bit for bit the CPU oracle's."""
    _destroy = "pq_dense_factor_batch_destroy"
    _kind = DENSE_LDLT_NO_PIVOT

    def __init__(self, batch, n, uplo=LOWER, device=0, max_nrhs=1):
        self.L = _lib.load()
        self.batch, self.n, self.uplo, self.device, self.max_nrhs = int(batch), int(n), int(uplo), int(device), int(max_nrhs)
        h = C.c_void_p()
        check(self.L.pq_dense_factor_batch_create(C.byref(h), self.device, self.batch, self.n, self._kind, self.uplo, self.max_nrhs), "pq_dense_factor_batch_create")
        self.h = h
        self.n_success = None

    def compute(self, A):
        """A: numpy [batch, n, n], A[i] the i-th matrix as written (A[i][r, c] = row r, column c); only the `uplo` triangle of each is read."""
        A = np.asarray(A, dtype=np.float64)
        assert A.shape == (self.batch, self.n, self.n)
        Af = np.ascontiguousarray(A.transpose(0, 2, 1))  # [i] column-major
        self.n_success = check(self.L.pq_dense_factor_batch_compute(self.h, Af.ctypes.data, self.n, self.n * self.n, MEM_HOST), "pq_dense_factor_batch_compute")
        return self

    def compute_colmajor(self, tensor_or_ptr, lda=None, stride=None, on_device=True):
        """Matrix i COLUMN-major at address + i * stride doubles, leading dimension lda (default n; stride default lda * n), in a torch CUDA tensor's storage or at a
        raw address; no copy through the host.  A contiguous torch [batch, n, n] tensor is a batch of ROW-major matrices, which this call reads as their column-major
        transposes: `uplo` then names the triangle of the TRANSPOSE, i.e. LOWER reads t[i].triu() (the upper triangle of the row-major matrix) and UPPER reads
        t[i].tril().  For a symmetric matrix that is only a question of which half has to be filled in."""
        p = tensor_or_ptr if isinstance(tensor_or_ptr, int) else _ptr(tensor_or_ptr)
        self._keep = tensor_or_ptr
        lda = self.n if lda is None else int(lda)
        stride = lda * self.n if stride is None else int(stride)
        if on_device:
            sync_current_stream(self.device)
        self.n_success = check(self.L.pq_dense_factor_batch_compute(self.h, p, lda, stride, MEM_DEVICE if on_device else MEM_HOST), "pq_dense_factor_batch_compute")
        return self

    def _status(self):
        info, bad = np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch, dtype=np.int32)
        check(self.L.pq_dense_factor_batch_info(self.h, info.ctypes.data, bad.ctypes.data), "pq_dense_factor_batch_info")
        return info, bad

    def info(self):
        """int array [batch]: 0 = Eigen::Success, 1 = Eigen::NumericalIssue"""
        return self._status()[0]

    def first_bad_col(self):
        """int array [batch]: -1, or the column at which the factorisation of that matrix gave up"""
        return self._status()[1]

    def solveInPlace(self, X, nrhs=None, ldx=None, stride=None, on_device=None):
        """X <- A_i^-1 X_i for every matrix whose factorisation succeeded (the others keep their block).  numpy or torch, C-contiguous: [batch, n] (one right-hand
        side each) or [batch, nrhs, ldx] with ldx >= n -- X[i, c, :n] is column c of matrix i's block, i.e. the blocks are column-major with leading dimension ldx.
        A raw address (int) takes nrhs, ldx, stride (doubles between blocks) and on_device explicitly."""
        if isinstance(X, int):
            p, nrhs, ldx = X, int(nrhs), self.n if ldx is None else int(ldx)
            on_device = True if on_device is None else on_device
        else:
            shape = tuple(X.shape)
            assert (str(X.dtype).endswith("float64")) and shape[0] == self.batch
            assert X.is_contiguous() if _is_torch(X) else X.flags.c_contiguous
            if len(shape) == 2:
                assert shape[1] == self.n
                nrhs, ldx = 1, self.n
            else:
                assert len(shape) == 3 and shape[2] >= self.n
                nrhs, ldx = shape[1], shape[2]
            p, on_device = _ptr(X), _is_torch(X)
        stride = ldx * nrhs if stride is None else int(stride)
        if on_device:
            sync_current_stream(self.device)
        check(self.L.pq_dense_factor_batch_solve_in_place(self.h, p, ldx, nrhs, stride, MEM_DEVICE if on_device else MEM_HOST), "pq_dense_factor_batch_solve_in_place")
        return X

    def solve(self, B):
        """numpy [batch, n] or [batch, nrhs, n] (B[i, c] = right-hand side c of matrix i); returns the solutions in the same shape"""
        return self.solveInPlace(np.array(B, dtype=np.float64, order="C"))

    def _matrix(self, i):
        out = np.zeros((self.n, self.n), order="F")
        check(self.L.pq_dense_factor_batch_matrix(self.h, int(i), out.ctypes.data, self.n), "pq_dense_factor_batch_matrix")
        return out

    def last_ms(self):
        """(device time of the factorisation launch, wall time of the whole compute()) of the last compute(), ms"""
        o = np.zeros(2)
        check(self.L.pq_dense_factor_batch_last_ms(self.h, o.ctypes.data), "pq_dense_factor_batch_last_ms")
        return float(o[0]), float(o[1])


class BatchLDLTNoPivot(_DenseFactorBatch):
    """a batch of piqp::dense::LDLTNoPivot<Mat, UpLo>: A_i = L_i D_i L_i^T = U_i^T D_i U_i without pivoting"""
    _kind = DENSE_LDLT_NO_PIVOT

    def matrixLDLT(self, i):
        """ldlt_no_pivot.hpp:217 for matrix i: the `uplo` triangle holds the strictly triangular part of the unit factor and D on the diagonal (the other: zeros)"""
        return self._matrix(i)

    def vectorD(self, i):
        return np.diag(self._matrix(i)).copy()

    def matrixL(self, i):
        m = self._matrix(i)
        m = m if self.uplo == LOWER else m.T
        return np.tril(m, -1) + np.eye(self.n)

    def matrixU(self, i):
        return self.matrixL(i).T


class BatchLLT(_DenseFactorBatch):
    """a batch of Eigen::LLT<Mat, UpLo>: A_i = L_i L_i^T = U_i^T U_i"""
    _kind = DENSE_CHOLESKY

    def matrixLLT(self, i):
        return self._matrix(i)

    def matrixL(self, i):
        m = self._matrix(i)
        return np.tril(m if self.uplo == LOWER else m.T)

    def matrixU(self, i):
        return self.matrixL(i).T
