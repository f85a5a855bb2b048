"""BatchDenseKKT: `batch` independent instances of piqp::dense::KKT (dense/kkt.hpp:39-160) with common n <= 128, p, m and factorisation kind, behind
pq_kkt_batch_* (include/piqp_amd.h).  One launch assembles and factors every instance, one launch solves, one launch per mat-vec evaluator; per instance every
result is the reference-order one of csrc/dense_kkt_batch.hip: bit for bit the CPU oracle's dense backend."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import VAR_NAMES, check
from .kkt import (DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT, KKT_UPDATE_A, KKT_UPDATE_G, KKT_UPDATE_P, MEM_DEVICE, MEM_HOST, _Handle, _is_torch,
                  check_device_tensor, sync_current_stream)

KKT_BATCH_DENSE_MAX_N = 128  # PQ_KKT_BATCH_DENSE_MAX_N: the n x n square of an instance lives in LDS


def var_shapes(b, n, p, m):
    """name -> shape of the ten [batch, len] vectors of a batch of piqp_amd.Variables"""
    return dict(zip(VAR_NAMES, ((b, n), (b, p), (b, m), (b, m), (b, n), (b, n), (b, m), (b, m), (b, n), (b, n))))


def select_list(instances):
    """the list of a clone(instances) as the library takes it: a contiguous C-int array, one-dimensional and non-empty, made from anything np.asarray takes whose
    entries are integers (ValueError otherwise; no library call in here -- the range of the entries is the library's check)"""
    try:
        a = np.asarray(instances)
    except Exception:
        raise ValueError("instances: a one-dimensional list of integers expected") from None
    if a.ndim != 1 or a.size == 0:
        raise ValueError(f"instances: shape {a.shape}, a one-dimensional, non-empty list expected")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"instances: dtype {a.dtype}, integers expected")
    return np.ascontiguousarray(a, dtype=np.intc)


class _BatchHandle(_Handle):
    """what the batched wrappers share: the argument handling and the one way to wrap a handle that exists already"""
    _dims_fn = None  # the library's getter of (batch, n, p, m) for this kind of handle

    @classmethod
    def _adopt(cls, h, device, kkt_solver, owner=None, **attrs):
        """the wrapper of the existing handle `h`, its dimensions read from the library.  owner: None = the new object owns the handle and destroys it (a clone);
        else the object that owns it, which is kept alive as long as the new one (a borrowed handle)"""
        k = cls.__new__(cls)
        k._owned, k._parent = owner is None, owner
        k.L, k.device, k.kkt_solver, k.h = _lib.load(), int(device), int(kkt_solver), h if isinstance(h, C.c_void_p) else C.c_void_p(h)
        d = [C.c_int() for _ in range(4)]
        check(getattr(k.L, cls._dims_fn)(k.h, *[C.byref(x) for x in d]), cls._dims_fn)
        k.batch, k.n, k.p, k.m = (x.value for x in d)
        for name, v in attrs.items():
            setattr(k, name, v)
        return k

    def _open(self, P, A, G, kkt_solver, device):
        """the start of a constructor from matrices: the library, the device, the kind and batch, n, p, m from the shapes"""
        self.L = _lib.load()
        self.device = int(device)
        if kkt_solver not in (DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT):
            raise ValueError(f"kkt_solver {kkt_solver}: DENSE_CHOLESKY or DENSE_LDLT_NO_PIVOT")
        shape = tuple(P.shape)
        if len(shape) != 3 or shape[1] != shape[2]:
            raise ValueError(f"P: shape {shape}, expected [batch, n, n]")
        self.batch, self.n = int(shape[0]), int(shape[1])
        self.p = 0 if A is None else int(A.shape[1]) if len(A.shape) == 3 else -1
        self.m = 0 if G is None else int(G.shape[1]) if len(G.shape) == 3 else -1
        if self.p < 0 or self.m < 0:
            raise ValueError("A: [batch, p, n] and G: [batch, m, n] expected")
        self.kkt_solver = int(kkt_solver)

    # ---- argument handling: no library call in here
    @staticmethod
    def _p(a):
        if a is None:
            return None
        return a.data_ptr() if _is_torch(a) else a.ctypes.data

    def _one(self, name, a, shape, transpose=False):
        """(array to pass, MEM_*) for one argument of the given shape"""
        if _is_torch(a):
            check_device_tensor(name, a, shape, self.device)
            if not a.is_contiguous():
                raise ValueError(f"{name}: not contiguous")
            return a, MEM_DEVICE
        a = np.asarray(a)
        if a.dtype != np.float64:
            raise TypeError(f"{name}: dtype {a.dtype}, float64 expected")
        if a.shape != tuple(shape):
            raise ValueError(f"{name}: shape {a.shape}, expected {tuple(shape)}")
        if transpose:
            return np.ascontiguousarray(a.transpose(0, 2, 1)), MEM_HOST  # [i] column-major
        if not a.flags.c_contiguous:
            raise ValueError(f"{name}: not C-contiguous")
        return a, MEM_HOST

    def _args(self, *specs):
        """specs: (name, array or None, shape[, transpose]).  Returns (MEM_*, arrays); all arguments that are given must live in the same memory."""
        out, mems = [], set()
        for spec in specs:
            name, a, shape = spec[:3]
            if a is None:
                out.append(None)
                continue
            arr, mem = self._one(name, a, shape, *spec[3:])
            out.append(arr)
            mems.add(mem)
        if len(mems) > 1:
            raise TypeError("numpy arrays and torch tensors in one call: every argument of a call lives in the same memory")
        return (mems.pop() if mems else MEM_HOST), out

    def _out(self, mem, *shape):
        if mem == MEM_DEVICE:
            import torch
            return torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.device}")
        return np.empty(shape, dtype=np.float64)

    def _call(self, mem, fn, *args):
        if mem == MEM_DEVICE:
            sync_current_stream(self.device)
        return check(getattr(self.L, fn)(self.h, *[self._p(a) for a in args], mem), fn)


class BatchDenseKKT(_BatchHandle):
    """BatchDenseKKT(P, A=None, G=None, kkt_solver=DENSE_CHOLESKY, device=0)

    numpy arguments: P [batch, n, n] as written (P[i][r, c] = row r, column c; the upper triangle of each is read), A [batch, p, n], G [batch, m, n], float64;
    the wrapper makes the column-major copies the library takes.
    torch CUDA tensors (float64, contiguous, on `device`) are passed by pointer without a copy.  A contiguous A[i] ([p, n], row-major) already is the column-major
    AT[i].  A contiguous P [batch, n, n] is a batch of ROW-major matrices, which the library reads as their column-major transposes: the upper triangle it reads
    is that of the TRANSPOSE, i.e. P[i].tril() (the lower triangle of the row-major matrix).  For a symmetric P that is only a question of which half has to be
    filled in; NaN in the other half is harmless.
    Vectors are [batch, len], per-instance scalars [batch]; numpy in, numpy out; torch in, torch out on the device.  Every argument of one call lives in the same
    memory.  Wrong dtype, shape, contiguity or device is refused before any library call."""
    _destroy = "pq_kkt_batch_destroy"
    _dims_fn = "pq_kkt_batch_dims"

    def __init__(self, P, A=None, G=None, kkt_solver=DENSE_CHOLESKY, device=0):
        self._open(P, A, G, kkt_solver, device)
        mem, (Pm, Am, Gm) = self._matrices(P, A, G)
        h = C.c_void_p()
        if mem == MEM_DEVICE:
            sync_current_stream(self.device)
        check(self.L.pq_kkt_batch_create_dense(C.byref(h), self.device, self.batch, self.n, self.p, self.m, self.kkt_solver, self._p(Pm), self._p(Am), self._p(Gm), mem),
              "pq_kkt_batch_create_dense")
        self.h = h

    # ---- argument handling: no library call in here
    def _matrices(self, P, A, G):
        b, n = self.batch, self.n
        return self._args(("P", P, (b, n, n), True), ("A", A, (b, self.p, n)), ("G", G, (b, self.m, n)))

    # ---- the KKTSolverBase surface, per instance
    def clone(self, instances=None):
        """a handle of its own in the state of this one; instances: None = every instance, else a list of instances (repeats allowed, any length >= 1): instance j
        of the clone is instance instances[j] of this handle"""
        h = C.c_void_p()
        if instances is None:
            check(self.L.pq_kkt_batch_clone(self.h, C.byref(h)), "pq_kkt_batch_clone")
        else:
            idx = select_list(instances)
            check(self.L.pq_kkt_batch_clone_select(self.h, idx.ctypes.data, len(idx), C.byref(h)), "pq_kkt_batch_clone_select")
        return self._adopt(h, self.device, self.kkt_solver)

    def update_data(self, P=None, A=None, G=None):
        """re-reads the matrices that are given (layouts as in the constructor); a new A recomputes A' A"""
        mem, (Pm, Am, Gm) = self._matrices(P, A, G)
        options = (KKT_UPDATE_P if P is not None else 0) | (KKT_UPDATE_A if A is not None else 0) | (KKT_UPDATE_G if G is not None else 0)
        if mem == MEM_DEVICE:
            sync_current_stream(self.device)
        check(self.L.pq_kkt_batch_update_data_dense(self.h, self._p(Pm), self._p(Am), self._p(Gm), options, mem), "pq_kkt_batch_update_data_dense")

    def update_scalings_and_factor(self, delta, x_reg, z_reg):
        """delta [batch], x_reg [batch, n], z_reg [batch, m]; returns the number of instances that factored"""
        b = self.batch
        mem, (d, x, z) = self._args(("delta", delta, (b,)), ("x_reg", x_reg, (b, self.n)), ("z_reg", z_reg, (b, self.m)))
        return self._call(mem, "pq_kkt_batch_update_scalings_and_factor", d, x, z)

    def _status(self):
        ok, bad = np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch, dtype=np.int32)
        check(self.L.pq_kkt_batch_info(self.h, ok.ctypes.data, bad.ctypes.data), "pq_kkt_batch_info")
        return ok, bad

    def ok(self):
        """bool array [batch]: the instance's last factorisation succeeded"""
        return self._status()[0].astype(bool)

    def first_bad_col(self):
        """int array [batch]: -1, or the column at which the factorisation of that instance gave up"""
        return self._status()[1]

    def solve(self, rhs_x, rhs_y, rhs_z, out=None):
        """returns (lhs_x, lhs_y, lhs_z); the blocks of an instance whose factorisation failed are left as they are (out: the three arrays to write into)"""
        b = self.batch
        shapes = ((b, self.n), (b, self.p), (b, self.m))
        mem, rhs = self._args(*[(nm, a, s) for nm, a, s in zip(("rhs_x", "rhs_y", "rhs_z"), (rhs_x, rhs_y, rhs_z), shapes)])
        if out is None:
            lhs = [self._out(mem, *s) for s in shapes]
        else:
            omem, lhs = self._args(*[(nm, a, s) for nm, a, s in zip(("lhs_x", "lhs_y", "lhs_z"), out, shapes)])
            if omem != mem:
                raise TypeError("out: not in the memory of the right-hand sides")
            lhs = list(out)
        self._call(mem, "pq_kkt_batch_solve", *rhs, *lhs)
        return tuple(lhs)

    def eval_P_x(self, alpha, x, out=None):
        b = self.batch
        mem, (a, xx, z) = self._args(("alpha", alpha, (b,)), ("x", x, (b, self.n)), ("z", out, (b, self.n)))
        z = self._out(mem, b, self.n) if out is None else out
        self._call(mem, "pq_kkt_batch_eval_P_x", a, xx, z)
        return z

    def _eval_nt(self, fn, cols, alpha_n, alpha_t, xn, xt, out):
        b = self.batch
        zn, zt = out if out is not None else (None, None)
        mem, (an, at, a, t, _, _) = self._args(("alpha_n", alpha_n, (b,)), ("alpha_t", alpha_t, (b,)), ("xn", xn, (b, self.n)), ("xt", xt, (b, cols)),
                                               ("zn", zn, (b, cols)), ("zt", zt, (b, self.n)))
        if out is None:
            zn, zt = self._out(mem, b, cols), self._out(mem, b, self.n)
        self._call(mem, fn, an, at, a, t, zn, zt)
        return zn, zt

    def eval_A_xn_and_AT_xt(self, alpha_n, alpha_t, xn, xt, out=None):
        """(zn, zt) = (alpha_n A xn, alpha_t A' xt) per instance; xn [batch, n], xt [batch, p]"""
        return self._eval_nt("pq_kkt_batch_eval_A_xn_and_AT_xt", self.p, alpha_n, alpha_t, xn, xt, out)

    def eval_G_xn_and_GT_xt(self, alpha_n, alpha_t, xn, xt, out=None):
        """(zn, zt) = (alpha_n G xn, alpha_t G' xt) per instance; xn [batch, n], xt [batch, m]"""
        return self._eval_nt("pq_kkt_batch_eval_G_xn_and_GT_xt", self.m, alpha_n, alpha_t, xn, xt, out)

    def internal_kkt_mat(self, i):
        """n x n: the KKT matrix of instance i, RECOMPUTED from the stored data and the scalings of the last factorisation (lower triangle meaningful)"""
        out = np.zeros((self.n, self.n), order="F")
        check(self.L.pq_kkt_batch_internal_kkt_mat(self.h, int(i), out.ctypes.data), "pq_kkt_batch_internal_kkt_mat")
        return out

    def internal_factor(self, i):
        """n x n: the stored factor of instance i (lower triangle; LDLT: unit L below D)"""
        out = np.zeros((self.n, self.n), order="F")
        check(self.L.pq_kkt_batch_internal_factor(self.h, int(i), out.ctypes.data), "pq_kkt_batch_internal_factor")
        return out

    def last_ms(self):
        """(device time of the last factorisation launch, device time of the last solve launch, wall time of the last update_scalings_and_factor call), ms"""
        o = np.zeros(3)
        check(self.L.pq_kkt_batch_last_ms(self.h, o.ctypes.data), "pq_kkt_batch_last_ms")
        return float(o[0]), float(o[1]), float(o[2])
