"""BatchKKTSystem: `batch` instances of piqp::KKTSystem (kkt_system.hpp) over the batched dense KKT backend (n <= 128), behind pq_kktsys_batch_* (include/piqp_amd.h).
update_scalings_and_factor, solve (with the iterative-refinement loop of every instance inside its own workgroup) and mul are one launch each; per instance every
result is bit for bit the CPU oracle's (csrc/dense_kktsys_batch.hip)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import VAR_NAMES, check
from .batch_kkt import BatchDenseKKT, _BatchHandle, select_list, var_shapes
from .kkt import DENSE_CHOLESKY, KKT_UPDATE_A, KKT_UPDATE_G, KKT_UPDATE_P, MEM_DEVICE, MEM_HOST, _is_torch, default_settings, sync_current_stream

STATE_X_REG, STATE_Z_REG, STATE_RHS_X_BAR, STATE_RHS_Z_BAR = 0, 1, 2, 3  # PQ_KKTSYS_BATCH_*
MAX_REFINE_ITER = 64


def _copy_settings(s):
    c = _lib.Settings()
    C.memmove(C.byref(c), C.byref(s), C.sizeof(c))
    return c


class BatchKKTSystem(_BatchHandle):
    """BatchKKTSystem(P, A=None, G=None, h_l_idx=None, h_u_idx=None, x_l_idx=None, x_u_idx=None, x_b_scaling=None, settings=None, kkt_solver=DENSE_CHOLESKY, device=0)

    Matrices as for BatchDenseKKT: P [batch, n, n], A [batch, p, n], G [batch, m, n].  The four finite-bound index lists are shared by the batch, ascending, host
    integers; h_l_idx / h_u_idx default to every row of G (each row must be in at least one of them), x_l_idx / x_u_idx to no box bound.  x_b_scaling [batch, n] (default
    ones) lives where the matrices live.  settings: a piqp_amd.default_settings() structure shared by the batch (its kkt_solver field is replaced by `kkt_solver`).
    A batch of variables is a dict of [batch, len] arrays under the names of piqp_amd.Variables (x, y, z_l, z_u, z_bl, z_bu, s_l, s_u, s_bl, s_bu; len = n, p, m, m, n,
    n, m, m, n, n); of the box vectors the first len(x_l_idx) / len(x_u_idx) entries of a row are meaningful.  An entry whose vector has no meaningful part may be
    missing.  BatchKKTSystem.per_instance(P, A, G, lists, ...) makes a system in which every instance has lists of its own.  numpy in, numpy out; torch CUDA tensors by pointer, torch out; every array of one call lives in the same memory; wrong dtype, shape, contiguity or device
    is refused before any library call."""
    _destroy = "pq_kktsys_batch_destroy"
    _dims_fn = "pq_kktsys_batch_dims"
    per_inst = False  # True: self.lists is a list of `batch` 4-tuples, one per instance (BatchKKTSystem.per_instance)

    def _open_settings(self, P, A, G, settings, kkt_solver, device):
        self._open(P, A, G, kkt_solver, device)
        self.settings = _copy_settings(settings if settings is not None else default_settings())
        self.settings.kkt_solver = self.kkt_solver
        if not 0 <= self.settings.iterative_refinement_max_iter <= MAX_REFINE_ITER:
            raise ValueError(f"iterative_refinement_max_iter {self.settings.iterative_refinement_max_iter}: [0, {MAX_REFINE_ITER}] (the loop runs inside a kernel)")

    def __init__(self, P, A=None, G=None, h_l_idx=None, h_u_idx=None, x_l_idx=None, x_u_idx=None, x_b_scaling=None, settings=None, kkt_solver=DENSE_CHOLESKY, device=0):
        self._open_settings(P, A, G, settings, kkt_solver, device)
        every = np.arange(self.m, dtype=np.int32)
        self.lists = tuple(self._list(name, v, default, length) for name, v, default, length in (
            ("h_l_idx", h_l_idx, every, self.m), ("h_u_idx", h_u_idx, every, self.m), ("x_l_idx", x_l_idx, every[:0], self.n), ("x_u_idx", x_u_idx, every[:0], self.n)))
        if self.m and len(np.union1d(self.lists[0], self.lists[1])) != self.m:
            raise ValueError("every row of G must be in h_l_idx or h_u_idx")
        mem, (Pm, Am, Gm, xbs) = self._args(("P", P, (self.batch, self.n, self.n), True), ("A", A, (self.batch, self.p, self.n)), ("G", G, (self.batch, self.m, self.n)),
                                            ("x_b_scaling", x_b_scaling, (self.batch, self.n)))
        h = C.c_void_p()
        if mem == MEM_DEVICE:
            sync_current_stream(self.device)
        check(self.L.pq_kktsys_batch_create_dense(C.byref(h), self.device, self.batch, self.n, self.p, self.m, self._p(Pm), self._p(Am), self._p(Gm),
                                                  *[len(l) for l in self.lists], *[l.ctypes.data for l in self.lists], self._p(xbs), C.byref(self.settings), mem),
              "pq_kktsys_batch_create_dense")
        self.h = h

    @classmethod
    def per_instance(cls, P, A, G, lists, x_b_scaling=None, settings=None, kkt_solver=DENSE_CHOLESKY, device=0):
        """the same system with finite-bound lists of its own for every instance: `lists` is a sequence of `batch` 4-tuples (h_l_idx, h_u_idx, x_l_idx, x_u_idx) of
        ascending integer lists, each under the rules of the constructor (None: its default there).  Of the box vectors of a batch of variables the first
        len(x_l_idx) / len(x_u_idx) entries of row i are meaningful for instance i; a box vector has to be passed when any instance uses it.  set_lists(lists)
        replaces the lists later (a new update_scalings_and_factor has to follow)."""
        k = cls.__new__(cls)
        k._open_settings(P, A, G, settings, kkt_solver, device)
        k.per_inst = True
        k.lists, packed = k._pack_lists(lists)
        mem, (Pm, Am, Gm, xbs) = k._args(("P", P, (k.batch, k.n, k.n), True), ("A", A, (k.batch, k.p, k.n)), ("G", G, (k.batch, k.m, k.n)),
                                         ("x_b_scaling", x_b_scaling, (k.batch, k.n)))
        h = C.c_void_p()
        if mem == MEM_DEVICE:
            sync_current_stream(k.device)
        check(k.L.pq_kktsys_batch_create_dense_lists(C.byref(h), k.device, k.batch, k.n, k.p, k.m, k._p(Pm), k._p(Am), k._p(Gm), *[a.ctypes.data for a in packed], k._p(xbs),
                                                     C.byref(k.settings), mem), "pq_kktsys_batch_create_dense_lists")
        k.h = h
        return k

    def set_lists(self, lists):
        """other lists for every instance of a per_instance system (validated as there, before the library call); allocates nothing on the device"""
        if not self.per_inst or self.lists is None:
            raise RuntimeError("set_lists: the lists of this BatchKKTSystem are shared by the batch (or it is borrowed)")
        new, packed = self._pack_lists(lists)
        check(self.L.pq_kktsys_batch_set_lists(self.h, *[a.ctypes.data for a in packed]), "pq_kktsys_batch_set_lists")
        self.lists = new

    # ---- argument handling: no library call in here
    def _pack_lists(self, lists):
        """(the validated per-instance lists, [counts [batch, 4], h_l_idx [batch, m], h_u_idx [batch, m], x_l_idx [batch, n], x_u_idx [batch, n]] as int32)"""
        try:
            lists = [tuple(t) for t in lists]
        except TypeError:
            raise TypeError("lists: a sequence of `batch` 4-tuples of index lists expected") from None
        if len(lists) != self.batch or any(len(t) != 4 for t in lists):
            raise ValueError(f"lists: {self.batch} 4-tuples (h_l_idx, h_u_idx, x_l_idx, x_u_idx) expected")
        every = np.arange(self.m, dtype=np.int32)
        lens = (self.m, self.m, self.n, self.n)
        counts = np.zeros((self.batch, 4), dtype=np.int32)
        packed = [np.zeros((self.batch, max(l, 1)), dtype=np.int32) for l in lens]
        out = []
        for i, t in enumerate(lists):
            one = tuple(self._list(f"lists[{i}].{name}", v, default, length) for name, v, default, length in (
                ("h_l_idx", t[0], every, self.m), ("h_u_idx", t[1], every, self.m), ("x_l_idx", t[2], every[:0], self.n), ("x_u_idx", t[3], every[:0], self.n)))
            if self.m and len(np.union1d(one[0], one[1])) != self.m:
                raise ValueError(f"lists[{i}]: every row of G must be in h_l_idx or h_u_idx")
            for k, a in enumerate(one):
                counts[i, k] = len(a)
                packed[k][i, :len(a)] = a
            out.append(one)
        return out, [counts] + packed

    @staticmethod
    def _list(name, v, default, length):
        if v is None:
            return default.copy()
        a = np.asarray(v)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise TypeError(f"{name}: a one-dimensional integer list expected")
        a = np.ascontiguousarray(a, dtype=np.int32)
        if a.size > length or (a.size and (a.min() < 0 or a.max() >= length)) or np.any(np.diff(a) <= 0):
            raise ValueError(f"{name}: strictly ascending indices in [0, {length}) expected")
        return a

    def var_shapes(self):
        return var_shapes(self.batch, self.n, self.p, self.m)

    def _used(self, name):
        if name in ("z_bl", "s_bl", "z_bu", "s_bu"):
            k = 2 if name in ("z_bl", "s_bl") else 3
            return any(len(t[k]) > 0 for t in self.lists) if self.per_inst else len(self.lists[k]) > 0
        return self.var_shapes()[name][1] > 0

    def _vars(self, what, v, names=VAR_NAMES):
        """(MEM_*, dict name -> array or None) for a batch of variables: every vector with a meaningful part must be there"""
        if self.lists is None:
            raise RuntimeError("this BatchKKTSystem is borrowed from a BatchDenseSolver, which does not hand out its bound lists: calls that take variables "
                               "(update_scalings_and_factor, solve, mul) are not available; the read-only hooks are (x_reg, z_reg, rhs_x_bar, rhs_z_bar, solve_ok, "
                               "refine_steps, backend_solves, refine_error, rhs_norm, last_ms, backend)")
        shapes = self.var_shapes()
        for name in names:
            if self._used(name) and v.get(name) is None:
                raise ValueError(f"{what}: {name} is missing")
        mem, arrs = self._args(*[(f"{what}.{name}", v.get(name) if self._used(name) else None, shapes[name]) for name in names])
        return mem, dict(zip(names, arrs))

    def _struct(self, d):
        s = _lib.Vars()
        for name in VAR_NAMES:
            setattr(s, name, self._p(d.get(name)))
        return s

    def _new_vars(self, mem):
        if mem == MEM_DEVICE:
            import torch
            return {k: torch.zeros(s, dtype=torch.float64, device=f"cuda:{self.device}") for k, s in self.var_shapes().items()}
        return {k: np.zeros(s) for k, s in self.var_shapes().items()}

    # ---- the KKTSystem surface, per instance
    def clone(self, instances=None):
        """a system of its own in the state of this one; instances: None = every instance, else a list of instances (repeats allowed, any length >= 1): instance j
        of the clone is instance instances[j] of this system, with that instance's lists when every instance has its own"""
        h = C.c_void_p()
        lists = self.lists
        if instances is None:
            check(self.L.pq_kktsys_batch_clone(self.h, C.byref(h)), "pq_kktsys_batch_clone")
        else:
            idx = select_list(instances)
            check(self.L.pq_kktsys_batch_clone_select(self.h, idx.ctypes.data, len(idx), C.byref(h)), "pq_kktsys_batch_clone_select")
            if self.per_inst and lists is not None:
                lists = [lists[i] for i in idx]
        return self._adopt(h, self.device, self.kkt_solver, lists=lists, per_inst=self.per_inst, settings=_copy_settings(self.settings))

    def backend(self):
        """the BatchDenseKKT this system owns (borrowed: it lives as long as this object)"""
        return BatchDenseKKT._adopt(self.L.pq_kktsys_batch_backend(self.h), self.device, self.kkt_solver, owner=self)

    def update_data(self, P=None, A=None, G=None, x_b_scaling=None):
        """re-reads what is given (layouts as in the constructor); a new A recomputes A' A"""
        mem, (Pm, Am, Gm, xbs) = self._args(("P", P, (self.batch, self.n, self.n), True), ("A", A, (self.batch, self.p, self.n)), ("G", G, (self.batch, self.m, self.n)),
                                            ("x_b_scaling", x_b_scaling, (self.batch, self.n)))
        options = (KKT_UPDATE_P if P is not None else 0) | (KKT_UPDATE_A if A is not None else 0) | (KKT_UPDATE_G if G is not None else 0)
        if mem == MEM_DEVICE:
            sync_current_stream(self.device)
        check(self.L.pq_kktsys_batch_update_data_dense(self.h, self._p(Pm), self._p(Am), self._p(Gm), self._p(xbs), options, mem), "pq_kktsys_batch_update_data_dense")

    def set_settings(self, settings):
        s = _copy_settings(settings)
        s.kkt_solver = self.kkt_solver
        check(self.L.pq_kktsys_batch_set_settings(self.h, C.byref(s)), "pq_kktsys_batch_set_settings")
        self.settings = s

    def update_scalings_and_factor(self, iterative_refinement, rho, delta, vars):
        """iterative_refinement: None (off everywhere), one bool for the batch, or an int32 [batch] array (a torch int32 tensor beside torch data); rho, delta [batch];
        vars: the interior-point state (the eight s / z vectors are read).  Returns the number of instances that factored."""
        b = self.batch
        mem, v = self._vars("vars", vars, VAR_NAMES[2:])
        m2, (r, d) = self._args(("rho", rho, (b,)), ("delta", delta, (b,)))
        if m2 != mem and any(self._used(nm) for nm in VAR_NAMES[2:]):
            raise TypeError("rho, delta: not in the memory of the variables")
        mem = m2
        flags = iterative_refinement
        if flags is not None and not _is_torch(flags):
            flags = np.ascontiguousarray(np.broadcast_to(np.asarray(flags).astype(np.int32), (b,)))
            if mem == MEM_DEVICE:
                import torch
                flags = torch.from_numpy(flags).to(f"cuda:{self.device}")
        elif flags is not None:
            import torch
            if flags.dtype != torch.int32 or tuple(flags.shape) != (b,) or not flags.is_cuda or flags.device.index != self.device or not flags.is_contiguous() or mem != MEM_DEVICE:
                raise TypeError("iterative_refinement: a contiguous int32 CUDA tensor [batch] beside torch data expected")
        if mem == MEM_DEVICE:
            sync_current_stream(self.device)
        vs = self._struct(v)
        return check(self.L.pq_kktsys_batch_update_scalings_and_factor(self.h, self._p(flags), self._p(r), self._p(d), C.byref(vs), mem), "pq_kktsys_batch_update_scalings_and_factor")

    def solve(self, rhs, out=None):
        """returns a dict of the ten [batch, len] vectors of the step; the rows of an instance whose factorisation failed are left as they are (out: the dict to write
        into).  solve_ok() tells which instances solved."""
        mem, r = self._vars("rhs", rhs)
        if out is None:
            out = self._new_vars(mem)
        omem, o = self._vars("out", out)
        if omem != mem:
            raise TypeError("out: not in the memory of the right-hand sides")
        if mem == MEM_DEVICE:
            sync_current_stream(self.device)
        rs, ls = self._struct(r), self._struct(o)
        check(self.L.pq_kktsys_batch_solve(self.h, C.byref(rs), C.byref(ls), mem), "pq_kktsys_batch_solve")
        return out

    def mul(self, lhs, out=None):
        """rhs = K lhs with the scalings of the last update_scalings_and_factor, a dict of ten [batch, len] vectors"""
        mem, l = self._vars("lhs", lhs)
        if out is None:
            out = self._new_vars(mem)
        omem, o = self._vars("out", out)
        if omem != mem:
            raise TypeError("out: not in the memory of lhs")
        if mem == MEM_DEVICE:
            sync_current_stream(self.device)
        ls, rs = self._struct(l), self._struct(o)
        check(self.L.pq_kktsys_batch_mul(self.h, C.byref(ls), C.byref(rs), mem), "pq_kktsys_batch_mul")
        return out

    def _info(self, pos, dtype):
        a = np.zeros(self.batch, dtype=dtype)
        args = [None] * 5
        args[pos] = a.ctypes.data
        check(self.L.pq_kktsys_batch_info(self.h, *args), "pq_kktsys_batch_info")
        return a

    def solve_ok(self):
        """bool [batch]: the last solve of the instance ended with finite numbers (and its factorisation had succeeded)"""
        return self._info(0, np.int32).astype(bool)

    def refine_steps(self):
        return self._info(1, np.int32)

    def backend_solves(self):
        return self._info(2, np.int32)

    def refine_error(self):
        return self._info(3, np.float64)

    def rhs_norm(self):
        return self._info(4, np.float64)

    def _state(self, what, length):
        a = np.zeros((self.batch, length))
        check(self.L.pq_kktsys_batch_state(self.h, what, a.ctypes.data), "pq_kktsys_batch_state")
        return a

    def x_reg(self):
        """[batch, n]: what the backend was given (with the static regularisation of refinement)"""
        return self._state(STATE_X_REG, self.n)

    def z_reg(self):
        """[batch, m]: without the static regularisation"""
        return self._state(STATE_Z_REG, self.m)

    def rhs_x_bar(self):
        return self._state(STATE_RHS_X_BAR, self.n)

    def rhs_z_bar(self):
        return self._state(STATE_RHS_Z_BAR, self.m)

    def last_ms(self):
        """device time of the last factor, solve and mul launch, ms"""
        o = np.zeros(3)
        check(self.L.pq_kktsys_batch_last_ms(self.h, o.ctypes.data), "pq_kktsys_batch_last_ms")
        return float(o[0]), float(o[1]), float(o[2])
