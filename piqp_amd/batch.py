"""Batched sparse solver over pq_batch_*: many structurally identical QPs, one workgroup per QP, one kernel launch.

Equivalent of looping the reference's `SparseSolver::setup(...); solve();` (solver.hpp:1293-1322) over the instances with
kkt_solver = sparse_multistage (the default here) or sparse_ldlt (the reference's own default: full KKT matrix, AMD order, up-looking LDLt, bitwise the
reference's factor; n + p + m <= 8192).  Patterns are shared; values are stacked along a leading batch axis.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import VAR_NAMES, check
from .batch_kkt import select_list
from .kkt import MEM_DEVICE, MEM_HOST, _Handle, _ptr, device_call, sync_current_stream, to_device_args


BOUND_SETS = {"shared": 0, "per_instance": 1}  # PQ_BOUND_SETS_*


class BatchSparseSolver(_Handle):
    _destroy = "pq_batch_destroy"

    def __init__(self, device=0, kkt_solver=None, bounds="shared"):
        """kkt_solver: None (sparse_multistage), SPARSE_MULTISTAGE, SPARSE_LDLT or SPARSE_LDLT_EXACT; settings.kkt_solver may also be set before setup().
        bounds: "shared" -- one set of finite bounds for the batch: setup and the updates refuse an instance that differs -- or "per_instance": every instance has
        the lists SparseSolver would hold for its own vectors, at setup and after every update (pq_batch_set_bound_sets), so a row of G or a box can be switched
        off per instance with -/+ inf and come back later.  In that mode pass G_values to update_data() together with bounds that re-enable a row that had no
        finite bound: its entries of G were zeroed when it was dropped and stay zero until new values are given (the row then reads h_l <= 0 <= h_u)."""
        if bounds not in BOUND_SETS:
            raise ValueError(f"bounds must be one of {sorted(BOUND_SETS)}, got {bounds!r}")
        self.L = _lib.load()
        h = C.c_void_p()
        check(self.L.pq_batch_create(C.byref(h), device), "pq_batch_create")
        self.h = h
        self.device = device
        self.batch = self.n = self.p = self.m = 0
        self._nnz = (0, 0, 0)
        self.bounds = bounds
        if kkt_solver is not None:
            self.settings.kkt_solver = int(kkt_solver)
        if bounds != "shared":
            check(self.L.pq_batch_set_bound_sets(self.h, BOUND_SETS[bounds]), "pq_batch_set_bound_sets")

    @property
    def settings(self):
        return self.L.pq_batch_settings(self.h).contents

    def clone(self, instances=None):
        """a second solver in the state of this one without a new setup (pq_batch_clone / pq_batch_clone_select): the whole batch, or instance j of the new solver is
        instance instances[j] of this one (repeats allowed, any count).  Settings, data, scalings, iterates, results, infos and the factors of kkt_factor() go along
        bit for bit; the two solvers are independent afterwards.  Scenario fan-out: s.clone([0] * S).update(b=...); stragglers:
        s.clone(np.flatnonzero(s.statuses() != SOLVED))."""
        h = C.c_void_p()
        if instances is None:
            check(self.L.pq_batch_clone(self.h, C.byref(h)), "pq_batch_clone")
            batch = self.batch
        else:
            idx = select_list(instances)
            check(self.L.pq_batch_clone_select(self.h, idx.ctypes.data, len(idx), C.byref(h)), "pq_batch_clone_select")
            batch = len(idx)
        c = type(self).__new__(type(self))
        c.L, c.h, c.device, c.bounds = self.L, h, self.device, self.bounds
        c.batch, c.n, c.p, c.m, c._nnz = batch, self.n, self.p, self.m, self._nnz
        return c

    def clone_ms(self):
        """of the clone() that made this solver: dict(wall_ms, device_ms -- the gathers); zeros on a solver that is no clone"""
        o = np.zeros(2)
        check(self.L.pq_batch_clone_ms(self.h, o.ctypes.data), "pq_batch_clone_ms")
        return dict(wall_ms=float(o[0]), device_ms=float(o[1]))

    @staticmethod
    def _pattern(M):
        import scipy.sparse as sp
        if M is None:
            return None, None, None
        M = sp.csc_matrix(M)
        M.sort_indices()
        return np.ascontiguousarray(M.indptr, dtype=np.int32), np.ascontiguousarray(M.indices, dtype=np.int32), M

    @staticmethod
    def _stack(a, batch, length):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == (batch, length), (a.shape, (batch, length))
        return a

    def arena_stride(self):
        """doubles per instance of the device arena: what a clone gathers per instance (pq_batch_arena_stride)"""
        return int(check(self.L.pq_batch_arena_stride(self.h), "pq_batch_arena_stride"))

    def setup(self, P_pattern, P_values, c, A_pattern=None, A_values=None, b=None, G_pattern=None, G_values=None, h_l=None, h_u=None, x_l=None, x_u=None):
        """*_pattern: scipy sparse matrices giving the (sorted CSC) patterns of P (n x n), A (p x n), G (m x n);
        *_values: [batch, nnz] arrays in that CSC order; vectors: [batch, len].
        If any of the value stacks or vectors is a torch CUDA tensor (float64, on the solver's GPU) the setup reads them all where they are
        (pq_batch_setup_sparse_mem): numpy arguments beside them are moved to the GPU, strided views are made contiguous, torch's current stream is drained.
        Nothing but instance 0's four bound vectors comes back to the host.  NumPy arguments alone take the same path behind one upload (pq_batch_setup_sparse):
        the result is the same bit for bit."""
        Pp, Pi, Pm = self._pattern(P_pattern)
        Ap, Ai, Am = self._pattern(A_pattern)
        Gp, Gi, Gm = self._pattern(G_pattern)
        n = Pm.shape[0]
        p = 0 if Am is None else Am.shape[0]
        m = 0 if Gm is None else Gm.shape[0]
        nnz = (Pm.nnz, 0 if Am is None else Am.nnz, 0 if Gm is None else Gm.nnz)
        batch = c.shape[0] if hasattr(c, "shape") else np.asarray(c).shape[0]
        if device_call((P_values, c, A_values, b, G_values, h_l, h_u, x_l, x_u)):
            no_A, no_G = Am is None, Gm is None
            args = dict(P_values=P_values, c=c, A_values=None if no_A else A_values, b=None if no_A else b, G_values=None if no_G else G_values,
                        h_l=None if no_G else h_l, h_u=None if no_G else h_u, x_l=x_l, x_u=x_u)
            shapes = dict(P_values=(batch, nnz[0]), A_values=(batch, nnz[1]), G_values=(batch, nnz[2]), c=(batch, n), b=(batch, p), h_l=(batch, m), h_u=(batch, m),
                          x_l=(batch, n), x_u=(batch, n))
            k, _ = to_device_args(args, shapes, self.device)
            sync_current_stream(self.device)
            keep = [Pp, Pi, k["P_values"], k["c"], Ap, Ai, k["A_values"], k["b"], Gp, Gi, k["G_values"], k["h_l"], k["h_u"], k["x_l"], k["x_u"]]
            ok = bool(check(self.L.pq_batch_setup_sparse_mem(self.h, batch, n, p, m, *[_ptr(a) for a in keep], MEM_DEVICE), "pq_batch_setup_sparse"))
            self.batch, self.n, self.p, self.m, self._nnz = batch, n, p, m, nnz
            return ok
        keep = [Pp, Pi, self._stack(P_values, batch, Pm.nnz), self._stack(c, batch, n),
                Ap, Ai, None if Am is None else self._stack(A_values, batch, Am.nnz), None if Am is None else self._stack(b, batch, p),
                Gp, Gi, None if Gm is None else self._stack(G_values, batch, Gm.nnz),
                None if Gm is None else self._stack(h_l, batch, m), None if Gm is None else self._stack(h_u, batch, m),
                self._stack(x_l, batch, n), self._stack(x_u, batch, n)]
        ok = bool(check(self.L.pq_batch_setup_sparse(self.h, batch, n, p, m, *[_ptr(a) for a in keep]), "pq_batch_setup_sparse"))
        self.batch, self.n, self.p, self.m = batch, n, p, m
        self._nnz = (Pm.nnz, 0 if Am is None else Am.nnz, 0 if Gm is None else Gm.nnz)
        return ok

    def last_ingest(self):
        """of the last setup / update, from the shapes (pq_batch_last_ingest): dict(link_bytes -- problem data moved across the host-device link: 8 x batch x the
        lengths given in a host call (a setup included: the upload of its staging buffer), 0 in a device update, the fetch of instance 0's bound vectors in a device
        setup --, kernel_bytes -- written into the arena by the ingest kernels: the same figure for a host and a device call of the same data)"""
        o = np.zeros(2, dtype=np.int64)
        check(self.L.pq_batch_last_ingest(self.h, o.ctypes.data), "pq_batch_last_ingest")
        return dict(link_bytes=int(o[0]), kernel_bytes=int(o[1]))

    def setup_ms(self):
        """of the last setup(): dict(wall_ms, analysis_ms -- host: symbolic analysis, maps, tables --, device_ms -- arena fill, equilibration, prepare; from host
        arrays the interval starts before their upload into the staging buffer)"""
        o = np.zeros(3)
        check(self.L.pq_batch_setup_ms(self.h, o.ctypes.data), "pq_batch_setup_ms")
        return dict(wall_ms=float(o[0]), analysis_ms=float(o[1]), device_ms=float(o[2]))

    def _device_args(self, args, rows=None):
        """torch CUDA tensors (numpy arguments beside them are moved to the GPU), checked and contiguous; torch's current stream is drained.
        rows: the leading length of the stacks (None: the batch; the length of the list of a call with instances)"""
        B = self.batch if rows is None else rows
        shapes = dict(P_values=(B, self._nnz[0]), A_values=(B, self._nnz[1]), G_values=(B, self._nnz[2]), c=(B, self.n), b=(B, self.p), h_l=(B, self.m), h_u=(B, self.m),
                      x_l=(B, self.n), x_u=(B, self.n))
        keep, _ = to_device_args(args, shapes, self.device)
        sync_current_stream(self.device)
        return keep

    @staticmethod
    def _instances(instances, unique):
        """the list of a call with instances (select_list); unique: ValueError for an instance listed twice -- two workgroups would work on one instance.  No
        library call in here: the range of the entries is the library's check."""
        idx = select_list(instances)
        if unique and len(np.unique(idx)) != len(idx):
            seen = {}
            for j, i in enumerate(idx.tolist()):
                if i in seen:
                    raise ValueError(f"instances[{j}] = {i} is listed twice (instances[{seen[i]}] too)")
                seen[i] = j
        return idx

    @staticmethod
    def _rows(name, a, rows, length):
        """a host stack of a call with instances: float64, contiguous, (len(instances), length) -- ValueError otherwise"""
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (rows, length):
            raise ValueError(f"{name}: shape {a.shape}, expected {(rows, length)} (one row per listed instance)")
        return a

    def _update_select(self, instances, mats, vecs):
        """update(instances=...) / update_data(instances=...): row j of every stack is for instance instances[j]"""
        idx = self._instances(instances, unique=True)
        R = len(idx)
        lens = dict(P_values=self._nnz[0], A_values=self._nnz[1], G_values=self._nnz[2], c=self.n, b=self.p, h_l=self.m, h_u=self.m, x_l=self.n, x_u=self.n)
        args = {**(mats or {}), **vecs}
        if device_call(args.values()):
            keep = self._device_args(args, R)
            mem = MEM_DEVICE
        else:
            keep = {k: self._rows(k, a, R, lens[k]) for k, a in args.items()}
            mem = MEM_HOST
        ptrs = [_ptr(a) for a in keep.values()]
        if mats is None:
            return bool(check(self.L.pq_batch_update_select_mem(self.h, idx.ctypes.data, R, *ptrs, mem), "pq_batch_update_select_mem"))
        return bool(check(self.L.pq_batch_update_data_select_mem(self.h, idx.ctypes.data, R, *ptrs, mem), "pq_batch_update_data_select_mem"))

    def update(self, c=None, b=None, h_l=None, h_u=None, x_l=None, x_u=None, instances=None):
        """new vectors for every instance ([batch, len] arrays, None = unchanged); matrices and the set of finite bounds stay (bounds="per_instance": the
        lists follow the vectors, see __init__).
        If any argument is a torch CUDA tensor the kernels read the data where it is (pq_batch_update_mem).
        instances: a list of distinct instances -- the arrays are [len(instances), len], row j for instance instances[j]; those instances alone are updated, in
        place, bit for bit as the whole-batch call given the same rows would, and nothing of any other instance is written (pq_batch_update_select_mem)."""
        if instances is not None:
            return self._update_select(instances, None, dict(c=c, b=b, h_l=h_l, h_u=h_u, x_l=x_l, x_u=x_u))
        if device_call((c, b, h_l, h_u, x_l, x_u)):
            keep = self._device_args(dict(c=c, b=b, h_l=h_l, h_u=h_u, x_l=x_l, x_u=x_u))
            return bool(check(self.L.pq_batch_update_mem(self.h, *[_ptr(a) for a in keep.values()], MEM_DEVICE), "pq_batch_update"))
        keep = [self._stack(c, self.batch, self.n), self._stack(b, self.batch, self.p), self._stack(h_l, self.batch, self.m), self._stack(h_u, self.batch, self.m),
                self._stack(x_l, self.batch, self.n), self._stack(x_u, self.batch, self.n)]
        return bool(check(self.L.pq_batch_update(self.h, *[_ptr(a) for a in keep]), "pq_batch_update"))

    def update_data(self, P_values=None, A_values=None, G_values=None, c=None, b=None, h_l=None, h_u=None, x_l=None, x_u=None, instances=None):
        """new matrix values ([batch, nnz] in the CSC order of the setup patterns) and / or vectors for every instance, None = unchanged:
        unscale -> assign -> (fresh) Ruiz equilibration on the device, solver.hpp:218-308.  torch CUDA tensors are read where they are (pq_batch_update_data_mem).
        instances: as at update() -- [len(instances), nnz] / [len(instances), len] stacks, the listed instances alone (pq_batch_update_data_select_mem)."""
        if instances is not None:
            return self._update_select(instances, dict(P_values=P_values, A_values=A_values, G_values=G_values), dict(c=c, b=b, h_l=h_l, h_u=h_u, x_l=x_l, x_u=x_u))
        if device_call((P_values, A_values, G_values, c, b, h_l, h_u, x_l, x_u)):
            keep = self._device_args(dict(P_values=P_values, A_values=A_values, G_values=G_values, c=c, b=b, h_l=h_l, h_u=h_u, x_l=x_l, x_u=x_u))
            return bool(check(self.L.pq_batch_update_data_mem(self.h, *[_ptr(a) for a in keep.values()], MEM_DEVICE), "pq_batch_update_data"))
        st = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        for a in (P_values, A_values, G_values):
            assert a is None or np.asarray(a).shape[0] == self.batch
        keep = [st(P_values), st(A_values), st(G_values), self._stack(c, self.batch, self.n), self._stack(b, self.batch, self.p), self._stack(h_l, self.batch, self.m),
                self._stack(h_u, self.batch, self.m), self._stack(x_l, self.batch, self.n), self._stack(x_u, self.batch, self.n)]
        return bool(check(self.L.pq_batch_update_data(self.h, *[_ptr(a) for a in keep]), "pq_batch_update_data"))

    def solve(self, instances=None):
        """returns the number of instances that ended SOLVED.
        instances: a list of distinct instances -- they alone are solved again, in place, with the settings as they stand (stragglers: raise settings.max_iter, then
        s.solve(np.flatnonzero(s.statuses() != SOLVED))); the others keep their results and infos; the count is of the listed ones (pq_batch_solve_select)."""
        if instances is not None:
            idx = self._instances(instances, unique=True)
            return check(self.L.pq_batch_solve_select(self.h, idx.ctypes.data, len(idx)), "pq_batch_solve_select")
        return check(self.L.pq_batch_solve(self.h), "pq_batch_solve")

    def info(self, i):
        ptr = self.L.pq_batch_info(self.h, i)
        if not ptr:
            raise IndexError(i)
        return ptr.contents

    def statuses(self):
        return np.array([self.info(i).status for i in range(self.batch)])

    def iterations(self):
        return np.array([self.info(i).iter for i in range(self.batch)])

    def result(self, name, device=False, instances=None):
        """[batch, len] numpy array, or (device=True) a torch tensor on the solver's GPU, copied there without leaving it.
        instances: a list of instances, repeats allowed -- [len(instances), len], row j of instance instances[j] (pq_batch_get_result_select_mem)"""
        k = VAR_NAMES.index(name)
        length = {"x": self.n, "y": self.p, "z_bl": self.n, "z_bu": self.n, "s_bl": self.n, "s_bu": self.n}.get(name, self.m)
        idx = None if instances is None else self._instances(instances, unique=False)
        rows = self.batch if idx is None else len(idx)
        if device:
            import torch
            out = torch.zeros((rows, length), dtype=torch.float64, device=f"cuda:{self.device}")
            sync_current_stream(self.device)
            if length and idx is None:
                check(self.L.pq_batch_get_result_mem(self.h, k, out.data_ptr(), MEM_DEVICE), "pq_batch_get_result")
            elif length:
                check(self.L.pq_batch_get_result_select_mem(self.h, idx.ctypes.data, rows, k, out.data_ptr(), MEM_DEVICE), "pq_batch_get_result_select_mem")
            return out
        out = np.zeros((rows, length))
        if length and idx is None:
            check(self.L.pq_batch_get_result(self.h, k, out.ctypes.data), "pq_batch_get_result")
        elif length:
            check(self.L.pq_batch_get_result_select_mem(self.h, idx.ctypes.data, rows, k, out.ctypes.data, MEM_HOST), "pq_batch_get_result_select_mem")
        return out

    def arena_row(self, i):
        """test hook: instance i's row of the device arena, arena_stride() doubles (pq_batch_arena_row)"""
        out = np.zeros(max(self.arena_stride(), 1))
        check(self.L.pq_batch_arena_row(self.h, int(i), out.ctypes.data), "pq_batch_arena_row")
        return out[:self.arena_stride()]

    def block_info(self):
        N = check(self.L.pq_batch_block_info(self.h, None, 0))
        out = np.zeros((N, 3), dtype=np.int32)
        check(self.L.pq_batch_block_info(self.h, out.ctypes.data, N))
        return out

    def kkt_factor(self, delta, x_reg, z_reg):
        """sparse_ldlt backend: KKTSolverBase::update_scalings_and_factor of every instance on its stored (scaled) data; delta [batch] (or a scalar),
        x_reg [batch, n], z_reg [batch, m].  Returns a bool array: False where a pivot was exactly zero (ldlt.hpp:163)"""
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(delta, dtype=np.float64), (self.batch,)))
        xr = np.ascontiguousarray(np.broadcast_to(np.asarray(x_reg, dtype=np.float64), (self.batch, self.n)))
        zr = np.ascontiguousarray(np.broadcast_to(np.asarray(z_reg, dtype=np.float64), (self.batch, self.m)))
        ok = np.zeros(max(self.batch, 1), dtype=np.int32)
        check(self.L.pq_batch_kkt_factor(self.h, _ptr(d), _ptr(xr), _ptr(zr), ok.ctypes.data), "pq_batch_kkt_factor")
        return ok[:self.batch] != 0

    def kkt_solve(self, rx, ry, rz):
        """sparse_ldlt backend: KKTSolverBase::solve of every instance with its last factorisation; [batch, len] right-hand sides -> (lx, ly, lz)"""
        rx, ry, rz = self._stack(rx, self.batch, self.n), self._stack(ry, self.batch, self.p), self._stack(rz, self.batch, self.m)
        lx, ly, lz = np.zeros((self.batch, self.n)), np.zeros((self.batch, self.p)), np.zeros((self.batch, self.m))
        check(self.L.pq_batch_kkt_solve(self.h, _ptr(rx), _ptr(ry), _ptr(rz), _ptr(lx), _ptr(ly), _ptr(lz)), "pq_batch_kkt_solve")
        return lx, ly, lz

    def ldlt_factor(self, i):
        """sparse_ldlt backend: the last factor of instance i as sparse/ldlt.hpp holds it -- the keys of SparseKKT.exact_factor()"""
        def item(what, dt, ln):
            a = np.zeros(max(int(ln), 1), dtype=dt)
            check(int(min(self.L.pq_batch_ldlt_factor(self.h, i, what, a.ctypes.data), 0)), "pq_batch_ldlt_factor")
            return a[:int(ln)]
        nnz = self.L.pq_batch_ldlt_factor(self.h, i, 0, None)
        check(int(min(nnz, 0)), "pq_batch_ldlt_factor")
        N = self.n + self.p + self.m
        out = {key: item(what, dt, ln) for key, what, dt, ln in (("L_cols", 1, np.int32, N + 1), ("L_ind", 2, np.int32, nnz), ("L_vals", 3, np.float64, nnz),
                                                                  ("D", 4, np.float64, N), ("D_inv", 5, np.float64, N), ("perm", 7, np.int32, N))}
        out["PKPt_val"] = item(6, np.float64, self.L.pq_batch_ldlt_factor(self.h, i, 6, None))
        return out

    def bound_lists(self, i):
        """the lists the kernels read for instance i now (the shared ones with bounds="shared"), from the device tables: dict(h_l_idx, h_u_idx, x_l_idx, x_u_idx --
        ascending int arrays --, dropped: bool [m], True on the rows of G without a finite bound, whose entries of G are zeroed)"""
        counts = np.zeros(4, dtype=np.int32)
        bufs = [np.zeros(max(ln, 1), dtype=np.int32) for ln in (self.m, self.m, self.n, self.n, self.m)]
        check(self.L.pq_batch_bound_lists(self.h, i, counts.ctypes.data, *[b.ctypes.data for b in bufs]), "pq_batch_bound_lists")
        out = {k: bufs[j][:counts[j]].copy() for j, k in enumerate(("h_l_idx", "h_u_idx", "x_l_idx", "x_u_idx"))}
        out["dropped"] = bufs[4][:self.m] != 0
        return out

    def profile(self, i):
        """device-clock seconds of instance i: dict(assemble, factor, chain_solve, kkt_solve, residuals, total); chain_solve = the backend's substitution"""
        out = np.zeros(8)
        check(self.L.pq_batch_get_profile(self.h, i, out.ctypes.data))
        return dict(zip(("assemble", "factor", "chain_solve", "kkt_solve", "residuals", "total"), out[:6]))

    def set_start_order(self, longest_first=True):
        """True (default): the instances that needed most iterations in the previous solve start first in the next launch; False: index order"""
        check(self.L.pq_batch_set_start_order(self.h, 1 if longest_first else 0), "pq_batch_set_start_order")

    def last_kernel_ms(self):
        ms, nt = C.c_double(), C.c_int()
        check(self.L.pq_batch_last_kernel_ms(self.h, C.byref(ms), C.byref(nt)))
        return ms.value, nt.value
