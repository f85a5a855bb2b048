"""BatchDenseSolver: `batch` small dense QPs (n <= 128) through piqp::DenseSolver's setup() and solve(), behind pq_solver_batch_* (include/piqp_amd.h).  The
interior-point state of every instance lives on the GPU; the host clocks rounds of three launches (csrc/dense_solver_batch.hip).  Per instance status, iterations,
trace, results and info are bit for bit the CPU oracle's."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import VAR_NAMES, check
from .batch_kkt import KKT_BATCH_DENSE_MAX_N, _BatchHandle, select_list, var_shapes
from .batch_kktsys import BatchKKTSystem, _copy_settings
from .kkt import (COL_MAJOR, DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT, MEM_DEVICE, MEM_HOST, ROW_MAJOR, _is_torch, check_device_tensor, device_call,
                  sync_current_stream, to_device_args)

SCALED_ITEMS = ("P_utri", "AT", "GT", "c", "b", "h_l", "h_u", "x_l", "x_u", "x_b_scaling", "delta", "delta_b", "c_scale")  # PQ_SOLVER_BATCH_*
_NAMES = ("P", "c", "A", "b", "G", "h_l", "h_u", "x_l", "x_u")
BOUND_SETS = {"shared": 0, "per_instance": 1}  # PQ_BOUND_SETS_*


def stack_layout(t):
    """(tensor to pass, order) for a torch stack [batch, rows, cols]: contiguous is ROW_MAJOR, a stack of transposed views of contiguous matrices is COL_MAJOR,
    anything else is made contiguous first"""
    if t.is_contiguous():
        return t, ROW_MAJOR
    if t.transpose(1, 2).is_contiguous():
        return t, COL_MAJOR
    return t.contiguous(), ROW_MAJOR


class BatchDenseSolver(_BatchHandle):
    """BatchDenseSolver(device=0, kkt_solver=DENSE_CHOLESKY, bounds="shared")

    s.settings: the pq_settings shared by the batch.  s.setup(P, c, A=None, b=None, G=None, h_l=None, h_u=None, x_l=None, x_u=None): P [batch, n, n], A [batch, p, n],
    G [batch, m, n], vectors [batch, len]; NumPy arrays, or torch CUDA float64 tensors (with any CUDA tensor among the arguments the data stays on the GPU and NumPy
    arguments beside it are moved there).  bounds="shared" (the default): the instances share the set of finite bounds, a checked promise; bounds="per_instance": every
    instance has the finite-bound lists DenseSolver would hold for its own vectors, at setup and after every update (-/+ inf switches a bound off).  s.solve() returns the number of instances that ended SOLVED.
    s.update(P=None, c=None, A=None, b=None, G=None, h_l=None, h_u=None, x_l=None, x_u=None): DenseSolver::update on the device, without a new setup; any subset of
    the arguments, under the rules of setup; with shared bounds the set of finite bounds must stay the setup's (RuntimeError otherwise, the handle is as it was).
    s.clone(instances=None): a second solver in the state of this one, without a new setup -- whole, or instance j of the clone being instance instances[j] of this
    one (repeats allowed, any length >= 1): settings, scaled data, stored scalings, bound sets, statuses, results and traces go along, so update() on the clone gives
    each copy its scenario and a clone of the instances that did not end SOLVED can be solved again with other settings.
    IN PLACE ON A LIST OF INSTANCES (pq_solver_batch_*_select): s.solve(instances=...), s.update(..., instances=...) and s.result(name, instances=...) act on the listed
    instances of this solver -- no second handle, no gather of its buffers.  instances: anything np.asarray makes a one-dimensional, non-empty list of integers of;
    for solve and update the entries are distinct.  update takes arrays [len(instances), ...], row j for instance instances[j], NumPy or torch CUDA tensors under
    the rules of setup; the listed instances end bit for bit where the whole-batch call given the same rows would leave them, and nothing of any other instance is
    written.  solve runs the listed instances again from the start with the settings as they stand (stragglers: raise settings.max_iter, then
    s.solve(instances=np.flatnonzero(s.statuses() != SOLVED))) and returns how many of them ended SOLVED; the others keep results, info and trace.  result gives
    [len(instances), len], repeats allowed.  A fleet of which a fraction gets new measurements: s.update(c=c_new, b=b_new, instances=ids); s.solve(instances=ids)."""
    _destroy = "pq_solver_batch_destroy"

    def __init__(self, device=0, kkt_solver=DENSE_CHOLESKY, bounds="shared"):
        if kkt_solver not in (DENSE_CHOLESKY, DENSE_LDLT_NO_PIVOT):
            raise ValueError(f"kkt_solver {kkt_solver}: DENSE_CHOLESKY or DENSE_LDLT_NO_PIVOT")
        if bounds not in BOUND_SETS:
            raise ValueError(f"bounds {bounds!r}: 'shared' or 'per_instance'")
        self.L = _lib.load()
        self.device = int(device)
        self.kkt_solver = int(kkt_solver)
        self.batch = self.n = self.p = self.m = None
        h = C.c_void_p()
        check(self.L.pq_solver_batch_create(C.byref(h), self.device), "pq_solver_batch_create")
        self.h = h
        self.settings.kkt_solver = self.kkt_solver
        self.bounds = bounds
        if bounds != "shared":
            check(self.L.pq_solver_batch_set_bound_sets(self.h, BOUND_SETS[bounds]), "pq_solver_batch_set_bound_sets")

    @property
    def settings(self):
        return self.L.pq_solver_batch_settings(self.h).contents

    def clone(self, instances=None):
        h = C.c_void_p()
        if instances is None:
            check(self.L.pq_solver_batch_clone(self.h, C.byref(h)), "pq_solver_batch_clone")
            batch = self.batch
        else:
            idx = select_list(instances)
            check(self.L.pq_solver_batch_clone_select(self.h, idx.ctypes.data, len(idx), C.byref(h)), "pq_solver_batch_clone_select")
            batch = len(idx)
        c = type(self).__new__(type(self))
        c.L, c.device, c.kkt_solver, c.bounds, c.h = self.L, self.device, self.kkt_solver, self.bounds, h
        c.batch, c.n, c.p, c.m = batch, self.n, self.p, self.m
        return c

    # ---- argument handling: no library call in here
    @staticmethod
    def shapes(P, A, G):
        """(batch, n, p, m) and the expected shape of every argument"""
        shape = tuple(P.shape)
        if len(shape) != 3 or shape[1] != shape[2]:
            raise ValueError(f"P: shape {shape}, expected [batch, n, n]")
        b, n = int(shape[0]), int(shape[1])
        if n > KKT_BATCH_DENSE_MAX_N:
            raise ValueError(f"n = {n}: the batched dense solver takes n <= {KKT_BATCH_DENSE_MAX_N}")
        for name, M in (("A", A), ("G", G)):
            if M is not None and (len(M.shape) != 3 or M.shape[0] != b or M.shape[2] != n):
                raise ValueError(f"{name}: shape {tuple(M.shape)}, expected [{b}, rows, {n}]")
        p = 0 if A is None else int(A.shape[1])
        m = 0 if G is None else int(G.shape[1])
        return (b, n, p, m), dict(P=(b, n, n), c=(b, n), A=(b, p, n), b=(b, p), G=(b, m, n), h_l=(b, m), h_u=(b, m), x_l=(b, n), x_u=(b, n))

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

    def _prepare(self, args, dims=None):
        """(dims, mem, order, the arrays to pass in the order of _NAMES); raises before any library call.  dims: None for a setup, which takes them from P, A and G;
        the (batch, n, p, m) of the setup for an update, where every argument is optional -- for an update of a list of instances the leading one is the length of
        the list"""
        a = dict(zip(_NAMES, args))
        if dims is None:
            if a["P"] is None or a["c"] is None:
                raise ValueError("P and c must be given")
            dims, shapes = self.shapes(a["P"], a["A"], a["G"])
            if a["A"] is None and a["b"] is not None or a["G"] is None and (a["h_l"] is not None or a["h_u"] is not None):
                raise ValueError("b without A, or h_l / h_u without G")
        else:
            b, n, p, m = dims
            shapes = dict(P=(b, n, n), c=(b, n), A=(b, p, n), b=(b, p), G=(b, m, n), h_l=(b, m), h_u=(b, m), x_l=(b, n), x_u=(b, n))
            for k in ("A", "b") if p == 0 else ():
                if a[k] is not None:
                    raise ValueError(f"{k} given, the setup has p = 0")
            for k in ("G", "h_l", "h_u") if m == 0 else ():
                if a[k] is not None:
                    raise ValueError(f"{k} given, the setup has m = 0")
        if device_call(args):
            mats = {}
            for k in ("P", "A", "G"):
                if a[k] is not None and _is_torch(a[k]):
                    mats[k] = stack_layout(check_device_tensor(k, a[k], shapes[k], self.device))
                    a[k] = None
            keep, _ = to_device_args(a, shapes, self.device)
            orders = {v[1] for v in mats.values()}
            order = COL_MAJOR if orders == {COL_MAJOR} and all(keep[k] is None for k in ("P", "A", "G")) else ROW_MAJOR
            for k, (t, o) in mats.items():
                keep[k] = t if o == order else t.contiguous()
            return dims, MEM_DEVICE, order, [keep[k] for k in _NAMES]
        out = []
        for k in _NAMES:
            v = a[k]
            if v is not None:
                v = np.ascontiguousarray(v, dtype=np.float64)
                if v.shape != shapes[k]:
                    raise ValueError(f"{k}: shape {v.shape}, expected {shapes[k]}")
            out.append(v)
        return dims, MEM_HOST, ROW_MAJOR, out

    # ---- the DenseSolver surface
    def enable_trace(self, max_rows=512):
        """keeps the per-iteration table of every instance in device memory; call before setup()"""
        check(self.L.pq_solver_batch_set_trace(self.h, int(max_rows)), "pq_solver_batch_set_trace")

    def setup(self, P, c, A=None, b=None, G=None, h_l=None, h_u=None, x_l=None, x_u=None):
        dims, mem, order, arrs = self._prepare((P, c, A, b, G, h_l, h_u, x_l, x_u))
        if mem == MEM_DEVICE:
            sync_current_stream(self.device)
        check(self.L.pq_solver_batch_setup_dense(self.h, *dims, *[self._p(v) for v in arrs], mem, order), "pq_solver_batch_setup_dense")
        self.batch, self.n, self.p, self.m = dims

    def update(self, P=None, c=None, A=None, b=None, G=None, h_l=None, h_u=None, x_l=None, x_u=None, instances=None):
        """instances: a list of distinct instances -- the arrays are [len(instances), ...], row j for instance instances[j]; those instances alone are updated, in
        place (pq_solver_batch_update_dense_select)"""
        if self.batch is None:
            raise RuntimeError("update before setup")
        idx = None if instances is None else self._instances(instances, unique=True)
        rows = self.batch if idx is None else len(idx)
        _, mem, order, arrs = self._prepare((P, c, A, b, G, h_l, h_u, x_l, x_u), (rows, self.n, self.p, self.m))
        if mem == MEM_DEVICE:
            sync_current_stream(self.device)
        ptrs = [self._p(v) for v in arrs]
        if idx is not None:
            return check(self.L.pq_solver_batch_update_dense_select(self.h, idx.ctypes.data, rows, *ptrs, mem, order), "pq_solver_batch_update_dense_select") == 1
        return check(self.L.pq_solver_batch_update_dense(self.h, *ptrs, mem, order), "pq_solver_batch_update_dense") == 1

    def clone_ms(self):
        """of the clone() that made this solver: dict(wall_ms, device_ms); zeros on a solver that is no clone"""
        o = np.zeros(2)
        check(self.L.pq_solver_batch_clone_ms(self.h, o.ctypes.data), "pq_solver_batch_clone_ms")
        return dict(wall_ms=float(o[0]), device_ms=float(o[1]))

    def last_update_ms(self):
        """of the last update: dict(wall_ms, device_ms)"""
        o = np.zeros(2)
        check(self.L.pq_solver_batch_last_update_ms(self.h, o.ctypes.data), "pq_solver_batch_last_update_ms")
        return dict(wall_ms=float(o[0]), device_ms=float(o[1]))

    def solve(self, instances=None):
        """returns the number of instances that ended SOLVED.  instances: a list of distinct instances -- they alone are solved again, in place, with the settings as
        they stand; the count is of the listed ones (pq_solver_batch_solve_select)"""
        if instances is not None:
            idx = self._instances(instances, unique=True)
            return check(self.L.pq_solver_batch_solve_select(self.h, idx.ctypes.data, len(idx)), "pq_solver_batch_solve_select")
        return check(self.L.pq_solver_batch_solve(self.h), "pq_solver_batch_solve")

    def info(self, i):
        ptr = self.L.pq_solver_batch_info(self.h, int(i))
        if not ptr:
            raise IndexError(self.L.pq_last_error_string().decode())
        return ptr.contents

    def statuses(self):
        return np.array([self.info(i).status for i in range(self.batch)], dtype=np.int32)

    def iterations(self):
        return np.array([self.info(i).iter for i in range(self.batch)], dtype=np.int32)

    def result(self, name, device=False, instances=None):
        """field `name` of Variables of all instances, [batch, len]: a NumPy array, or with device=True a torch CUDA tensor (no copy across the link).
        instances: a list of instances, repeats allowed -- [len(instances), len], row j of instance instances[j] (pq_solver_batch_get_result_select_mem)"""
        field = VAR_NAMES.index(name)
        idx = None if instances is None else self._instances(instances, unique=False)
        shape = var_shapes(self.batch if idx is None else len(idx), self.n, self.p, self.m)[name]
        if device:
            import torch
            out = torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.device}")
            sync_current_stream(self.device)
            ptr, mem = out.data_ptr(), MEM_DEVICE
        else:
            out = np.zeros(shape)
            ptr, mem = out.ctypes.data, MEM_HOST
        if idx is None:
            check(self.L.pq_solver_batch_get_result_mem(self.h, field, ptr, mem), "pq_solver_batch_get_result_mem")
        else:  # (an empty torch tensor has no address to give: a field of length 0 is checked like any other and nothing is written, so any address stands for it)
            check(self.L.pq_solver_batch_get_result_select_mem(self.h, idx.ctypes.data, len(idx), field, ptr or idx.ctypes.data, mem), "pq_solver_batch_get_result_select_mem")
        return out

    def trace(self, i):
        rows = C.c_int(0)
        check(self.L.pq_solver_batch_get_trace(self.h, int(i), None, C.byref(rows)), "pq_solver_batch_get_trace")
        out = np.zeros((rows.value, 11))
        if rows.value:
            check(self.L.pq_solver_batch_get_trace(self.h, int(i), out.ctypes.data, C.byref(rows)), "pq_solver_batch_get_trace")
        return out

    def last_ms(self):
        """of the last solve: dict(wall_ms, device_ms, rounds, launches, factor_ms, solve_ms)"""
        o = np.zeros(6)
        check(self.L.pq_solver_batch_last_ms(self.h, o.ctypes.data), "pq_solver_batch_last_ms")
        return dict(wall_ms=float(o[0]), device_ms=float(o[1]), rounds=int(o[2]), launches=int(o[3]), factor_ms=float(o[4]), solve_ms=float(o[5]))

    def max_rounds(self):
        """the bound on the rounds of a solve with the present settings"""
        return (self.settings.max_iter + 1) * (self.settings.max_factor_retires + 4)

    # ---- test hooks
    def scaled_data(self, i, name):
        n, p, m = self.n, self.p, self.m
        what = SCALED_ITEMS.index(name)
        shape = ((n, n), (n, p), (n, m), (n,), (p,), (m,), (m,), (n,), (n,), (n,), (n + p + m,), (n,), (1,))[what]
        out = np.zeros(shape, order="F")
        check(self.L.pq_solver_batch_scaled_data(self.h, int(i), what, out.ctypes.data), "pq_solver_batch_scaled_data")
        return out

    def kktsys(self):
        """the BatchKKTSystem this solver owns (borrowed: it lives until the next setup() or the end of this object).  The solver keeps the bound lists to itself,
        so the borrowed system has lists = None: its read-only hooks work, its calls that take variables raise RuntimeError"""
        h = self.L.pq_solver_batch_kktsys(self.h)
        if not h:
            raise RuntimeError(self.L.pq_last_error_string().decode())
        return BatchKKTSystem._adopt(h, self.device, self.kkt_solver, owner=self, lists=None, settings=_copy_settings(self.settings))
