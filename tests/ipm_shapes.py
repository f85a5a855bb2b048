"""The shapes at which the interior-point loop (piqp_amd/csrc/device_ipm.hip, and the host loop of csrc/solver.cpp) is held to the CPU oracle, with the helpers
the two test modules share (tests/test_ipm_shapes.py on the CPU, tests/test_ipm_loop_gpu.py on the device).

Every reduction launch of the loop has G = min(512, ceil(max(n, p, m) / 256)) blocks of 256 threads, and the five index spaces n, p, m, nxl, nxu share that one
grid.  The regimes: one block (<= 256 elements); up to 64 blocks, where each lane of k_final_reduce folds one partial; more than 64 blocks (> 16 384 elements),
where a lane folds several; and the grid-stride loops wrapping (> 131 072 elements).  k_seq_dots has its own edges at lengths 0, 63, 64, 65.  Every count below
lands on or beside 0, 1, 64, 256, 16 384 or 131 072 at least once; L1 - L4 are the smallest sizes that cross the two upper edges."""
from collections import namedtuple

import numpy as np

from qp_gen import edge_qp

Shape = namedtuple("Shape", "name dense n p m nxl nxu seed")

SMALL = [
    Shape("s64", False, 64, 0, 0, 64, 0, 101),
    Shape("s65", False, 65, 1, 63, 0, 65, 102),
    Shape("s63", False, 63, 0, 64, 1, 63, 103),
    Shape("s256", False, 256, 64, 255, 255, 1, 104),
    Shape("s257", False, 257, 65, 257, 64, 256, 105),
    Shape("s255", False, 255, 63, 256, 65, 0, 106),
]
LARGE = [
    Shape("L1", False, 16461, 300, 16389, 16461, 16385, 201),
    Shape("L2", False, 131461, 300, 500, 131461, 131073, 202),
    Shape("L3", True, 48, 5, 16461, 20, 30, 203),
    Shape("L4", True, 48, 5, 131461, 20, 30, 204),
]
SHAPES = SMALL + LARGE
BY_NAME = {s.name: s for s in SHAPES}

VARS = ("x", "y", "z_l", "z_u", "z_bl", "z_bu", "s_l", "s_u", "s_bl", "s_bu")
# every pq_info field the oracle has too: the 22 doubles from rho to duality_gap_rel, then reg_limit and the three counters
INFO_DOUBLES = ("rho", "delta", "mu", "sigma", "primal_step", "dual_step", "primal_res", "primal_res_rel", "dual_res", "dual_res_rel", "primal_res_reg",
                "primal_res_reg_rel", "dual_res_reg", "dual_res_reg_rel", "primal_prox_inf", "dual_prox_inf", "prev_primal_res", "prev_dual_res", "primal_obj",
                "dual_obj", "duality_gap", "duality_gap_rel")
INFO_FIELDS = ("status", "iter") + INFO_DOUBLES + ("reg_limit", "factor_retires", "no_primal_update", "no_dual_update")
TRACE_COLS = ("iter", "primal_obj", "dual_obj", "duality_gap", "primal_res", "dual_res", "rho", "delta", "mu", "primal_step", "dual_step")
MU_FLOOR = 1e-6  # trace rows whose oracle mu is below this are decided by rounding in the reference itself
BIG = 1e30       # restore_dual's slack of an absent / inactive bound


def args_of(shape):
    return edge_qp(shape.n, shape.p, shape.m, shape.nxl, shape.nxu, shape.seed, dense=shape.dense)


def reversed_args(args, dense):
    """the same QP with variables and rows in reversed order: every summation and elimination order of a solve changes, the problem does not"""
    P, c, A, b, G, h_l, h_u, x_l, x_u = args
    rv = lambda v: None if v is None else np.ascontiguousarray(v[::-1])
    if dense:
        F = P + np.triu(P, 1).T
        Pr = np.triu(F[::-1, ::-1])
        rm = lambda M: None if M is None else np.ascontiguousarray(M[::-1, ::-1])
    else:
        import scipy.sparse as sp
        F = sp.csc_matrix(P + sp.triu(P, 1).T)
        Pr = sp.csc_matrix(sp.triu(F[::-1, :][:, ::-1]))
        rm = lambda M: None if M is None else sp.csc_matrix(M[::-1, :][:, ::-1])
    return (Pr, rv(c), rm(A), rv(b), rm(G), rv(h_l), rv(h_u), rv(x_l), rv(x_u))


def snapshot(solver, status):
    """status, the info fields, the per-iteration table and the ten result vectors of a solver (device or oracle) as plain values"""
    info = solver.info
    d = {k: getattr(info, k) for k in INFO_FIELDS}
    d["status"] = status
    return dict(info=d, trace=solver.trace(), result={k: np.array(v, dtype=np.float64, copy=True) for k, v in solver.result().items()})


def oracle_solve(orc, args, dense, kkt_solver=None, twice=False):
    """one oracle solve; twice: a second solve() of the same handle behind it, both returned"""
    so = orc.Solver()
    so.settings.kkt_solver = (0 if dense else orc.SPARSE_LDLT) if kkt_solver is None else kkt_solver
    so.enable_trace(256)
    assert so.setup(*args, sparse=not dense)
    first = snapshot(so, so.solve())
    if not twice:
        return first
    so.enable_trace(256)
    return first, snapshot(so, so.solve())


def unreverse(snap):
    out = dict(snap)
    out["result"] = {k: np.ascontiguousarray(v[::-1]) for k, v in snap["result"].items()}
    return out


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a == b) | ((a != a) & (b != b))


def first_difference(got, ref):
    """None if `got` is bitwise `ref` (NaN equal to NaN); otherwise a description of the first differing field and index"""
    for k in INFO_FIELDS:
        if not _same(got["info"][k], ref["info"][k]):
            return f"info.{k}: {got['info'][k]!r} != {ref['info'][k]!r}"
    tg, tr = got["trace"], ref["trace"]
    if tg.shape != tr.shape:
        return f"trace: {tg.shape[0]} rows != {tr.shape[0]}"
    bad = np.argwhere(~_same(tg, tr))
    if bad.size:
        r, c = bad[0]
        return f"trace row {r} column {c} ({TRACE_COLS[c]}): {tg[r, c]!r} != {tr[r, c]!r}"
    for k in VARS:
        g, r = got["result"][k], ref["result"][k]
        if g.shape != r.shape:
            return f"result.{k}: length {g.size} != {r.size}"
        bad = np.nonzero(~_same(g, r))[0]
        if bad.size:
            i = bad[0]
            return f"result.{k}[{i}] of {g.size}: {g[i]!r} != {r[i]!r} ({bad.size} entries differ, the last at {bad[-1]})"
    return None


def special(v):
    """the entries of a result vector that are rules, not arithmetic: exact zeros and the 1e30 of an absent / inactive bound"""
    return (v == 0.0) | (v == BIG)


def kept_rows(trace):
    return np.nonzero(trace[:, 8] >= MU_FLOOR)[0]


def reorder_differences(a, b):
    """the largest difference of two solves of the same problem: per trace column (relative, over the rows whose mu in `a` is >= MU_FLOOR) and per result vector
    (absolute, over the entries that are not exact 0.0 / 1e30); None where the two are not comparable (status, count, special entries differ)"""
    if a["info"]["status"] != b["info"]["status"] or a["info"]["iter"] != b["info"]["iter"] or a["trace"].shape != b["trace"].shape:
        return None
    rows = kept_rows(a["trace"])
    ta, tb = a["trace"][rows], b["trace"][rows]
    zero = ta == 0.0
    if not np.array_equal(zero, tb == 0.0):
        return None
    rel = np.where(zero, 0.0, np.abs(tb - ta) / np.where(zero, 1.0, np.abs(ta)))
    out = {"trace": rel.max(axis=0), "result": {}}
    for k in VARS:
        va, vb = a["result"][k], b["result"][k]
        sp = special(va)
        if not np.array_equal(va[sp], vb[sp]) or not np.array_equal(sp, special(vb)):
            return None
        out["result"][k] = float(np.abs(va - vb)[~sp].max()) if (~sp).any() else 0.0
    return out


RTOL = 1e-6    # the project's trajectory figure (tests/test_solver_gpu.py::test_iteration_parity_random_qp)
MARGIN = 30.0  # one and a half decades: another factorisation differs from the oracle's in more than order


def tolerances(diff, ref):
    """per trace column a relative tolerance, per result vector an absolute one: the larger of MARGIN x the reference's own reorder difference and RTOL (times the
    largest regular entry of the vector)"""
    tol = {"trace": np.maximum(MARGIN * diff["trace"], RTOL), "result": {}}
    for k in VARS:
        v = ref["result"][k]
        reg = np.abs(v[~special(v)])
        tol["result"][k] = max(MARGIN * diff["result"][k], RTOL * (float(reg.max()) if reg.size else 0.0))
    return tol


def summed_terms(shape, args):
    """the number of terms of the longest single sum behind the three sum-carrying trace columns"""
    h_l, h_u = args[5], args[6]
    free = None if h_l is None else ~np.isfinite(h_l) & ~np.isfinite(h_u)  # a row without a finite bound is kept with bounds -1, 1 (data.hpp disable_inf_constraints)
    nhl = 0 if h_l is None else int((np.isfinite(h_l) | free).sum())
    nhu = 0 if h_u is None else int((np.isfinite(h_u) | free).sum())
    return {"primal_obj": shape.n, "dual_obj": max(shape.n, shape.p, shape.m, shape.nxl, shape.nxu), "mu": nhl + nhu + shape.nxl + shape.nxu}
