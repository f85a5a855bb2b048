"""Cases and the CPU reference for the non-batched KKTSystem shell (piqp_amd/csrc/kkt_system.hip), shared by tests/test_kktsys_shapes.py (CPU: the cases reach what
they claim on the oracle, the NumPy restatement IS the oracle's arithmetic bit for bit) and tests/test_kktsys_kernels_gpu.py (the kernels are the oracle bit for bit).

A problem is a shape (n, p, m), a bound pattern of the rows of G, a bound pattern of the variables and a storage (dense for the dense backends, sparse for the sparse
ones).  Every row of G has at least one finite bound (the reference asserts it).  x_b_scaling is uniform in [0.5, 2) and is written into the oracle's data through
od.vec("x_b_scaling"); the device handle is fed the oracle's own matrices, index lists and x_b_scaling (device_data).

A handle of a problem runs under one settings variant and takes STEPS in order: every (state, right-hand side) with refinement off and on.  cases() lists the
(problem, variant) pairs: at every shape each of the 16 (row pattern, box pattern) pairs occurs once, and the variants go round with them, so every variant meets
every shape at least twice.

The NumPy restatement (scalings, static_regularization, rhs_bars, recover, mul) restates the elementwise formulas of the reference's kkt_system.hpp:150-252, :310-366
and :392-425 with one IEEE operation per reference operation, in the reference's operand order; NumPy does not fuse.  Its inputs besides the state and the right-hand
side are what the backend produced: lhs.x, lhs.y, lhs_z and the mat-vec results."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from qp_gen import random_vars

NAMES = ("x", "y", "z_l", "z_u", "z_bl", "z_bu", "s_l", "s_u", "s_bl", "s_bu")
# each of n, p, m is the largest once; 63/64/65 and 255/256/257 occur; one of each length needs three blocks of 256
SHAPES = [(1, 0, 0), (1, 1, 1), (5, 3, 4), (64, 65, 63), (255, 0, 257), (256, 256, 256), (257, 300, 64), (64, 257, 0), (513, 2, 7), (7, 513, 2), (2, 7, 513)]
ROW_PATTERNS = ("mixed", "two-sided", "lower", "upper")
BOX_PATTERNS = ("mixed", "none", "both", "lower")
VARIANTS = {
    "default": {},
    "B": dict(iterative_refinement_static_regularization_eps=1e-4),
    "D": dict(iterative_refinement_static_regularization_eps=1e-4, iterative_refinement_eps_abs=0.0, iterative_refinement_eps_rel=0.0),
    "E": dict(iterative_refinement_static_regularization_eps=1e-4, iterative_refinement_max_iter=2),
    "rate": dict(iterative_refinement_static_regularization_eps=1e-4, iterative_refinement_min_improvement_rate=1e30),
    "zero-tol": dict(iterative_refinement_eps_abs=0.0, iterative_refinement_eps_rel=0.0),
    "no-iter": dict(iterative_refinement_max_iter=0),
}
# (state, right-hand side, refinement) of the steps one handle takes, in order
STEPS = [(st, rhs, ref) for st, rhs in (("early", "normal"), ("late", "normal"), ("early", "zero")) for ref in (0, 1)]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    """tests/test_dense_exact_gpu.py::same: equal shapes and equal bit patterns (NaN and the sign of zero cannot hide a difference)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def cases():
    """(shape, row pattern, box pattern, variant) of every handle"""
    out = []
    names = list(VARIANTS)
    for si, shape in enumerate(SHAPES):
        for j in range(16):
            out.append((shape, ROW_PATTERNS[j // 4], BOX_PATTERNS[j % 4], names[(j + si) % len(names)]))
    return out


# ------------------------------------------------------------------------------------------------------------------- problems
def bounds(n, m, rows, boxes, rng):
    row = rng.integers(0, 3, m) if rows == "mixed" else np.full(m, {"two-sided": 0, "lower": 1, "upper": 2}[rows])  # 0 both bounds, 1 lower only, 2 upper only
    var = rng.integers(0, 4, n) if boxes == "mixed" else np.full(n, {"both": 0, "lower": 1, "none": 3}[boxes])     # 0 both, 1 lower only, 2 upper only, 3 none
    h_l = np.where(row == 2, -np.inf, -rng.uniform(0.5, 2.0, m))
    h_u = np.where(row == 1, np.inf, rng.uniform(0.5, 2.0, m))
    x_l = np.where(var <= 1, -rng.uniform(0.5, 2.0, n), -np.inf)
    x_u = np.where((var == 0) | (var == 2), rng.uniform(0.5, 2.0, n), np.inf)
    return h_l, h_u, x_l, x_u


def seed_of(shape, rows, boxes, sparse):
    n, p, m = shape
    return [n, p, m, ROW_PATTERNS.index(rows), BOX_PATTERNS.index(boxes), int(sparse)]


def sparse_rows(k, n, w, rng, allowed):
    """k rows with min(w, len(allowed)) entries each in distinct columns out of `allowed`"""
    w = min(w, len(allowed))
    cols = np.stack([rng.choice(allowed, w, replace=False) for _ in range(k)]).ravel() if k else np.zeros(0, dtype=np.int64)
    return sp.csc_matrix((rng.standard_normal(k * w), (np.repeat(np.arange(k), w), cols)), shape=(k, n))


@functools.lru_cache(maxsize=None)
def problem(shape, rows, boxes, sparse):
    """the nine setup arguments as a dict, and x_b_scaling.  dense: P positive definite with entries of both signs, A and G dense.  sparse: a diagonally dominant P
    whose diagonal entry is structurally absent at every variable j = 1 mod 3 (kkt_system.hpp:430-453 leaves a zero there; such a variable has no entry in P at
    all, so P stays positive semidefinite, and none in A or G: its pivot is rho alone, which at rho = 1e-10 would cancel against everything coupled to it), with
    entries (j, j + 3) between the variables j = 0 mod 3; A and G rows of three entries."""
    n, p, m = shape
    rng = np.random.default_rng(seed_of(shape, rows, boxes, sparse))
    if sparse:
        d = rng.uniform(0.5, 1.5, n)
        keep = np.arange(n) % 3 != 1
        j = np.arange(0, max(n - 3, 0), 3)
        off = rng.uniform(-0.1, 0.1, j.size)
        P = sp.csc_matrix((np.concatenate([d[keep], off, off]), (np.concatenate([np.arange(n)[keep], j, j + 3]), np.concatenate([np.arange(n)[keep], j + 3, j]))), shape=(n, n))
        A, G = sparse_rows(p, n, 3, rng, np.flatnonzero(keep)), sparse_rows(m, n, 3, rng, np.flatnonzero(keep))
    else:
        k = min(n, 48)
        F = rng.standard_normal((n, k))
        P = F @ F.T / k + np.diag(rng.uniform(0.5, 1.5, n))
        P = np.triu(P) + np.triu(P, 1).T
        A, G = rng.standard_normal((p, n)), rng.standard_normal((m, n))
    h_l, h_u, x_l, x_u = bounds(n, m, rows, boxes, rng)
    q = dict(P=P, c=rng.standard_normal(n), A=A if p else None, b=rng.standard_normal(p) if p else None, G=G if m else None, h_l=h_l if m else None,
             h_u=h_u if m else None, x_l=x_l, x_u=x_u)
    return q, rng.uniform(0.5, 2.0, n)


def oracle_data(orc, q, xbs, sparse):
    od = (orc.Data.sparse if sparse else orc.Data.dense)(**q)
    od.vec("x_b_scaling")[:] = xbs
    return od


def lists(od):
    """what the elementwise formulas need of the data: sizes, finite-bound index lists, x_b_scaling, the diagonal of P (kkt_system.hpp:430-453)"""
    d = SimpleNamespace(n=od.n, p=od.p, m=od.m, h_l=od.idx("h_l"), h_u=od.idx("h_u"), x_l=od.idx("x_l"), x_u=od.idx("x_u"), xbs=od.vec("x_b_scaling").copy())
    if od.ptr.contents.is_sparse:
        d.P_diag = np.asarray(od.csc("P_utri").diagonal(), dtype=np.float64)
    else:
        d.P_diag = np.array(np.diagonal(od.mat("P_utri")), dtype=np.float64)
    d.used = dict(zip(NAMES, (d.n, d.p, d.m, d.m, len(d.x_l), len(d.x_u), d.m, d.m, len(d.x_l), len(d.x_u))))
    return d


def device_data(hip, od):
    """the oracle's own data as the device handle's input: matrices, index lists and x_b_scaling are the oracle's arrays"""
    n, p, m = od.n, od.p, od.m
    sparse = bool(od.ptr.contents.is_sparse)
    d = object.__new__(hip.SparseData if sparse else hip.Data)
    d.n, d.p, d.m = n, p, m
    if sparse:
        d.P_utri, d.AT, d.GT = od.csc("P_utri"), od.csc("AT"), od.csc("GT")
    else:
        d.P_utri, d.AT, d.GT = (np.asfortranarray(od.mat(nm).copy()) for nm in ("P_utri", "AT", "GT"))
    d.h_l_idx, d.h_u_idx, d.x_l_idx, d.x_u_idx = od.idx("h_l"), od.idx("h_u"), od.idx("x_l"), od.idx("x_u")
    d.n_h_l, d.n_h_u, d.n_x_l, d.n_x_u = od.counts()
    d.x_b_scaling = od.vec("x_b_scaling").copy()
    return d


# ------------------------------------------------------------------------------------------------------------------- states
def state(kind, shape, rng):
    """(rho, delta, vars): early -- the solver's initial regularisation and a mild interior point; late -- the regularisation floor and slacks / multipliers spread
    over twenty orders of magnitude"""
    n, p, m = shape
    if kind == "early":
        return 1e-6, 1e-4, random_vars(n, p, m, rng, positive=True)
    v = random_vars(n, p, m, rng)
    for nm in NAMES[2:]:
        v[nm] = np.exp(rng.uniform(-12, 8, v[nm].shape))
    return 1e-10, 1e-10, v


def rhs_of(kind, shape, rng):
    n, p, m = shape
    v = random_vars(n, p, m, rng)
    return {nm: np.zeros_like(a) for nm, a in v.items()} if kind == "zero" else v


def step_inputs(shape, rows, boxes, sparse, variant):
    """[(refine, rho, delta, vars, rhs, lhs_mul)] of the STEPS of one handle"""
    rng = np.random.default_rng(seed_of(shape, rows, boxes, sparse) + [list(VARIANTS).index(variant), 1])
    out = []
    for st, rk, refine in STEPS:
        rho, delta, v = state(st, shape, rng)
        out.append((refine, rho, delta, v, rhs_of(rk, shape, rng), random_vars(*shape, rng)))
    return out


def oracle_step(ko, d, refine, rho, delta, v, rhs, lhs_mul):
    """one step on the oracle: everything a device result is compared with"""
    R = SimpleNamespace(ok_f=ko.update_scalings_and_factor(refine, rho, delta, v), x_reg=ko.x_reg(), z_reg=ko.z_reg())
    if R.ok_f:
        before = ko.backend_solves()
        R.ok_s, R.lhs = ko.solve(rhs)
        R.steps, R.solves, R.exit = ko.last_refine_steps(), ko.backend_solves() - before, ko.last_refine_exit()
        R.refine_error, R.rhs_norm = ko.last_refine_error(), ko.last_rhs_norm()
        R.rxb, R.rzb, R.lhs_z = ko.rhs_x_bar(), ko.rhs_z_bar(), ko.lhs_z()
    R.mul = ko.mul(lhs_mul)
    return R


def condensed_residual(ko, d, S, x_reg, R, rhs):
    """(||rhs_bar - K_cond lhs||_inf, ||rhs_bar||_inf) of a solve, kkt_system.hpp:499-536, from the oracle backend's mat-vecs: what the refinement loop computes
    of its kept iterate, restated for the solves that ran without it"""
    b = ko.backend()
    x, y, z = R.lhs["x"], R.lhs["y"], R.lhs_z
    ex = b.eval_P_x(1.0, x)
    ex += x_reg * x
    ey, t = b.eval_A_xn_and_AT_xt(1.0, 1.0, x, y)
    ex += t
    ey -= S.delta * y
    ez, t = b.eval_G_xn_and_GT_xt(1.0, 1.0, x, z)
    ex += t
    ez -= S.z_reg * z
    nrm = lambda *vs: max([0.0] + [float(np.abs(a).max()) for a in vs if a.size])
    return nrm(R.rxb - ex, rhs["y"] - ey, R.rzb - ez), nrm(R.rxb, rhs["y"], R.rzb)


# ------------------------------------------------------------------------------------------------------------------- the NumPy restatement
def scalings(d, rho, delta, v):
    """kkt_system.hpp:150-193"""
    S = SimpleNamespace(rho=rho, delta=delta)
    nl, nu = len(d.x_l), len(d.x_u)
    S.s_l, S.s_u, S.s_bl, S.s_bu = v["s_l"].copy(), v["s_u"].copy(), v["s_bl"][:nl].copy(), v["s_bu"][:nu].copy()
    S.zi_l, S.zi_u, S.zi_bl, S.zi_bu = 1.0 / v["z_l"], 1.0 / v["z_u"], 1.0 / v["z_bl"][:nl], 1.0 / v["z_bu"][:nu]
    x = np.full(d.n, rho)
    x[d.x_l] += d.xbs[d.x_l] * d.xbs[d.x_l] / (S.zi_bl * S.s_bl + delta)
    x[d.x_u] += d.xbs[d.x_u] * d.xbs[d.x_u] / (S.zi_bu * S.s_bu + delta)
    z = np.zeros(d.m)
    z[d.h_l] += 1.0 / (S.zi_l[d.h_l] * S.s_l[d.h_l] + delta)
    z[d.h_u] += 1.0 / (S.zi_u[d.h_u] * S.s_u[d.h_u] + delta)
    S.x_reg, S.z_reg = x, 1.0 / z
    return S


def static_regularization(d, S, settings):
    """kkt_system.hpp:197-206: (reg, x_reg + reg); max_diag is a maximum, exact in any order"""
    max_diag = max([0.0] + [float(np.abs(a).max()) for a in (d.P_diag + S.x_reg, S.z_reg) if a.size])
    reg = settings.iterative_refinement_static_regularization_eps + settings.iterative_refinement_static_regularization_rel * max_diag
    return reg, S.x_reg + reg


def rhs_bars(d, S, rhs):
    """kkt_system.hpp:219-252: (rhs_x_bar, rhs_z_bar)"""
    nl, nu = len(d.x_l), len(d.x_u)
    hl, hu = d.h_l, d.h_u
    z = np.zeros(d.m)
    z[hl] -= 1.0 / (S.zi_l[hl] * S.s_l[hl] + S.delta) * (rhs["z_l"][hl] - S.zi_l[hl] * rhs["s_l"][hl])
    z[hu] += 1.0 / (S.zi_u[hu] * S.s_u[hu] + S.delta) * (rhs["z_u"][hu] - S.zi_u[hu] * rhs["s_u"][hu])
    z *= S.z_reg
    x = rhs["x"].copy()
    x[d.x_l] -= d.xbs[d.x_l] * (rhs["z_bl"][:nl] - S.zi_bl * rhs["s_bl"][:nl]) / (S.s_bl * S.zi_bl + S.delta)
    x[d.x_u] += d.xbs[d.x_u] * (rhs["z_bu"][:nu] - S.zi_bu * rhs["s_bu"][:nu]) / (S.s_bu * S.zi_bu + S.delta)
    return x, z


def recover(d, S, rhs, lhs_x, lhs_z):
    """kkt_system.hpp:310-366: the eight recovered vectors (box vectors up to n_x_l / n_x_u)"""
    nl, nu = len(d.x_l), len(d.x_u)
    l, u = np.zeros(d.m, bool), np.zeros(d.m, bool)
    l[d.h_l], u[d.h_u] = True, True
    both, lo, up = l & u, l & ~u, u & ~l
    with np.errstate(all="ignore"):
        rz_l_bar = rhs["z_l"] - S.zi_l * rhs["s_l"]
        W_l_inv = 1.0 / (S.zi_l * S.s_l + S.delta)
        rz_u_bar = rhs["z_u"] - S.zi_u * rhs["s_u"]
        W_u_inv = 1.0 / (S.zi_u * S.s_u + S.delta)
        r_sum = W_l_inv * W_u_inv * (rz_l_bar + rz_u_bar)
        z_l = np.where(both, -S.z_reg * (r_sum + W_l_inv * lhs_z), np.where(lo, -lhs_z, 0.0))
        z_u = np.where(both, -S.z_reg * (r_sum - W_u_inv * lhs_z), np.where(up, lhs_z, 0.0))
        s_l = np.where(l, S.zi_l * (rhs["s_l"] - S.s_l * z_l), 0.0)
        s_u = np.where(u, S.zi_u * (rhs["s_u"] - S.s_u * z_u), 0.0)
    z_bl = (-d.xbs[d.x_l] * lhs_x[d.x_l] - rhs["z_bl"][:nl] + S.zi_bl * rhs["s_bl"][:nl]) / (S.s_bl * S.zi_bl + S.delta)
    z_bu = (d.xbs[d.x_u] * lhs_x[d.x_u] - rhs["z_bu"][:nu] + S.zi_bu * rhs["s_bu"][:nu]) / (S.s_bu * S.zi_bu + S.delta)
    s_bl = S.zi_bl * (rhs["s_bl"][:nl] - S.s_bl * z_bl)
    s_bu = S.zi_bu * (rhs["s_bu"][:nu] - S.s_bu * z_bu)
    return dict(z_l=z_l, z_u=z_u, z_bl=z_bl, z_bu=z_bu, s_l=s_l, s_u=s_u, s_bl=s_bl, s_bu=s_bu)


def mul(d, S, lhs, Px, Ax, ATy, Gx, GTz):
    """kkt_system.hpp:392-425 from the mat-vec results P x, A x, A' y, G x and G' (z_u - z_l): all ten vectors (box vectors up to n_x_l / n_x_u)"""
    nl, nu = len(d.x_l), len(d.x_u)
    x = Px.copy()
    x += S.rho * lhs["x"]
    x += ATy
    y = Ax - S.delta * lhs["y"]
    z_l = -Gx
    x += GTz
    z_l += lhs["s_l"] - S.delta * lhs["z_l"]
    z_u = Gx + (lhs["s_u"] - S.delta * lhs["z_u"])
    s_l = S.s_l * lhs["z_l"] + lhs["s_l"] / S.zi_l
    s_u = S.s_u * lhs["z_u"] + lhs["s_u"] / S.zi_u
    x[d.x_l] -= d.xbs[d.x_l] * lhs["z_bl"][:nl]
    z_bl = -d.xbs[d.x_l] * lhs["x"][d.x_l] - S.delta * lhs["z_bl"][:nl] + lhs["s_bl"][:nl]
    s_bl = S.s_bl * lhs["z_bl"][:nl] + lhs["s_bl"][:nl] / S.zi_bl
    x[d.x_u] += d.xbs[d.x_u] * lhs["z_bu"][:nu]
    z_bu = d.xbs[d.x_u] * lhs["x"][d.x_u] - S.delta * lhs["z_bu"][:nu] + lhs["s_bu"][:nu]
    s_bu = S.s_bu * lhs["z_bu"][:nu] + lhs["s_bu"][:nu] / S.zi_bu
    return dict(x=x, y=y, z_l=z_l, z_u=z_u, z_bl=z_bl, z_bu=z_bu, s_l=s_l, s_u=s_u, s_bl=s_bl, s_bu=s_bu)


def mul_from_backend(b, d, S, lhs):
    """mul with the mat-vecs of a backend `b` (the oracle's or the device's: eval_P_x, eval_A_xn_and_AT_xt, eval_G_xn_and_GT_xt)"""
    h = lambda a: np.asarray(a, dtype=np.float64)
    Px = h(b.eval_P_x(1.0, lhs["x"]))
    Ax, ATy = (h(a) for a in b.eval_A_xn_and_AT_xt(1.0, 1.0, lhs["x"], lhs["y"]))
    Gx, GTz = (h(a) for a in b.eval_G_xn_and_GT_xt(1.0, 1.0, lhs["x"], lhs["z_u"] - lhs["z_l"]))
    return mul(d, S, lhs, Px, Ax, ATy, Gx, GTz)


def differing(d, got, ref, names=NAMES):
    """the names whose meaningful parts differ in a bit"""
    return [nm for nm in names if not same(np.asarray(got[nm])[:d.used[nm]], np.asarray(ref[nm])[:d.used[nm]])]


# ------------------------------------------------------------------------------------------------------------------- non-finite right-hand sides
POSITIONS = (0, 63, 64, 255, 256, 299)
SLOT_SHAPES = dict(x=(300, 50, 40), y=(50, 300, 40), z=(50, 40, 300))  # the slot's own length is the largest, and the only one the positions from 63 on exist in
BAD_VALUES = (np.nan, np.inf, -np.inf)


@functools.lru_cache(maxsize=None)
def decoupled_problem(slot):
    """a sparse problem in which a non-finite entry of the right-hand side stays where it is: P diagonal, A and G with at most one entry per row.  Of the slot's own
    index space the POSITIONS are cut off from everything else: slot x -- variables touched by neither A nor G (and without box bounds); slot y / z -- empty rows
    of A / G.  The other two matrices have an empty row of their own (row 1) and variable 1 is touched by neither wherever it can be."""
    n, p, m = SLOT_SHAPES[slot]
    rng = np.random.default_rng([n, p, m])
    free_vars = set(POSITIONS) if slot == "x" else {1}
    cols = np.array([j for j in range(n) if j not in free_vars])

    def rows(k, empty):
        r = np.array([i for i in range(k) if i not in empty])
        c = rng.choice(cols, r.size, replace=r.size > cols.size)
        return sp.csc_matrix((rng.uniform(0.5, 2.0, r.size) * rng.choice([-1.0, 1.0], r.size), (r, c)), shape=(k, n))
    A = rows(p, set(POSITIONS) if slot == "y" else {1})
    G = rows(m, set(POSITIONS) if slot == "z" else {1})
    P = sp.diags(rng.uniform(0.5, 2.0, n), format="csc")
    h_l, h_u, x_l, x_u = bounds(n, m, "mixed", "mixed", rng)
    for j in free_vars:
        x_l[j], x_u[j] = -np.inf, np.inf
    if slot == "z":  # (the spoiled entry goes into rhs.z_u: those rows have an upper bound, and a lower one)
        h_l[list(POSITIONS)], h_u[list(POSITIONS)] = -1.0, 1.0
    q = dict(P=P, c=rng.standard_normal(n), A=A, b=rng.standard_normal(p), G=G, h_l=h_l, h_u=h_u, x_l=x_l, x_u=x_u)
    return q, rng.uniform(0.5, 2.0, n)


def spoiled(rhs, slot, pos, value):
    """a copy of the right-hand side with `value` at `pos` of the slot: rhs.x, rhs.y or rhs.z_u"""
    bad = {nm: a.copy() for nm, a in rhs.items()}
    bad[dict(x="x", y="y", z="z_u")[slot]][pos] = value
    return bad


def nonfinite_cases():
    """(slot, position, value) of every spoiled solve"""
    return [(slot, pos, val) for slot in ("x", "y", "z") for pos in POSITIONS for val in BAD_VALUES]
