"""The problems at which the chain engine of the `sparse_multistage` backend (csrc/multistage_kkt.hip, csrc/multistage_device.hpp) is held to a high-precision
reference (tests/test_multistage_branches_gpu.py), each the smallest found that reaches one branch of MultistageKKT::plan_lds(), with the plan that branch needs.
tests/test_multistage_shapes.py re-derives every plan on the CPU from the oracle's block structure, so a changed generator or a changed structure heuristic names
the shapes that no longer reach their branch instead of the GPU test quietly testing less.  Nothing in this module needs a GPU.

plan_lds() in doubles (LDS_LIMIT_BYTES = 159 KiB = 20352 doubles, ASM_CHUNK = 4096 front entries per assembly workgroup); h_b = w_b + off_b + arrow is the order of
stage b's front, w_b the columns it eliminates, u_b = h_b - w_b the order of the update matrix it carries on:
  factor_in_lds  max_h^2 + max_u^2 + max_w^2 <= 20352                      k_ms_factor<true>: front, carried update and inverse in LDS
  li_in_lds      factor_in_lds or max_w^2 <= 20352 (w <= 142)              k_ms_factor<false>: front factored in place in HBM, the inverse staged in LDS or not
  solve_in_lds   2 max(1, max_h) + max_b (h_b w_b + w_b^2) <= 20352        k_ms_solve<true> / <false>
  asm_chunks     max(1, ceil(max_h^2 / 4096))                              grid.y of k_ms_assemble and k_ms_gram
"""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from qp_gen import mpc_chain

U = 2.0 ** -53
LDS_DOUBLES = 159 * 1024 // 8
ASM_CHUNK = 4096
PLAN_KEYS = ("factor_in_lds", "li_in_lds", "solve_in_lds", "asm_chunks", "max_h", "max_w", "factor_lds_bytes")

# name, (nx, nu, T) and the keyword arguments of branch_qp, (n, p, m), arrow width, the pinned plan in the order of PLAN_KEYS, and what the row is for
Shape = namedtuple("Shape", "name chain kw dims arrow plan branch")


def gamma(k):
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------------------------------------------------------------------------- problems
def branch_qp(nx, nu, T, seed=7, g_seed=3, eq=True, ineq=True, arrow=True, tail=0):
    """qp_gen.mpc_chain(nx, nu, T, seed) -- dense dynamics blocks, so dense fronts: a sparse L would hide a wrong index -- plus general inequality rows, so that the
    X_G W X_G^T term of the assembly and the G half of fold / recover are live in every chunk: per stage (nx + nu) // 2 rows with three entries at random positions
    inside that stage's variables, and (arrow) one last row with 0.5 on variable 0 and 1.0 on the last three variables, which couples the first stage to the
    last and makes the structure heuristic open an arrow.  Bounds -1 / +1.
    eq = False: no equality rows; the dynamics couple the stages through P instead, P + A^T A (block tridiagonal, positive definite), and there is no Gram term.
    tail = k: k more variables behind x_T with a dense positive definite block of P of their own and nothing that couples them to the chain -- a small last stage, next
    to which the structure heuristic finds no arrow worth its cost: arrow width 0 (an arrow row is then left out by the caller).
    Returns the nine setup arguments."""
    P, c, A, b, _, _, _, x_l, x_u = mpc_chain(nx, nu, T, seed)
    n, nz = P.shape[0], nx + nu
    G = h_l = h_u = None
    if ineq:
        rng = np.random.default_rng(g_seed)
        per = nz // 2
        rows, cols, vals = [], [], []
        for t in range(T):
            for r in range(per):
                rows += [t * per + r] * 3
                cols += list(t * nz + rng.choice(nz, 3, replace=False))
                vals += list(rng.standard_normal(3))
        m = T * per
        if arrow:
            rows += [m] * 4
            cols += [0, n - 3, n - 2, n - 1]
            vals += [0.5, 1.0, 1.0, 1.0]
            m += 1
        G = sp.csc_matrix((vals, (rows, cols)), shape=(m, n))
        h_l, h_u = -np.ones(m), np.ones(m)
    if not eq:
        P = sp.csc_matrix(sp.triu(P + A.T @ A))
        A = b = None
    if tail:
        rng = np.random.default_rng([g_seed, tail])
        M = rng.standard_normal((tail, tail))
        P = sp.block_diag([P, np.triu(M @ M.T / tail + np.eye(tail))], format="csc")
        c, x_l, x_u = np.concatenate([c, rng.standard_normal(tail)]), np.concatenate([x_l, -np.ones(tail)]), np.concatenate([x_u, np.ones(tail)])
        A = None if A is None else sp.hstack([A, sp.csc_matrix((A.shape[0], tail))], format="csc")
        G = None if G is None else sp.hstack([G, sp.csc_matrix((G.shape[0], tail))], format="csc")
    return (sp.csc_matrix(P), c, A, b, G, h_l, h_u, x_l, x_u)


def args_of(shape):
    return branch_qp(*shape.chain, **shape.kw)


def dense3(args):
    """(Pf, A, G) as dense arrays: the full symmetric P, and 0 x n arrays for an absent A or G"""
    P, A, G = args[0], args[2], args[4]
    n = P.shape[0]
    Pu = np.triu(P.toarray())
    return Pu + np.triu(Pu, 1).T, (A.toarray() if A is not None else np.zeros((0, n))), (G.toarray() if G is not None else np.zeros((0, n)))


def new_values(args, seed=5):
    """the same patterns with other values (the recipe of test_multistage_gpu.py::test_update_data_matches_fresh): every stored value times 1 + 0.1 N(0, 1), then P's
    diagonal raised, if need be, until the smallest eigenvalue of P is 0.01"""
    rng = np.random.default_rng(seed)
    out = list(args)
    for i in (0, 2, 4):
        if args[i] is not None:
            M = sp.csc_matrix(args[i], copy=True)
            M.sort_indices()
            M.data = M.data * (1.0 + 0.1 * rng.standard_normal(M.data.size))
            out[i] = M
    Pd = np.triu(out[0].toarray())
    mn = np.linalg.eigvalsh(Pd + np.triu(Pd, 1).T).min()
    if mn < 0.01:
        nnz = out[0].nnz
        out[0] = sp.csc_matrix(out[0] + sp.eye(Pd.shape[0]) * (0.01 - mn))
        assert out[0].nnz == nnz
    return tuple(out)


REGIMES = ("well", "ipm")


def scalings(regime, n, m, seed=5):
    """(delta, x_reg, z_reg).  well: the regime of the reference's FactorizeSolveSQP test; ipm: what a late interior-point iteration hands the backend"""
    rng = np.random.default_rng([seed, REGIMES.index(regime)])
    if regime == "well":
        return 1.2, rng.uniform(0.5, 2.0, n), rng.uniform(0.1, 3.0, m)
    return 1e-4, rng.uniform(1e-6, 1e-2, n), 10.0 ** rng.uniform(-4.0, 2.0, m)


def right_hand_sides(n, p, m):
    """four right-hand sides (rx, ry, rz) at the scales of factor_bounds.right_hand_sides; the fifth solve repeats the first"""
    rng = np.random.default_rng([n + p + m, 11])
    return [tuple(rng.standard_normal(k) * s for k in (n, p, m)) for s in (1.0, 3.0, 0.01, 1.0)]


# ---------------------------------------------------------------------------------------------------------------------------------- plan
def plan_of(block_info):
    """MultistageKKT::plan_lds() restated on the rows (start, diag_size, off_diag_size) of block_info (last row: the arrow corner); a dict over PLAN_KEYS"""
    bi = np.asarray(block_info, dtype=np.int64)
    arrow = int(bi[-1, 1])
    w = bi[:, 1].copy()
    h = w + bi[:, 2] + arrow
    h[-1] = arrow
    max_h, max_w, max_u = int(h.max()), int(w.max()), int((h - w).max())
    max_pan = int((h * w + w * w).max())
    factor_in_lds = max_h * max_h + max_u * max_u + max_w * max_w <= LDS_DOUBLES
    li_in_lds = factor_in_lds or max_w * max_w <= LDS_DOUBLES
    lds = 8 * (max_h * max_h + max_u * max_u + max_w * max_w) if factor_in_lds else (8 * max_w * max_w if li_in_lds else 0)
    return dict(factor_in_lds=int(factor_in_lds), li_in_lds=int(li_in_lds), solve_in_lds=int(2 * max(1, max_h) + max_pan <= LDS_DOUBLES),
                asm_chunks=max(1, -(-max_h * max_h // ASM_CHUNK)), max_h=max_h, max_w=max_w, factor_lds_bytes=lds)


def stages_of(block_info):
    return len(block_info) - 1


# ---------------------------------------------------------------------------------------------------------------------------------- reference
def kkt_matrix(Pf, A, G, x_reg, delta, z_reg):
    """the 3 x 3 block matrix the backend solves with: [P + diag(x_reg), A^T, G^T; A, -delta I, 0; G, 0, -diag(z_reg)]"""
    n, p, m = Pf.shape[0], A.shape[0], G.shape[0]
    K = np.zeros((n + p + m, n + p + m))
    K[:n, :n] = Pf
    K[np.arange(n), np.arange(n)] += x_reg
    K[:n, n:n + p] = A.T; K[n:n + p, :n] = A
    K[:n, n + p:] = G.T; K[n + p:, :n] = G
    K[np.arange(n, n + p), np.arange(n, n + p)] = -delta
    K[np.arange(n + p, n + p + m), np.arange(n + p, n + p + m)] = -z_reg
    return K


def reference_solve(Pf, A, G, x_reg, delta, z_reg, rhs, steps=4):
    """rhs: (n + p + m) or (n + p + m) x k.  The full KKT matrix solved in fp64 (LAPACK LU with partial pivoting), then `steps` steps of iterative refinement with
    the residual formed, and the solution accumulated, in numpy.longdouble.  Returns (solution in fp64, largest |residual| per right-hand side of the
    longdouble solution, in longdouble)."""
    from scipy.linalg import lu_factor, lu_solve
    K = kkt_matrix(Pf, A, G, x_reg, delta, z_reg)
    lu = lu_factor(K)
    rows, cols = np.nonzero(K)  # (row-major order: rows ascending)
    vals = K[rows, cols].astype(np.longdouble)
    first = np.searchsorted(rows, np.arange(K.shape[0]))  # every row holds its diagonal entry, so none is empty
    bl = np.asarray(rhs, dtype=np.longdouble)
    one = bl.ndim == 1
    bl = bl.reshape(K.shape[0], -1)

    def residual(x):  # b - K x, every product and sum in longdouble
        return bl - np.add.reduceat(vals[:, None] * x[cols], first, axis=0)
    x = lu_solve(lu, bl.astype(np.float64)).astype(np.longdouble)
    for _ in range(steps):
        x = x + lu_solve(lu, residual(x).astype(np.float64)).astype(np.longdouble)
    res = np.abs(residual(x)).max(axis=0)
    x = x.astype(np.float64)
    return (x[:, 0], res[0]) if one else (x, res)


def split(v, n, p, m):
    return v[:n], v[n:n + p], v[n + p:n + p + m]


def field_errors(sol, ref):
    """err(v) = max |v - v_ref| / max |v_ref| per field (x, y, z); 0 for an empty field"""
    return [0.0 if r.size == 0 else float(np.abs(np.asarray(s) - r).max() / np.abs(r).max()) for s, r in zip(sol, ref)]


def condensed_matrix(Pf, A, G, x_reg, delta, z_reg):
    """P + diag(x_reg) + A^T A / delta + G^T diag(1 / z_reg) G: what the chain factors"""
    K = Pf + np.diag(x_reg) + A.T @ A / delta
    return K + (G.T * (1.0 / z_reg)) @ G if G.shape[0] else K


def block_conditions(Kc, block_info):
    """2-norm condition numbers of the diagonal blocks, by the block layout, of the Cholesky factor of Kc: the blocks the device inverts explicitly"""
    L = np.linalg.cholesky(Kc)
    return [float(np.linalg.cond(L[s:s + w, s:s + w])) for s, w, _ in np.asarray(block_info) if w > 0]


# ---------------------------------------------------------------------------------------------------------------------------------- the table
def _plan(*v):
    return dict(zip(PLAN_KEYS, v))


# in the order of ascending novelty: what the suite already reaches first, the all-HBM row last
SHAPES = [
    Shape("lds-lds-1chunk", (16, 8, 4), {}, (112, 64, 49), 4, _plan(1, 1, 1, 1, 44, 36, 29056),
          "what the suite's fixtures already reach (fronts <= 64): everything in LDS, one assembly chunk"),
    Shape("lds-lds", (32, 32, 5), {}, (352, 160, 161), 8, _plan(1, 1, 1, 3, 104, 88, 161280),
          "factor and solve in LDS with 3 assembly / Gram chunks (blockIdx.y > 0); 161280 of the 162816 bytes of LDS"),
    Shape("hbm-li-lds", (40, 24, 3), {}, (232, 120, 97), 12, _plan(0, 1, 1, 4, 116, 92, 67712),
          "k_ms_factor<false>: fronts factored in place in HBM, update carried with ldu = ld, inverse staged in LDS; solve still in LDS"),
    Shape("hbm-li-lds-m0", (40, 24, 3), dict(ineq=False), (232, 120, 0), 8, _plan(0, 1, 1, 4, 112, 96, 73728),
          "the same without inequality rows: no k_ms_reciprocal, no X_G W X_G^T term, empty z"),
    Shape("hbm-li-lds-p0", (40, 24, 3), dict(eq=False), (232, 0, 97), 12, _plan(0, 1, 1, 4, 116, 92, 67712),
          "the same without equality rows: stages coupled through a block-tridiagonal P, the Gram term all zero, empty y"),
    Shape("hbm-li-hbm-arrow0", (40, 24, 3), dict(arrow=False, tail=24), (256, 120, 96), 0, _plan(0, 1, 0, 3, 104, 104, 86528),
          "arrow width 0 (the chain loops leave at the empty corner block), a last stage that receives no update; k_ms_solve<false>"),
    Shape("hbm-li-hbm", (45, 20, 3), {}, (240, 135, 97), 12, _plan(0, 1, 0, 4, 122, 98, 76832),
          "k_ms_factor<false> with the inverse staged in LDS, k_ms_solve<false>: the panel read from HBM"),
    Shape("hbm-li142-hbm", (63, 32, 3), {}, (348, 189, 142), 16, _plan(0, 1, 0, 8, 174, 142, 161312),
          "max_w = 142: the widest panel whose inverse is still staged in LDS (142^2 = 20164 <= 20352)"),
    Shape("hbm-hbm143-hbm", (64, 31, 3), {}, (349, 192, 142), 16, _plan(0, 0, 0, 8, 175, 143, 0),
          "max_w = 143: the narrowest panel whose inverse is written straight to HBM (143^2 = 20449), no dynamic LDS in the factorisation"),
    Shape("hbm-hbm-hbm", (64, 40, 3), {}, (376, 192, 157), 16, _plan(0, 0, 0, 9, 184, 152, 0),
          "everything in HBM, 9 assembly / Gram chunks"),
]
BY_NAME = {s.name: s for s in SHAPES}
ALL_HBM = "hbm-hbm-hbm"
# the four factor / solve configurations of plan_lds() as (factor_in_lds, li_in_lds, solve_in_lds).  Of the other combinations (0, 0, 1) cannot occur (a panel wider than
# 142 has w^2 + h w >= 2 w^2 > 20352) and (1, 1, 0) only where h w + w^2 + 2 h exceeds the budget that h^2 + u^2 + w^2 still meets (u^2 < 2 h, at the very edge)
CONFIGURATIONS = {(1, 1, 1), (0, 1, 1), (0, 1, 0), (0, 0, 0)}
