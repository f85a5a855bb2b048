"""Batches of small dense QPs that share one set of finite bounds and are feasible by construction, for the tests of the batched DenseSolver.

feasible_batch(n, p, m, batch, pattern): seed = 1000 n + 10 p + m.  The bound kinds of the batch come from default_rng(seed): per row of G both bounds / lower only /
upper only (1/3 each), per variable both box bounds / lower / upper / none (1/4 each); pattern "no box" sets every variable to none, "lower box" every variable to
lower only.  Instance i uses default_rng(seed * 100003 + i): P, c, A, G as random_qp of tests/test_dense_exact_gpu.py draws them, then a planted x0 ~ N(0, 1),
b = A x0, general bounds G x0 -/+ U(0.1, 1) and box bounds x0 -/+ U(0.1, 1), about 30 % of the lower ones of either kind active (distance 0).  random_qp's own b and
bounds are not used: with a shared pattern they give infeasible instances that run to the iteration limit.

ruiz_numpy restates RuizEquilibration::scale_data (dense, first run) in NumPy, one IEEE operation per oracle operation; the oracle exposes its scaled data but not its
scalings, so a test first holds this restatement to the oracle's scaled data bit for bit and then takes delta, delta_b and c from it."""
import numpy as np

from test_dense_exact_gpu import random_qp

KEYS = ("P", "c", "A", "b", "G", "h_l", "h_u", "x_l", "x_u")


def feasible_batch(n, p, m, batch, pattern="random"):
    """list of `batch` dicts with the keys of KEYS (A, b / G, h_l, h_u missing when p / m is 0)"""
    seed = 1000 * n + 10 * p + m
    rng = np.random.default_rng(seed)
    row = rng.integers(0, 3, m)  # 0 both bounds, 1 lower only, 2 upper only
    var = rng.integers(0, 4, n)  # 0 both box bounds, 1 lower only, 2 upper only, 3 none
    if pattern == "no box":
        var[:] = 3
    elif pattern == "lower box":
        var[:] = 1
    else:
        assert pattern == "random"
    out = []
    for i in range(batch):
        q0, r = random_qp(n, p, m, seed=seed * 100003 + i)
        q = dict(P=q0["P"], c=q0["c"])
        x0 = r.standard_normal(n)
        if p:
            q.update(A=q0["A"], b=q0["A"] @ x0)
        if m:
            g = q0["G"] @ x0
            lo = np.where(r.uniform(size=m) < 0.3, 0.0, r.uniform(0.1, 1.0, m))
            hi = r.uniform(0.1, 1.0, m)
            q.update(G=q0["G"], h_l=np.where(row == 2, -np.inf, g - lo), h_u=np.where(row == 1, np.inf, g + hi))
        lo = np.where(r.uniform(size=n) < 0.3, 0.0, r.uniform(0.1, 1.0, n))
        hi = r.uniform(0.1, 1.0, n)
        q["x_l"] = np.where(var <= 1, x0 - lo, -np.inf)
        q["x_u"] = np.where((var == 0) | (var == 2), x0 + hi, np.inf)
        out.append(q)
    return out


def stacked(qs):
    """dict name -> [batch, ...] array (None where the batch has none)"""
    return {k: (np.stack([q[k] for q in qs]) if k in qs[0] else None) for k in KEYS}


def limit_scaling(d):
    return np.where(d < 1e-4, 1.0, np.where(d > 1e4, 1e4, d))


def ruiz_numpy(P_utri, AT, GT, c, x_b_scaling, max_iter, scale_cost, epsilon=1e-3):
    """orc_solver.c:136-227 on copies of one instance's unscaled data (P_utri n x n with a zero lower triangle, AT n x p, GT n x m).  Returns the scaled
    (P_utri, AT, GT, c, x_b_scaling) and (delta, delta_b, c_scale)."""
    P, AT, GT, c, xbs = (np.array(a, dtype=np.float64, order="F") for a in (P_utri, AT, GT, c, x_b_scaling))
    n, p, m = P.shape[0], AT.shape[1], GT.shape[1]
    N = n + p + m
    delta, delta_b, rc = np.ones(N), np.ones(n), 1.0
    di, dib = np.zeros(N), np.zeros(n)
    iu = np.triu(np.ones((n, n), dtype=bool))
    for _ in range(max_iter):
        dev = max(np.max(np.abs(1.0 - di)), np.max(np.abs(1.0 - dib)))
        if not dev > epsilon:
            break
        S = np.abs(np.where(iu, P, P.T))  # the symmetric matrix the upper triangle stands for
        v = S.max(axis=1)
        if p:
            v = np.maximum(v, np.abs(AT).max(axis=1))
        if m:
            v = np.maximum(v, np.abs(GT).max(axis=1))
        di[:n] = np.maximum(v, xbs)
        di[n:n + p] = np.abs(AT).max(axis=0) if p else 0.0
        di[n + p:] = np.abs(GT).max(axis=0) if m else 0.0
        dib[:] = xbs
        di = 1.0 / np.sqrt(limit_scaling(di))
        dib = 1.0 / np.sqrt(limit_scaling(dib))
        P = np.where(iu, (P * di[None, :n]) * di[:n, None], P)  # the column pass, then the row pass
        c = c * di[:n]
        AT = (di[:n, None] * AT) * di[None, n:n + p]
        GT = (di[:n, None] * GT) * di[None, n + p:]
        xbs = xbs * (dib * di[:n])
        delta = delta * di
        delta_b = delta_b * dib
        if scale_cost:
            cm = np.abs(np.where(iu, P, P.T)).max(axis=1)
            gamma = 0.0
            for k in range(n):
                gamma += cm[k]
            gamma = float(limit_scaling(gamma / n))
            gamma = max(gamma, float(np.max(np.abs(c))))
            gamma = 1.0 / float(limit_scaling(gamma))
            P = P * gamma
            c = c * gamma
            rc = rc * gamma
    return (P, AT, GT, c, xbs), (delta, delta_b, np.array([rc]))
