"""Batches of small dense QPs that share one set of finite bounds and are feasible by construction, for the tests of the batched DenseSolver.

feasible_batch(n, p, m, batch, pattern): seed = 1000 n + 10 p + m.  The bound kinds of the batch come from default_rng(seed): per row of G both bounds / lower only /
upper only (1/3 each), per variable both box bounds / lower / upper / none (1/4 each); pattern "no box" sets every variable to none, "lower box" every variable to
lower only.  Instance i uses default_rng(seed * 100003 + i): P, c, A, G as random_qp of tests/test_dense_exact_gpu.py draws them, then a planted x0 ~ N(0, 1),
b = A x0, general bounds G x0 -/+ U(0.1, 1) and box bounds x0 -/+ U(0.1, 1), about 30 % of the lower ones of either kind active (distance 0).  random_qp's own b and
bounds are not used: with a shared pattern they give infeasible instances that run to the iteration limit.

ruiz_numpy (tests/ruiz_shapes.py, the dense first run of ruiz_reference) restates RuizEquilibration::scale_data in NumPy, one IEEE operation per oracle operation; the
oracle exposes its scaled data but not its scalings, so a test first holds this restatement to the oracle's scaled data bit for bit and then takes delta, delta_b and c
from it."""
import numpy as np

from ruiz_shapes import limit_scaling, ruiz_numpy  # noqa: F401  (the tests of the batched solvers import them from here)
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
