"""Batches of small dense QPs in which every instance has a set of finite bounds of its own, feasible by construction, for the tests of the batched DenseSolver
with per-instance bound sets.

mixed_batch(n, p, m, batch, salt=0): seed = 1000 n + 10 p + m.  Instance i takes P, c, A, G from random_qp(n, p, m, seed * 100003 + i) of
tests/test_dense_exact_gpu.py, then a planted x0, b = A x0 and the distances of its bounds from G x0 and x0 exactly as feasible_batch of tests/batch_qp.py draws
them (the same generator, the same draws in the same order).  Its bound kinds come from default_rng((seed * 7919 + i) * 31 + salt): per row of G both bounds / lower
only / upper only / NEITHER (0..3, 1/4 each; a row with neither is one DenseSolver drops), per variable both box bounds / lower / upper / none (0..3).  Four
instances are forced, f = (i + salt) % batch:
    f = 0   every row and every variable two-sided
    f = 1   rows lower only, no box at all
    f = 2   rows upper only, every variable boxed on both sides
    f = 3   every row of G without a bound (all dropped), lower boxes only
salt changes the patterns only: P, A, G, x0 and the distances stay, so the bounds of salt = 1 are an update of the instance of salt = 0 that keeps it feasible."""
import numpy as np

from test_dense_exact_gpu import random_qp

FORCED = {0: (0, 0), 1: (1, 3), 2: (2, 0), 3: (3, 1)}  # f -> (kind of every row, kind of every variable)


def kinds(n, p, m, batch, i, salt=0):
    """(row kinds [m], variable kinds [n]) of instance i"""
    seed = 1000 * n + 10 * p + m
    rng = np.random.default_rng((seed * 7919 + i) * 31 + salt)
    row = rng.integers(0, 4, m)
    var = rng.integers(0, 4, n)
    f = (i + salt) % batch
    if f in FORCED:
        row[:], var[:] = FORCED[f]
    return row, var


def mixed_batch(n, p, m, batch, salt=0):
    """list of `batch` dicts with the keys of batch_qp.KEYS (A, b / G, h_l, h_u missing when p / m is 0)"""
    seed = 1000 * n + 10 * p + m
    out = []
    for i in range(batch):
        row, var = kinds(n, p, m, batch, i, salt)
        q0, r = random_qp(n, p, m, seed=seed * 100003 + i)
        q = dict(P=q0["P"], c=q0["c"])
        x0 = r.standard_normal(n)
        if p:
            q.update(A=q0["A"], b=q0["A"] @ x0)
        if m:
            g = q0["G"] @ x0
            lo = np.where(r.uniform(size=m) < 0.3, 0.0, r.uniform(0.1, 1.0, m))
            hi = r.uniform(0.1, 1.0, m)
            q.update(G=q0["G"], h_l=np.where(row <= 1, g - lo, -np.inf), h_u=np.where((row == 0) | (row == 2), g + hi, np.inf))
        lo = np.where(r.uniform(size=n) < 0.3, 0.0, r.uniform(0.1, 1.0, n))
        hi = r.uniform(0.1, 1.0, n)
        q["x_l"] = np.where(var <= 1, x0 - lo, -np.inf)
        q["x_u"] = np.where((var == 0) | (var == 2), x0 + hi, np.inf)
        out.append(q)
    return out


def forced_lists(n, m, f):
    """the (h_l_idx, h_u_idx, x_l_idx, x_u_idx) DenseSolver holds for the forced instance f (a dropped row is in both row lists)"""
    rows, cols, none = list(range(m)), list(range(n)), []
    return {0: (rows, rows, cols, cols), 1: (rows, none, none, none), 2: (none, rows, cols, cols), 3: (rows, rows, cols, none)}[f]


_oracle = {}


def oracle_of_mixed(orc, hip, n, p, m, batch, kind, salt=0, **kw):
    """(the batch, every instance through orc.Solver): computed once per key and shared by the tests; nobody changes it"""
    from test_dense_solver_batch_gpu import oracle_run
    key = (n, p, m, batch, kind, salt, tuple(sorted(kw.items())))
    if key not in _oracle:
        qs = mixed_batch(n, p, m, batch, salt)
        _oracle[key] = (qs, oracle_run(orc, hip, qs, kind, **kw))
    return _oracle[key]


def hinges_on_a_rounding(orc, q, q1, name):
    """An update of instance q with h_l or h_u (`name`) of q1 ALONE: True when the reference's lists after it hinge on a rounding.  The reference stores an infinite
    bound as -/+ 1e30, multiplies it by its row's scaling (the tail of scale_data) and by the inverse (unscale_data at the update), and its disable_inf_constraints
    compares that number with 1e30: where the given bound is infinite and the stored other one is too, the row is dropped if the product came back to 1e30 and is left
    in neither list if it came back as its neighbour; and a drop makes it take both lists again from the numbers.  The library takes a stored infinite bound as infinite and drops the row (include/piqp_amd.h), so on such an
    instance the two differ by rule.  The scalings are ruiz_numpy's, which tests/test_dense_solver_batch_gpu.py holds to the oracle bit for bit."""
    from batch_qp import ruiz_numpy
    other = "h_u" if name == "h_l" else "h_l"
    m, n = len(q[name]), len(q["c"])
    p = len(q["b"]) if "b" in q else 0
    od = orc.Data.dense(**q)
    _, (delta, _, _) = ruiz_numpy(od.mat("P_utri"), od.mat("AT"), od.mat("GT"), od.vec("c"), od.vec("x_b_scaling"), 10, 0)
    d = delta[n + p:]
    back = (np.array(od.vec(other)) * d) * (1.0 / d)  # the stored numbers as the update sees them (a row dropped at the setup: -1 / 1)
    infinite = np.abs(np.array(od.vec(other))) >= 1e30
    drifted = infinite & (np.abs(back) < 1e30)
    # a drifted row under an infinite given bound is left in neither list; and once any row is dropped the reference takes both lists again from the numbers, which
    # puts every drifted row into the list of the side that was not given
    return m > 0 and bool(drifted.any() and (infinite & ~np.isfinite(q1[name])).any())


def reference_lists_after_one_sided(orc, q, q1, name):
    """(counts, {list name: list}) the reference holds after update(h_l or h_u = q1[name] ALONE) of instance q, from its rules on the NUMBERS it stores
    (dense/data.hpp:98-169): the given side's list from the given vector; a row is dropped when the given bound and the stored number of the other side -- after the
    scaling and un-scaling described at hinges_on_a_rounding -- both compare as infinite; if any row is dropped both lists are taken again from the numbers, else the
    list of the other side stays as it is.  The box lists stay."""
    from batch_qp import ruiz_numpy
    other = "h_u" if name == "h_l" else "h_l"
    m, n = len(q[name]), len(q["c"])
    p = len(q["b"]) if "b" in q else 0
    od = orc.Data.dense(**q)
    _, (delta, _, _) = ruiz_numpy(od.mat("P_utri"), od.mat("AT"), od.mat("GT"), od.vec("c"), od.vec("x_b_scaling"), 10, 0)
    d = delta[n + p:]
    back = (np.array(od.vec(other)) * d) * (1.0 / d)
    finite = {name: q1[name] > -1e30 if name == "h_l" else q1[name] < 1e30, other: back > -1e30 if other == "h_l" else back < 1e30}
    dead = ~finite[name] & ~finite[other]
    old = np.zeros(m, dtype=bool)
    old[od.idx(other)] = True
    lists = {name: np.flatnonzero(finite[name] | dead).tolist(), other: np.flatnonzero(finite[other] | dead if dead.any() else old).tolist(),
             "x_l": od.idx("x_l").tolist(), "x_u": od.idx("x_u").tolist()}
    return tuple(len(lists[k]) for k in ("h_l", "h_u", "x_l", "x_u")), lists
