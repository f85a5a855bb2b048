"""The batched KKTSystem with finite-bound lists per instance (BatchKKTSystem.per_instance, pq_kktsys_batch_create_dense_lists, pq_kktsys_batch_set_lists;
piqp_amd/csrc/dense_kktsys_batch.hip): every instance is compared with its own CPU oracle, orc.KKTSystem over orc.Data.dense of that instance, on the raw doubles.
There is no tolerance in this file and no instance is left out: equality is same() of tests/test_dense_exact_gpu.py.

Inputs follow Sys of tests/test_kktsys_batch_gpu.py -- random_qp data, x_b_scaling, states and right-hand sides drawn in the same way, the handle fed the oracle's own
P_utri / AT / GT and lists -- with the bound kinds of instance i those of tests/batch_qp_mixed.py (kinds): rows with both / lower / upper / NO bound, variables with
both / lower / upper / no box bound, four forced instances.  A row without a bound is dropped by the oracle's data: its row of G is zero and it is in both lists.
Of a box vector the entries an instance's own count covers are compared.

Shapes: (4, 2, 3, 67), four instances with different counts per workgroup of the factor launch and a ragged last one; (33, 0, 300, 9), a workgroup per instance, m
past one K block.  Both factorisations.  iterative_refinement_static_regularization_eps = 1e-4, so that refinement steps occur: that they do, with different counts in
a batch, is asserted on the oracle before the device is touched."""
import numpy as np
import pytest

from batch_qp_mixed import kinds
from test_dense_exact_gpu import lower, random_qp, same
from test_kktsys_batch_gpu import KINDS, NAMES, VARIANTS, Sys, oracle_step, row

pytestmark = pytest.mark.gpu

SHAPES = [(4, 2, 3, 67), (33, 0, 300, 9)]
LISTS = ("h_l", "h_u", "x_l", "x_u")
VARIANT = "B"  # iterative_refinement_static_regularization_eps = 1e-4


class MixedSys(Sys):
    """Sys with a bound pattern per instance (salt: another set of patterns over the same matrices, x_b_scaling and bound values)"""

    def __init__(self, orc, n, p, m, batch, salt=0):
        self.n, self.p, self.m, self.batch = n, p, m, batch
        self.seed = seed = 1000 * n + 10 * p + m
        self.q, self.xbs = [], np.zeros((batch, n))
        for i in range(batch):
            rw, var = kinds(n, p, m, batch, i, salt)
            q, r = random_qp(n, p, m, seed=seed * 100003 + i)
            if m:
                q["h_l"] = np.where(rw <= 1, q["h_l"], -np.inf)
                q["h_u"] = np.where((rw == 0) | (rw == 2), q["h_u"], np.inf)
            q["x_l"] = np.where(var <= 1, -r.uniform(0.5, 2.0, n), -np.inf)
            q["x_u"] = np.where((var == 0) | (var == 2), r.uniform(0.5, 2.0, n), np.inf)
            self.xbs[i] = r.uniform(0.5, 2.0, n)
            self.q.append(q)
        self.od = [orc.Data.dense(**q) for q in self.q]
        for od, xbs in zip(self.od, self.xbs):
            od.vec("x_b_scaling")[:] = xbs
        self.lists = [tuple(od.idx(nm) for nm in LISTS) for od in self.od]
        self.P = np.stack([np.array(od.mat("P_utri")) for od in self.od])
        self.A = np.stack([np.array(od.mat("AT")).T for od in self.od]) if p else None
        self.G = np.stack([np.array(od.mat("GT")).T for od in self.od]) if m else None
        self.shapes = dict(zip(NAMES, ((batch, n), (batch, p), (batch, m), (batch, m), (batch, n), (batch, n), (batch, m), (batch, m), (batch, n), (batch, n))))

    def used(self, i):
        """how much of a row of instance i means something"""
        nl, nu = len(self.lists[i][2]), len(self.lists[i][3])
        return dict(zip(NAMES, (self.n, self.p, self.m, self.m, nl, nu, self.m, self.m, nl, nu)))

    def handle(self, hip, kind, variant=VARIANT):
        return hip.BatchKKTSystem.per_instance(self.P, self.A, self.G, self.lists, x_b_scaling=self.xbs, settings=hip.default_settings(**VARIANTS[variant]), kkt_solver=kind)


_cache = {}


def sys_of(orc, n, p, m, batch, salt=0):
    key = (n, p, m, batch, salt)
    if key not in _cache:
        _cache[key] = MixedSys(orc, n, p, m, batch, salt)
    return _cache[key]


def check_vars(B, got, ref_rows, tag):
    bad = []
    for i, ref in enumerate(ref_rows):
        used = B.used(i)
        bad += [(i, nm) for nm in NAMES if not same(np.asarray(got[nm])[i, :used[nm]], ref[nm][:used[nm]])]
    assert not bad, (tag, bad)


def step(k, kos, B, flags, rng, tag):
    """one update_scalings_and_factor, solve and mul on every oracle and on the handle: x_reg, z_reg, the factor, the ten-vector step, the refinement step counts, the
    backend solves and mul, per instance"""
    flags = np.broadcast_to(np.asarray(flags, dtype=np.int32), (B.batch,))
    state, rhs, lhs_mul = B.state(rng), B.normal(rng), B.normal(rng)
    R = oracle_step(kos, flags, state, rhs, lhs_mul)
    assert all(R["ok_f"]) and all(R["ok_s"]), (tag, "every instance factors and solves on the oracle")
    if flags.any() and B.p + B.m > 0:
        assert len(set(np.array(R["steps"])[flags != 0])) >= 2, (tag, "the instances must take different numbers of refinement steps", R["steps"])
    rho, delta, v = state
    assert k.update_scalings_and_factor(flags, rho, delta, v) == B.batch, tag
    kb, xr, zr = k.backend(), k.x_reg(), k.z_reg()
    bad = []
    for i in range(B.batch):
        bad += [(i, what) for what, a, b in (("x_reg", xr[i], R["x_reg"][i]), ("z_reg", zr[i], R["z_reg"][i]), ("factor", lower(kb.internal_factor(i)), R["factor"][i])) if not same(a, b)]
    assert not bad, (tag, bad)
    got = k.solve(rhs)
    assert k.solve_ok().all(), tag
    check_vars(B, got, R["lhs"], (tag, "solve"))
    assert np.array_equal(k.refine_steps(), R["steps"]) and np.array_equal(k.backend_solves(), R["solves"]), (tag, k.refine_steps(), R["steps"])
    rxb, rzb = k.rhs_x_bar(), k.rhs_z_bar()
    assert all(same(rxb[i], R["rxb"][i]) and same(rzb[i], R["rzb"][i]) for i in range(B.batch)), (tag, "rhs_bar")
    check_vars(B, k.mul(lhs_mul), R["mul"], (tag, "mul"))
    return R


@pytest.mark.parametrize("n,p,m,batch", SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_every_instance_with_its_own_lists_is_bitwise_the_oracle_s(hip, orc, kind, n, p, m, batch):
    B = sys_of(orc, n, p, m, batch)
    assert len({tuple(len(l) for l in t) for t in B.lists}) >= 3, "the instances must hold different sets"
    assert any(len(t[2]) == 0 for t in B.lists) and any(len(t[2]) == n for t in B.lists) and any(not np.array(od.mat("GT")).any() for od in B.od)
    rng = np.random.default_rng([B.seed, kind, 11])
    k, kos = B.handle(hip, kind), B.oracles(orc, kind, VARIANT)
    for flags, what in ((0, "off"), (1, "on"), ((np.arange(batch) % 2).astype(np.int32), "alternating")):
        step(k, kos, B, flags, rng, (n, p, m, what))
    # a clone carries the kind of the lists, the tables, the scalings state and the factors
    c = k.clone()
    rhs = B.normal(rng)
    ref = [ko.solve(row(rhs, i)) for i, ko in enumerate(kos)]
    got = c.solve(rhs)
    assert np.array_equal(c.solve_ok(), [ok for ok, _ in ref])
    check_vars(B, got, [lhs for _, lhs in ref], ("clone: solve",))
    assert np.array_equal(c.refine_steps(), [ko.last_refine_steps() for ko in kos])
    step(c, kos, B, 1, rng, (n, p, m, "clone: a step of its own"))


@pytest.mark.parametrize("n,p,m,batch", SHAPES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_set_lists_to_another_pattern(hip, orc, kind, n, p, m, batch):
    B, B1 = sys_of(orc, n, p, m, batch), sys_of(orc, n, p, m, batch, salt=1)
    assert sum(any(not np.array_equal(a, b) for a, b in zip(t, t1)) for t, t1 in zip(B.lists, B1.lists)) >= batch - 2, "the lists are to change"
    rng = np.random.default_rng([B.seed, kind, 12])
    k = B.handle(hip, kind)
    step(k, B.oracles(orc, kind, VARIANT), B, 1, rng, (n, p, m, "before"))
    c0 = k.L.pq_debug_alloc_count()
    k.set_lists(B1.lists)
    assert k.L.pq_debug_alloc_count() == c0, "set_lists must not allocate"
    with pytest.raises(RuntimeError, match="before update_scalings_and_factor"):  # the factors belong to the old lists
        k.solve(B1.normal(rng))
    k.update_data(G=B1.G)  # the rows the new patterns drop are zero in the oracle's G, those that came back are not
    k1 = k.clone()
    step(k, B1.oracles(orc, kind, VARIANT), B1, 1, rng, (n, p, m, "after"))
    step(k1, B1.oracles(orc, kind, VARIANT), B1, 0, rng, (n, p, m, "a clone taken after set_lists"))
    # a shared handle has no lists to replace
    shared = Sys(orc, 4, 2, 3, 5)
    with pytest.raises(RuntimeError):
        shared.handle(hip, kind).set_lists([tuple(shared.lists)] * 5)
