"""The batched KKTSystem (piqp_amd/csrc/dense_kktsys_batch.hip, pq_kktsys_batch_*, piqp_amd.BatchKKTSystem; n <= 128): every instance of a batch is compared with
its own CPU oracle, orc.KKTSystem(orc.Data.dense(**q_i), orc.Settings(kkt_solver=0 or 16, ...)) (oracle/orc_kkt_system.c over oracle/orc_dense.c), on the raw doubles.
There is no tolerance in this file and no instance is left out: equality is same() of tests/test_dense_exact_gpu.py (the uint64 views).  The handle is fed the oracle's
own P_utri / AT / GT and index lists; the per-instance x_b_scaling is written into the oracle's data through od.vec("x_b_scaling").

Inputs: instance i of a batch is random_qp(n, p, m, seed * 100003 + i) with seed = 1000 n + 10 p + m; the bound pattern shared by the batch comes from
np.random.default_rng(seed): per row of G both bounds / lower only / upper only (1/3 each), per variable both box bounds / lower / upper / none (1/4 each).  Per
instance x_b_scaling is uniform in [0.5, 2), every s and z entry 10^U(-6, 2), rho and delta 10^U(-9, -3), right-hand sides standard normal.

The oracle's results of a step are computed once (oracle_step) and compared with the device's afterwards; the conditions the refinement tests need (instances of one
batch taking different numbers of steps) are asserted on the oracle alone before the device is touched.  One of them cannot hold for any input: at the shape
(1, 0, 0) there is no A and no G, the static regularisation sits in x_reg alone, the condensed matrix is the factored one, and with a positive tolerance no
instance takes a step; there the test asserts exactly that (zero steps everywhere) and two distinct counts only where the tolerance is zero."""
import numpy as np
import pytest

from test_dense_exact_gpu import lower, random_qp, same
from test_dense_kkt_batch_gpu import carved, patterned

pytestmark = pytest.mark.gpu

LLT, LDLT = 0, 16
KINDS = [pytest.param(LLT, id="llt"), pytest.param(LDLT, id="ldlt")]
NAMES = ("x", "y", "z_l", "z_u", "z_bl", "z_bu", "s_l", "s_u", "s_bl", "s_bu")
SHAPES = [(1, 0, 0, 67), (4, 2, 3, 67), (31, 7, 5, 67), (32, 3, 5, 9), (33, 0, 300, 9), (64, 40, 257, 9), (128, 7, 5, 9)]
# the settings variants of the refinement tests
VARIANTS = {
    "default": {},
    "B": dict(iterative_refinement_static_regularization_eps=1e-4),
    "D": dict(iterative_refinement_static_regularization_eps=1e-4, iterative_refinement_eps_abs=0.0, iterative_refinement_eps_rel=0.0),
    "E": dict(iterative_refinement_static_regularization_eps=1e-4, iterative_refinement_max_iter=2),
}


class Sys:
    """`batch` random QPs of one shape with one bound pattern, each with data and x_b_scaling of its own, and the oracle's view of them"""

    def __init__(self, orc, n, p, m, batch, pattern="random", free=(), edit=None):
        self.n, self.p, self.m, self.batch = n, p, m, batch
        self.seed = seed = 1000 * n + 10 * p + m
        rng = np.random.default_rng(seed)
        row = rng.integers(0, 3, m)  # 0 both bounds, 1 lower only, 2 upper only
        var = rng.integers(0, 4, n)  # 0 both box bounds, 1 lower only, 2 upper only, 3 none
        if pattern == "no box":
            var[:] = 3
        elif pattern == "every box":
            var[:] = 0
        elif pattern == "two-sided rows":
            row[:] = 0
        var[list(free)] = 3
        self.q, self.xbs = [], np.zeros((batch, n))
        for i in range(batch):
            q, r = random_qp(n, p, m, seed=seed * 100003 + i)
            if m:
                q["h_l"] = np.where(row == 2, -np.inf, q["h_l"])
                q["h_u"] = np.where(row == 1, np.inf, q["h_u"])
            q["x_l"] = np.where(var <= 1, -r.uniform(0.5, 2.0, n), -np.inf)
            q["x_u"] = np.where((var == 0) | (var == 2), r.uniform(0.5, 2.0, n), np.inf)
            self.xbs[i] = r.uniform(0.5, 2.0, n)
            self.q.append(q)
        if edit:
            edit(self.q)
        self.od = [orc.Data.dense(**q) for q in self.q]
        for od, xbs in zip(self.od, self.xbs):
            od.vec("x_b_scaling")[:] = xbs
        self.lists = [self.od[0].idx(nm) for nm in ("h_l", "h_u", "x_l", "x_u")]
        assert all(np.array_equal(od.idx(nm), l) for od in self.od for nm, l in zip(("h_l", "h_u", "x_l", "x_u"), self.lists))
        assert np.array_equal(self.lists[2], np.flatnonzero(var <= 1)) and np.array_equal(self.lists[3], np.flatnonzero((var == 0) | (var == 2)))
        self.P = np.stack([np.array(od.mat("P_utri")) for od in self.od])
        self.A = np.stack([np.array(od.mat("AT")).T for od in self.od]) if p else None
        self.G = np.stack([np.array(od.mat("GT")).T for od in self.od]) if m else None
        self.shapes = dict(zip(NAMES, ((batch, n), (batch, p), (batch, m), (batch, m), (batch, n), (batch, n), (batch, m), (batch, m), (batch, n), (batch, n))))
        # how much of a row means something
        self.used = dict(zip(NAMES, (n, p, m, m, len(self.lists[2]), len(self.lists[3]), m, m, len(self.lists[2]), len(self.lists[3]))))

    def handle(self, hip, kind, variant="default"):
        h_l, h_u, x_l, x_u = self.lists
        return hip.BatchKKTSystem(self.P, self.A, self.G, h_l_idx=h_l, h_u_idx=h_u, x_l_idx=x_l, x_u_idx=x_u, x_b_scaling=self.xbs,
                                  settings=hip.default_settings(**VARIANTS[variant]), kkt_solver=kind)

    def oracles(self, orc, kind, variant="default"):
        return [orc.KKTSystem(od, orc.Settings(kkt_solver=kind, **VARIANTS[variant])) for od in self.od]

    def state(self, rng):
        """an interior-point state: (rho, delta, vars)"""
        v = {nm: 10.0 ** rng.uniform(-6, 2, self.shapes[nm]) if nm[0] in "sz" else np.zeros(self.shapes[nm]) for nm in NAMES}
        rho, delta = 10.0 ** rng.uniform(-9, -3, (2, self.batch))
        return rho, delta, v

    def normal(self, rng):
        return {nm: rng.standard_normal(self.shapes[nm]) for nm in NAMES}


_cache = {}


def sys_of(orc, n, p, m, batch, pattern="random"):
    key = (n, p, m, batch, pattern)
    if key not in _cache:
        _cache[key] = Sys(orc, n, p, m, batch, pattern)
    return _cache[key]


def row(v, i):
    return {nm: np.ascontiguousarray(a[i]) for nm, a in v.items()}


def oracle_step(kos, flags, state, rhs, lhs_mul):
    """update_scalings_and_factor, solve and mul of every oracle, each on its own row; everything a device result is compared with"""
    rho, delta, v = state
    R = dict(ok_f=[], x_reg=[], z_reg=[], factor=[], ok_s=[], lhs=[], steps=[], solves=[], rxb=[], rzb=[], mul=[])
    for i, ko in enumerate(kos):
        ok = ko.update_scalings_and_factor(int(flags[i]), float(rho[i]), float(delta[i]), row(v, i))
        R["ok_f"].append(ok)
        R["x_reg"].append(ko.x_reg())
        R["z_reg"].append(ko.z_reg())
        R["factor"].append(lower(ko.backend().internal_factor()).copy() if ok else None)
        if ok:
            before = ko.L.orc_kkt_system_backend_solves(ko.ptr)
            ok_s, lhs = ko.solve(row(rhs, i))
            R["ok_s"].append(ok_s)
            R["lhs"].append(lhs)
            R["steps"].append(ko.last_refine_steps())
            R["solves"].append(ko.L.orc_kkt_system_backend_solves(ko.ptr) - before)
            R["rxb"].append(ko.rhs_x_bar())
            R["rzb"].append(ko.rhs_z_bar())
        else:
            for nm in ("lhs", "rxb", "rzb"):
                R[nm].append(None)
            R["ok_s"].append(False)
            R["steps"].append(0)
            R["solves"].append(0)
        R["mul"].append(ko.mul(row(lhs_mul, i)))
    return R


def check_vars(B, got, ref_rows, tag, only=None):
    bad = []
    for i, ref in enumerate(ref_rows):
        if ref is None or (only is not None and not only[i]):
            continue
        bad += [(i, nm) for nm in NAMES if not same(np.asarray(got[nm])[i, :B.used[nm]], ref[nm][:B.used[nm]])]
    assert not bad, (tag, bad)


def device_step(k, B, flags, state, rhs, lhs_mul, R, tag, out=None):
    """the same step on the handle, every number against the oracle's; returns the solve's output"""
    rho, delta, v = state
    n_ok = k.update_scalings_and_factor(flags, rho, delta, v)
    assert n_ok == sum(R["ok_f"]), (tag, n_ok, R["ok_f"])
    kb = k.backend()
    assert np.array_equal(kb.ok(), R["ok_f"]), (tag, kb.ok(), R["ok_f"])
    xr, zr = k.x_reg(), k.z_reg()
    bad = []
    for i in range(B.batch):
        if not same(xr[i], R["x_reg"][i]):
            bad.append((i, "x_reg"))
        if not same(zr[i], R["z_reg"][i]):
            bad.append((i, "z_reg"))
        if R["ok_f"][i] and not same(lower(kb.internal_factor(i)), R["factor"][i]):
            bad.append((i, "factor"))
    assert not bad, (tag, bad)
    got = k.solve(rhs, out=out)
    assert np.array_equal(k.solve_ok(), R["ok_s"]), (tag, k.solve_ok(), R["ok_s"])
    check_vars(B, got, R["lhs"], (tag, "solve"), only=R["ok_s"])
    live = np.array(R["ok_f"], dtype=bool)
    assert np.array_equal(k.refine_steps()[live], np.array(R["steps"])[live]), (tag, k.refine_steps(), R["steps"])
    assert np.array_equal(k.backend_solves()[live], np.array(R["solves"])[live]), (tag, k.backend_solves(), R["solves"])
    rxb, rzb = k.rhs_x_bar(), k.rhs_z_bar()
    bad = [(i, "rhs_bar") for i in range(B.batch) if R["ok_s"][i] and not (same(rxb[i], R["rxb"][i]) and same(rzb[i], R["rzb"][i]))]
    assert not bad, (tag, bad)
    check_vars(B, k.mul(lhs_mul), R["mul"], (tag, "mul"))
    return got


def step(k, kos, B, flags, rng, tag):
    flags = np.broadcast_to(np.asarray(flags, dtype=np.int32), (B.batch,))
    args = (B.state(rng), B.normal(rng), B.normal(rng))
    R = oracle_step(kos, flags, *args)
    device_step(k, B, flags, *args, R, tag)
    return R


# ---- 1. every member, refinement off and on, default settings
def every_member(hip, orc, kind, B):
    rng = np.random.default_rng([B.seed, kind])
    k, kos = B.handle(hip, kind), B.oracles(orc, kind)
    assert (k.batch, k.n, k.p, k.m) == (B.batch, B.n, B.p, B.m)
    tag = (B.n, B.p, B.m)
    for flags, what in ((0, "off"), (1, "on"), (0, "off again"), (1, "on again")):
        R = step(k, kos, B, flags, rng, tag + (what,))
        assert all(R["ok_f"]) and all(R["ok_s"]), (tag, what, "the recipe's instances all factor and solve on the oracle")
    # a clone carries the scalings state and the factors: a solve on it continues where the original stands
    c = k.clone()
    rhs = B.normal(rng)
    ref = [ko.solve(row(rhs, i)) for i, ko in enumerate(kos)]
    got = c.solve(rhs)
    assert np.array_equal(c.solve_ok(), [ok for ok, _ in ref])
    check_vars(B, got, [lhs for _, lhs in ref], (tag, "clone: solve"))
    assert np.array_equal(c.refine_steps(), [ko.last_refine_steps() for ko in kos])
    step(c, kos, B, 1, rng, tag + ("clone: a step of its own",))
    step(k, kos, B, 0, rng, tag + ("the original after the clone's step",))


@pytest.mark.parametrize("n,p,m,batch", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_member_is_bitwise_the_oracle_s(hip, orc, kind, n, p, m, batch):
    every_member(hip, orc, kind, sys_of(orc, n, p, m, batch))


@pytest.mark.parametrize("pattern", ["no box", "every box", "two-sided rows"])
@pytest.mark.parametrize("n,p,m,batch", [(31, 7, 5, 67), (33, 0, 300, 9)])
@pytest.mark.parametrize("kind", KINDS)
def test_bound_patterns(hip, orc, kind, n, p, m, batch, pattern):
    every_member(hip, orc, kind, sys_of(orc, n, p, m, batch, pattern))


# ---- 2. the refinement loop takes its own course per instance
_refine = {}


def refinement_reference(orc, shape, variant):
    """the oracle's step with refinement on everywhere under a settings variant (LLT), computed once"""
    key = (shape, variant)
    if key not in _refine:
        B = sys_of(orc, *shape)
        # (the third number picks a stream of states and right-hand sides with which the oracle meets every condition asserted below)
        rng = np.random.default_rng([B.seed, sorted(VARIANTS).index(variant), 4])
        kos = B.oracles(orc, LLT, variant)
        flags = np.ones(B.batch, dtype=np.int32)
        args = (B.state(rng), B.normal(rng), B.normal(rng))
        _refine[key] = (B, flags, args, oracle_step(kos, flags, *args))
    return _refine[key]


@pytest.mark.parametrize("variant", ["B", "D", "E"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_instance_takes_its_own_number_of_refinement_steps(orc, hip, shape, variant):
    B, flags, args, R = refinement_reference(orc, shape, variant)
    # on the oracle alone, before the device is touched: the batch is not uniform
    steps = np.array(R["steps"])
    max_iter = VARIANTS[variant].get("iterative_refinement_max_iter", 10)
    assert all(R["ok_f"]) and all(R["ok_s"])
    if shape[1] == shape[2] == 0 and variant != "D":
        # no A and no G: reg sits in x_reg alone, so the condensed matrix IS the factored one and the refine error of the first solve is one rounding of a
        # scalar, far below eps_abs = 1e-12: no instance can take a step unless the tolerance is zero (variant D).  The oracle says so for every stream.
        assert not steps.any(), (shape, variant, np.bincount(steps))
    else:
        assert len(set(steps)) >= 2, (shape, variant, np.bincount(steps))
    if shape == (4, 2, 3, 67) and variant == "B":
        assert len(set(steps)) >= 4 and (steps == max_iter).any(), np.bincount(steps)
    assert steps.max() <= max_iter
    device_step(B.handle(hip, LLT, variant), B, flags, *args, R, (shape, variant))


@pytest.mark.parametrize("shape", [(4, 2, 3, 67), (33, 0, 300, 9)], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_the_refinement_flag_alternates_within_a_batch(hip, orc, kind, shape):
    B = sys_of(orc, *shape)
    rng = np.random.default_rng([B.seed, kind, 2])
    flags = (np.arange(B.batch) % 2).astype(np.int32)
    k, kos = B.handle(hip, kind, "B"), B.oracles(orc, kind, "B")
    R = step(k, kos, B, flags, rng, (shape, "alternating"))
    assert not np.array(R["steps"])[flags == 0].any() and np.array(R["steps"])[flags == 1].any()
    step(k, kos, B, 1 - flags, rng, (shape, "the other way round"))
    k.set_settings(hip.default_settings(**VARIANTS["E"]))
    for ko in kos:
        ko.settings.s.iterative_refinement_max_iter = 2
    R = step(k, kos, B, flags, rng, (shape, "after set_settings"))
    assert max(R["steps"]) <= 2


@pytest.mark.parametrize("shape", [(4, 2, 3, 67), (33, 7, 5, 9)], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_the_borrowed_backend_is_as_its_own_factorisation_would_have_left_it(hip, orc, kind, shape):
    """after the system's launch the backend handle answers as after pq_kkt_batch_update_scalings_and_factor(delta_reg, x_reg, z_reg_iter_ref): its stored scalings
    (internal_kkt_mat recomputes the matrix from them) and its own solve are the oracle backend's"""
    B = sys_of(orc, *shape) if shape in SHAPES else Sys(orc, *shape)
    rng = np.random.default_rng([B.seed, kind, 7])
    flags = (np.arange(B.batch) % 2).astype(np.int32)
    k, kos = B.handle(hip, kind, "B"), B.oracles(orc, kind, "B")
    step(k, kos, B, flags, rng, (shape, "system"))
    kb, b = k.backend(), B.batch
    assert kb.ok().all() and (kb.first_bad_col() == -1).all()
    rx, ry, rz = rng.standard_normal((b, B.n)), rng.standard_normal((b, B.p)), rng.standard_normal((b, B.m))
    got = kb.solve(rx, ry, rz)
    bad = []
    for i, ko in enumerate(kos):
        ob = ko.backend()
        if not same(lower(kb.internal_kkt_mat(i)), lower(ob.internal_kkt_mat())):
            bad.append((i, "kkt_mat"))
        bad += [(i, what) for g, ref, what in zip(got, ob.solve(rx[i], ry[i], rz[i]), ("lhs_x", "lhs_y", "lhs_z")) if not same(g[i], ref)]
    assert not bad, bad


# ---- 3. trouble stays in its instance
def test_an_llt_failure_stays_in_its_instance(hip, orc):
    import torch
    n, p, m, batch, cols = 33, 0, 0, 9, {2: 3, 7: 20}  # column 3 lies in the first panel of width 8, column 20 in the third

    def spoil(qs):
        for i, c in cols.items():
            qs[i]["P"][c, c] = -1e3
    B = Sys(orc, n, p, m, batch, free=cols.values(), edit=spoil)  # (the spoiled variables carry no box bound: nothing is added to their diagonal entries but rho)
    rng = np.random.default_rng(5)
    k, kos = B.handle(hip, LLT), B.oracles(orc, LLT)
    for flags in (0, 1):
        R = step(k, kos, B, flags, rng, ("spoiled", flags))
        assert [i for i in range(batch) if not R["ok_f"][i]] == sorted(cols), R["ok_f"]
        assert np.array_equal(k.backend().first_bad_col(), [cols.get(i, -1) for i in range(batch)])
        assert not k.solve_ok()[sorted(cols)].any() and k.solve_ok().sum() == batch - len(cols)
    # the ten rows of a failed instance keep the bit pattern they held before the call, in host and in device memory; the other instances are the oracle's
    rhs = B.normal(rng)
    before = {nm: patterned(B.shapes[nm], 1 + j) for j, nm in enumerate(NAMES)}
    out = {nm: a.copy() for nm, a in before.items()}
    k.solve(rhs, out=out)
    dout = {nm: torch.from_numpy(a.copy()).cuda() for nm, a in before.items()}
    k.solve({nm: torch.from_numpy(a).cuda() for nm, a in rhs.items()}, out=dout)
    ref = [ko.solve(row(rhs, i))[1] if i not in cols else None for i, ko in enumerate(kos)]
    check_vars(B, out, ref, "beside the failed instances")
    for i in range(batch):
        for nm in NAMES:
            assert same(out[nm][i], dout[nm][i].cpu().numpy()), (i, nm)
            if i in cols:
                assert same(out[nm][i], before[nm][i]), (i, nm)
            else:  # (what lies behind the meaningful part of a box row is not written either)
                assert same(out[nm][i, B.used[nm]:], before[nm][i, B.used[nm]:]), (i, nm)
    # repaired: all nine are the oracle's again
    G = Sys(orc, n, p, m, batch, free=cols.values())
    k.update_data(P=G.P)
    R = step(k, G.oracles(orc, LLT), G, 1, rng, "repaired")
    assert all(R["ok_f"])


@pytest.mark.parametrize("shape", [(4, 2, 3, 67), (33, 7, 5, 9)], ids=str)
@pytest.mark.parametrize("refine", [0, 1], ids=["off", "on"])
def test_a_nan_stays_in_its_instance(hip, orc, shape, refine):
    B = sys_of(orc, *shape) if shape in SHAPES else Sys(orc, *shape)
    rng = np.random.default_rng([B.seed, refine, 3])
    k, kos = B.handle(hip, LLT), B.oracles(orc, LLT)
    flags = np.full(B.batch, refine, dtype=np.int32)
    state, rhs, lhs_mul = B.state(rng), B.normal(rng), B.normal(rng)
    sick = B.batch // 2
    rhs["x"][sick, 0] = np.nan
    R = oracle_step(kos, flags, state, rhs, lhs_mul)
    assert [i for i in range(B.batch) if not R["ok_s"][i]] == [sick], R["ok_s"]
    device_step(k, B, flags, state, rhs, lhs_mul, R, (shape, "a NaN in rhs.x"))
    assert not k.solve_ok()[sick] and k.solve_ok().sum() == B.batch - 1
    step(k, kos, B, flags, rng, (shape, "after the NaN"))


# ---- 4. device memory equals host memory
@pytest.mark.parametrize("n,p,m,batch", [(8, 2, 6, 67), (33, 7, 5, 9), (64, 0, 0, 9)])
@pytest.mark.parametrize("kind", KINDS)
def test_device_memory_equals_host_memory(hip, orc, kind, n, p, m, batch):
    import torch
    L = hip._lib.load()
    B = sys_of(orc, n, p, m, batch)
    rng = np.random.default_rng([B.seed, kind, 4])
    kh = B.handle(hip, kind, "B")
    Pt = np.ascontiguousarray(B.P.transpose(0, 2, 1))  # the column-major P_utri[i] as a C-contiguous array; its unread triangle is all NaN
    Pt[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = np.nan
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    h_l, h_u, x_l, x_u = B.lists
    kd = hip.BatchKKTSystem(dev(Pt), dev(B.A), dev(B.G), h_l_idx=h_l, h_u_idx=h_u, x_l_idx=x_l, x_u_idx=x_u, x_b_scaling=dev(B.xbs),
                            settings=hip.default_settings(**VARIANTS["B"]), kkt_solver=kind)
    kd.update_data(P=dev(Pt), A=dev(B.A), G=dev(B.G), x_b_scaling=dev(B.xbs))
    flags = (np.arange(batch) % 2).astype(np.int32)
    (rho, delta, v), rhs, lhs_mul = B.state(rng), B.normal(rng), B.normal(rng)
    dv, drhs, dmul = ({nm: dev(a) for nm, a in d.items()} for d in (v, rhs, lhs_mul))
    drho, ddelta, dflags = dev(rho), dev(delta), torch.from_numpy(flags).cuda()
    outs = {(what, nm): carved(B.shapes[nm], None) for what in ("solve", "mul") for nm in NAMES}
    view = lambda what: {nm: outs[what, nm][0] for nm in NAMES}
    torch.cuda.synchronize()
    c0 = L.pq_debug_alloc_count()
    assert kh.update_scalings_and_factor(flags, rho, delta, v) == batch
    ref = {"solve": kh.solve(rhs), "mul": kh.mul(lhs_mul)}
    info = kh.solve_ok(), kh.refine_steps(), kh.backend_solves(), kh.refine_error(), kh.rhs_norm()
    assert (info[1][flags == 1].any() or p + m == 0) and not info[1][flags == 0].any()  # (without A and G the first solve is exact to a rounding: no step)
    c1 = L.pq_debug_alloc_count()
    assert kd.update_scalings_and_factor(dflags, drho, ddelta, dv) == batch
    kd.solve(drhs, out=view("solve"))
    kd.mul(dmul, out=view("mul"))
    dinfo = kd.solve_ok(), kd.refine_steps(), kd.backend_solves(), kd.refine_error(), kd.rhs_norm()
    c2 = L.pq_debug_alloc_count()
    assert c0 == c1 == c2, (c0, c1, c2)
    assert all(same(a, b) if a.dtype == np.float64 else np.array_equal(a, b) for a, b in zip(info, dinfo))
    for (what, nm), (vw, whole, before) in outs.items():
        used = B.used[nm]
        assert same(vw.cpu().numpy()[:, :used], ref[what][nm][:, :used]), (what, nm)
        if used < B.shapes[nm][1]:  # the rest of a box row is not written
            assert same(vw.cpu().numpy()[:, used:], before[5:-5].reshape(B.shapes[nm])[:, used:]), (what, nm, "behind the meaningful part")
        after, pad = whole.cpu().numpy(), 5
        assert same(after[:pad], before[:pad]) and same(after[-pad:], before[-pad:]), (what, nm, "the doubles around the output")
    assert same(kd.x_reg(), kh.x_reg()) and same(kd.z_reg(), kh.z_reg()) and same(kd.rhs_x_bar(), kh.rhs_x_bar()) and same(kd.rhs_z_bar(), kh.rhs_z_bar())
    for i in range(batch):
        assert same(lower(kd.backend().internal_factor(i)), lower(kh.backend().internal_factor(i))), i


# ---- 5. a launch wider than the chip
@pytest.mark.parametrize("n", [8, 40])
@pytest.mark.parametrize("kind", KINDS)
def test_a_launch_wider_than_the_chip(hip, orc, kind, n):
    B = sys_of(orc, n, 2, 6, 1031)
    rng = np.random.default_rng([B.seed, kind, 5])
    R = step(B.handle(hip, kind, "B"), B.oracles(orc, kind, "B"), B, 1, rng, (n, "wide"))
    assert len(set(R["steps"])) >= 2


# ---- 6. the same call twice gives the same bits
@pytest.mark.parametrize("kind", KINDS)
def test_the_same_call_gives_the_same_bits(hip, orc, kind):
    B = sys_of(orc, 33, 7, 5, 9)
    rng = np.random.default_rng([B.seed, kind, 6])
    k = B.handle(hip, kind, "B")
    (rho, delta, v), rhs, lhs_mul = B.state(rng), B.normal(rng), B.normal(rng)
    flags = (np.arange(9) % 2).astype(np.int32)
    runs = []
    for _ in range(3):
        assert k.update_scalings_and_factor(flags, rho, delta, v) == 9
        got, mul = k.solve(rhs), k.mul(lhs_mul)
        runs.append([k.backend().internal_factor(i) for i in range(9)] + [k.x_reg(), k.z_reg(), k.rhs_x_bar(), k.rhs_z_bar(), k.refine_steps().astype(np.float64),
                                                                         k.refine_error(), k.rhs_norm()] + [got[nm] for nm in NAMES] + [mul[nm] for nm in NAMES])
    for r in runs[1:]:
        assert all(same(a, b) for a, b in zip(r, runs[0]))
    fac_ms, solve_ms, mul_ms = k.last_ms()
    assert fac_ms > 0 and solve_ms > 0 and mul_ms > 0
