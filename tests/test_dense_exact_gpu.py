"""The reference-order dense backend (piqp_amd/csrc/dense_exact.hip; kkt_solver = DENSE_CHOLESKY_EXACT = 19, n <= 1024): every result is compared with the CPU
oracle's dense backend (oracle/orc_dense.c, kkt_solver = dense_cholesky) on the raw doubles.  There is no tolerance in this file: equality is np.array_equal on the
uint64 views (NaN and the sign of zero cannot hide a difference)."""
import ctypes as C

import numpy as np
import pytest

from qp_io import dense_args, load_qp
from test_mm_dense_gpu import ROUNDING_DECIDED as MM_ROUNDING_DECIDED
from test_mm_dense_gpu import dense_sweep_names
from test_solver_gpu import FIXTURES
from test_solver_gpu import ROUNDING_DECIDED as SOLVER_ROUNDING_DECIDED

pytestmark = pytest.mark.gpu

EXACT = 19
PQ_ERR_UNSUPPORTED = -3  # include/piqp_amd.h
SWEEP = dense_sweep_names()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def lower(M):
    return np.asarray(M)[np.tril_indices(np.asarray(M).shape[0])]


def random_qp(n, p, m, seed):
    """P symmetric positive definite with entries of both signs, A and G dense (no structure the order of summation could hide behind)"""
    rng = np.random.default_rng(seed)
    k = min(n, 48)
    F = rng.standard_normal((n, k))
    P = F @ F.T / k + np.diag(rng.uniform(0.5, 1.5, n))
    P = np.triu(P) + np.triu(P, 1).T
    q = dict(P=P, c=rng.standard_normal(n))
    if p:
        q.update(A=rng.standard_normal((p, n)), b=rng.standard_normal(p))
    if m:
        q.update(G=rng.standard_normal((m, n)), h_l=-rng.uniform(0.5, 2.0, m), h_u=rng.uniform(0.5, 2.0, m))
    return q, rng


def backends(hip, orc, q):
    d, od = hip.Data(**q), orc.Data.dense(**q)
    return d, od, hip.DenseKKT(d, kkt_solver=EXACT), orc.KKT(od)


def check_members(k, ko, n, p, m, rng, tag):
    """assembly, factor, solve and the three mat-vecs of one pair of handles"""
    delta = 10.0 ** rng.uniform(-9, -3)
    x_reg = 10.0 ** rng.uniform(-9, -3, n)
    z_reg = 10.0 ** rng.uniform(-6, 3, m)
    ok, oko = k.update_scalings_and_factor(delta, x_reg, z_reg), ko.update_scalings_and_factor(delta, x_reg, z_reg)
    assert ok and oko, (tag, ok, oko)
    assert same(lower(k.internal_kkt_mat()), lower(ko.internal_kkt_mat())), (tag, "kkt_mat")
    assert same(lower(k.internal_factor()), lower(ko.internal_factor())), (tag, "factor")
    rx, ry, rz = rng.standard_normal(n), rng.standard_normal(p), rng.standard_normal(m)
    for got, ref, what in zip(k.solve(rx, ry, rz), ko.solve(rx, ry, rz), ("lhs_x", "lhs_y", "lhs_z")):
        assert same(got, ref), (tag, "solve", what)
    alpha, an, at = rng.standard_normal(3)
    assert same(k.eval_P_x(alpha, rx), ko.eval_P_x(alpha, rx)), (tag, "eval_P_x")
    for got, ref, what in zip(k.eval_A_xn_and_AT_xt(an, at, rx, ry), ko.eval_A_xn_and_AT_xt(an, at, rx, ry), ("zn", "zt")):
        assert same(got, ref), (tag, "eval_A", what)
    for got, ref, what in zip(k.eval_G_xn_and_GT_xt(an, at, rx, rz), ko.eval_G_xn_and_GT_xt(an, at, rx, rz), ("zn", "zt")):
        assert same(got, ref), (tag, "eval_G", what)


# n crosses the unblocked / blocked switch at 32 and the panel widths 8, 16, 80, 112, 128 of block_size_rule with ragged last panels; p and m cross the K block of 256
@pytest.mark.parametrize("n", [4, 31, 32, 33, 100, 255, 256, 257, 640, 1000, 1024])
def test_every_member_is_bitwise_the_oracle_s(hip, orc, n):
    for p in (0, 7, 300):
        for m in (0, 5, 257, 600):
            q, rng = random_qp(n, p, m, seed=1000 * n + 10 * p + m)
            d, od, k, ko = backends(hip, orc, q)
            check_members(k, ko, n, p, m, rng, (n, p, m))
            check_members(k, ko, n, p, m, rng, (n, p, m, "second factorisation on the same handle"))
            check_members(k.clone(), ko, n, p, m, rng, (n, p, m, "clone"))


@pytest.mark.parametrize("n,p,m", [(33, 7, 5), (257, 300, 257)])
def test_update_data_equals_a_fresh_handle(hip, orc, n, p, m):
    q, rng = random_qp(n, p, m, seed=5)
    q2, _ = random_qp(n, p, m, seed=6)
    d, od, k, ko = backends(hip, orc, q)
    check_members(k, ko, n, p, m, rng, "before")
    k.update_data(hip.Data(**q2), hip.KKT_UPDATE_P | hip.KKT_UPDATE_A | hip.KKT_UPDATE_G)
    d2, od2, kf, kof = backends(hip, orc, q2)
    check_members(k, kof, n, p, m, np.random.default_rng(9), "updated handle against a fresh oracle")
    check_members(kf, kof, n, p, m, np.random.default_rng(9), "fresh handle")
    delta, x_reg, z_reg = 1e-5, np.full(n, 1e-6), np.full(m, 0.3)
    assert k.update_scalings_and_factor(delta, x_reg, z_reg) and kf.update_scalings_and_factor(delta, x_reg, z_reg)
    assert same(k.internal_factor(), kf.internal_factor())


@pytest.mark.parametrize("col", [3, 50])
def test_a_pivot_that_is_not_positive_fails_on_both_sides(hip, orc, col):
    """n = 100: panels of 8 columns.  col = 3 lies in the first panel, col = 50 in the seventh; the leading col x col block is positive definite, so col is the first
    failing pivot.  Both report 'not factored'; the columns left of the failing panel are final on both sides and equal."""
    n = 100
    q, rng = random_qp(n, 0, 0, seed=77)
    q["P"][col, col] = -1.0
    d, od, k, ko = backends(hip, orc, q)
    x_reg = np.full(n, 1e-8)
    assert not k.update_scalings_and_factor(1e-6, x_reg, np.zeros(0))
    assert not ko.update_scalings_and_factor(1e-6, x_reg, np.zeros(0))
    left = (col // 8) * 8
    Lh, Lo = k.internal_factor(), ko.internal_factor()
    for j in range(left):
        assert same(Lh[j:, j], Lo[j:, j]), j
    # and the handle recovers: the next factorisation of a definite matrix is the oracle's again
    q["P"][col, col] = 5.0
    d, od, k2, ko2 = backends(hip, orc, q)
    k.update_data(hip.Data(**q), hip.KKT_UPDATE_P)
    check_members(k, ko2, n, 0, 0, rng, "after the failure")


def test_recorded_states_of_the_hardest_fixture(hip, orc):
    """every interior-point state of the oracle's qp_robot_arm_sqp solve (the ill-conditioned matrices at the regularisation floor, where the iteration counts of the
    fast dense backend leave the oracle's): the same states factor on both sides, and factor and solve are bitwise equal on them"""
    q = load_qp("qp_robot_arm_sqp")
    so = orc.Solver(); so.settings.kkt_solver = 0
    assert so.setup(*dense_args(q))
    states = so.record_states()
    so.solve()
    od = so.data()
    n, p, m = od.n, od.p, od.m
    assert n <= 1024
    Pu, AT, GT = od.mat("P_utri").copy(), od.mat("AT").copy(), od.mat("GT").copy()

    class Scaled(hip.Data):  # the Ruiz-scaled matrices of the oracle's solve, for both backends
        def __init__(self):
            self.n, self.p, self.m = n, p, m
            self.P_utri, self.AT, self.GT = np.asfortranarray(Pu), np.asfortranarray(AT), np.asfortranarray(GT)
            self.h_l_idx, self.h_u_idx, self.x_l_idx, self.x_u_idx = od.idx("h_l"), od.idx("h_u"), od.idx("x_l"), od.idx("x_u")
            self.n_h_l, self.n_h_u, self.n_x_l, self.n_x_u = od.counts()
            self.x_b_scaling = od.vec("x_b_scaling").copy()
    kh = hip.KKTSystem(Scaled(), hip.default_settings(kkt_solver=EXACT))
    ko = orc.KKTSystem(od, orc.Settings(kkt_solver=0))
    fs = [s for s in states if s["kind"] == 0]
    ss = [s for s in states if s["kind"] == 1]
    assert len(fs) >= 18 and ss  # (the oracle's solve takes 18 iterations: at least one factorisation each)
    factored = floor_states = 0
    for it, st in enumerate(fs):
        rhs = ss[min(2 * it + 1, len(ss) - 1)]["vars"]
        okh = kh.update_scalings_and_factor(False, st["rho"], st["delta"], st["vars"])
        oko = ko.update_scalings_and_factor(False, st["rho"], st["delta"], st["vars"])
        assert okh == oko, (it, okh, oko)
        if not oko:
            continue
        factored += 1
        floor_states += st["delta"] <= 1e-10
        assert same(lower(kh.backend().internal_factor()), lower(ko.backend().internal_factor())), (it, "factor")
        (_, lh), (_, lo) = kh.solve(rhs), ko.solve(rhs)
        for key in lo:
            assert same(lh[key], lo[key]), (it, "solve", key)
    # (replayed out of their context -- no retry with a raised regularisation -- some states at the floor do not factor, on either side: okh == oko above;
    # the comparison is over every state the oracle factors, and that set is not empty and reaches the floor rho = delta = 1e-10)
    print(f"{len(fs)} recorded factorisation states, {factored} factor on both sides, the others on neither")
    assert factored > 0 and floor_states > 0, (factored, floor_states)


def _solve_pair(hip, orc, name):
    args = dense_args(load_qp(name))
    assert args[0].shape[0] <= 1024, (name, args[0].shape[0])
    sh, so = hip.DenseSolver(), orc.Solver()
    sh.settings.kkt_solver = EXACT
    so.settings.kkt_solver = 0
    sh.enable_trace(); so.enable_trace()
    assert sh.setup(*args) and so.setup(*args)
    st_h, st_o = sh.solve(), so.solve()
    print(f"{name}: status {st_h} / {st_o}, iterations {sh.info.iter} / {so.info.iter}")
    assert st_h == st_o, (name, st_h, st_o)
    assert sh.info.iter == so.info.iter, (name, sh.info.iter, so.info.iter)
    th, to = sh.trace(), so.trace()
    if not same(th, to):
        rows = min(len(th), len(to))
        bad = [r for r in range(rows) if not same(th[r], to[r])]
        assert False, (name, "trace", len(th), len(to), "first differing row", bad[0] if bad else rows, th[bad[0]] if bad else None, to[bad[0]] if bad else None)
    assert same(sh.result()["x"], so.result()["x"]), (name, "x")


def _whole_solves(hip, orc, names):
    failures = []
    for name in names:
        try:
            _solve_pair(hip, orc, name)
        except AssertionError as e:  # (every problem is run and reported, none is dropped: the test fails if any did)
            failures.append(str(e)[:400])
    assert not failures, (len(failures), failures)
    return len(names)


@pytest.mark.parametrize("host_loop", [False, True])
def test_whole_solves_of_the_dense_sweep(hip, orc, host_loop, monkeypatch):
    """all 72 problems of the reference's dense Maros-Meszaros sweep: status, iteration count, the per-iteration table and x bitwise the oracle's, with the
    device-resident interior-point loop and with the host loop -- the 15 names of tests/test_mm_dense_gpu.py::ROUNDING_DECIDED included"""
    if host_loop:
        monkeypatch.setenv("PIQP_AMD_HOST_IPM", "1")
    assert set(MM_ROUNDING_DECIDED) <= set(SWEEP)
    assert _whole_solves(hip, orc, SWEEP) == 72


@pytest.mark.parametrize("host_loop", [False, True])
def test_whole_solves_of_the_solver_fixtures(hip, orc, host_loop, monkeypatch):
    """the nine fixtures of tests/test_solver_gpu.py (qp_robot_arm_sqp of its ROUNDING_DECIDED among them; each asserted to have n <= 1024)"""
    if host_loop:
        monkeypatch.setenv("PIQP_AMD_HOST_IPM", "1")
    assert set(SOLVER_ROUNDING_DECIDED) <= set(FIXTURES)
    assert _whole_solves(hip, orc, FIXTURES) == 9


def test_sizes_above_1024_are_refused(hip):
    q, _ = random_qp(1025, 0, 0, seed=1)
    desc = hip.Data(**q).descriptor()
    h = C.c_void_p()
    L = hip._lib.load()
    assert L.pq_kkt_create_dense(C.byref(h), C.byref(desc), EXACT, 0) == PQ_ERR_UNSUPPORTED
    assert b"1024" in L.pq_last_error_string()
    s = hip.DenseSolver(); s.settings.kkt_solver = EXACT
    assert not s.setup(q["P"], q["c"])


def test_device_sqrt_is_correctly_rounded(hip):
    """the factorisation's pivots go through the device's fp64 square root: it must be IEEE's, like the host's (numpy calls the hardware instruction)"""
    rng = np.random.default_rng(2024)
    mant = rng.integers(0, 1 << 52, 300000, dtype=np.uint64)
    expo = rng.integers(1, 2047, 300000, dtype=np.uint64)  # every normal exponent
    rand = ((expo << np.uint64(52)) | mant).view(np.float64)
    sub = rng.integers(1, 1 << 52, 20000, dtype=np.uint64).view(np.float64)  # subnormals
    r = rng.integers(1, 1 << 26, 60000).astype(np.float64)
    sq = r * r  # exact squares
    near = np.concatenate([np.nextafter(sq, 0.0), np.nextafter(sq, np.inf)])
    wide = (rng.integers(1 << 26, 1 << 53, 60000).astype(np.float64)) * 2.0 ** rng.integers(-500, 500, 60000)
    x = np.ascontiguousarray(np.concatenate([rand, sub, sq, near, wide * wide, np.array([0.0, 1.0, 2.0, 4.0, np.inf, np.finfo(float).tiny, np.finfo(float).max])]))
    out = np.empty_like(x)
    L = hip._lib.load()
    assert L.pq_debug_device_sqrt(0, x.ctypes.data, out.ctypes.data, x.size) == 0, L.pq_last_error_string()
    ref = np.sqrt(x)
    bad = np.nonzero(bits(out) != bits(ref))[0]
    assert bad.size == 0, (bad.size, x[bad[:5]], out[bad[:5]], ref[bad[:5]])
