"""The batched dense KKT backend (piqp_amd/csrc/dense_kkt_batch.hip, pq_kkt_batch_*, piqp_amd.BatchDenseKKT; n <= 128): every instance of a batch is compared with
its own CPU oracle, orc.KKT(data, kind="dense", use_ldlt=...) (oracle/orc_dense.c), on the raw doubles.  There is no tolerance in this file and no instance is left
out: equality is np.array_equal on the uint64 views, as in tests/test_dense_exact_gpu.py, whose matrices (random_qp) and scalings (check_members) these are.  The
handle is fed the oracle's own P_utri / AT / GT, so both sides see the same doubles."""
import numpy as np
import pytest

from test_dense_exact_gpu import bits, lower, random_qp, same

pytestmark = pytest.mark.gpu

LLT, LDLT = 0, 16
PQ_ERR_INVALID = -1
KINDS = [pytest.param(LLT, id="llt"), pytest.param(LDLT, id="ldlt")]


class Batch:
    """`batch` random QPs of one shape, each with data of its own, and the oracle's view of them"""

    def __init__(self, orc, n, p, m, batch, seed, edit=None):
        self.n, self.p, self.m, self.batch = n, p, m, batch
        self.q = [random_qp(n, p, m, seed=seed * 100003 + i)[0] for i in range(batch)]
        if edit:
            edit(self.q)
        self.od = [orc.Data.dense(**q) for q in self.q]
        # the oracle's own doubles: P[i] as written (upper triangle; the other one is zero), A[i] = AT[i]', G[i] = GT[i]'
        self.P = np.stack([np.array(od.mat("P_utri")) for od in self.od])
        self.A = np.stack([np.array(od.mat("AT")).T for od in self.od]) if p else None
        self.G = np.stack([np.array(od.mat("GT")).T for od in self.od]) if m else None

    def handle(self, hip, kind):
        return hip.BatchDenseKKT(self.P, self.A, self.G, kkt_solver=kind)

    def oracles(self, orc, kind):
        return [orc.KKT(od, use_ldlt=kind == LDLT) for od in self.od]


_cache = {}


def batch_of(orc, n, p, m, batch, seed):
    key = (n, p, m, batch, seed)
    if key not in _cache:
        _cache[key] = Batch(orc, n, p, m, batch, seed)
    return _cache[key]


def scalings(rng, batch, n, m, z_lo=-6, z_hi=3):
    return 10.0 ** rng.uniform(-9, -3, batch), 10.0 ** rng.uniform(-9, -3, (batch, n)), 10.0 ** rng.uniform(z_lo, z_hi, (batch, m))


def check_factor(k, kos, sc, tag, matrices=True):
    """factorisation of every instance against its oracle; returns the oracle's flags"""
    delta, x_reg, z_reg = sc
    n_ok = k.update_scalings_and_factor(delta, x_reg, z_reg)
    flags = np.array([ko.update_scalings_and_factor(float(delta[i]), x_reg[i], z_reg[i]) for i, ko in enumerate(kos)])
    assert n_ok == flags.sum(), (tag, n_ok, flags)
    assert np.array_equal(k.ok(), flags), (tag, k.ok(), flags)
    bad = []
    for i, ko in enumerate(kos):
        if not flags[i]:
            continue
        if matrices and not same(lower(k.internal_kkt_mat(i)), lower(ko.internal_kkt_mat())):
            bad.append((i, "kkt_mat"))
        if not same(lower(k.internal_factor(i)), lower(ko.internal_factor())):
            bad.append((i, "factor"))
    assert not bad, (tag, bad)
    return flags


def check_solve(k, kos, flags, rng, tag):
    b, n, p, m = k.batch, k.n, k.p, k.m
    rx, ry, rz = rng.standard_normal((b, n)), rng.standard_normal((b, p)), rng.standard_normal((b, m))
    got = k.solve(rx, ry, rz)
    bad = []
    for i, ko in enumerate(kos):
        if flags[i]:
            bad += [(i, what) for g, ref, what in zip(got, ko.solve(rx[i], ry[i], rz[i]), ("lhs_x", "lhs_y", "lhs_z")) if not same(g[i], ref)]
    assert not bad, (tag, "solve", bad)
    return rx, ry, rz


def check_members(k, kos, rng, tag):
    """assembly, factor, solve and the three mat-vecs of every instance, each with scalings, right-hand sides and alphas of its own"""
    b, n, m = k.batch, k.n, k.m
    flags = check_factor(k, kos, scalings(rng, b, n, m), tag)
    assert flags.all(), (tag, flags)
    rx, ry, rz = check_solve(k, kos, flags, rng, tag)
    alpha, an, at = rng.standard_normal((3, b))
    zP = k.eval_P_x(alpha, rx)
    zA, zG = k.eval_A_xn_and_AT_xt(an, at, rx, ry), k.eval_G_xn_and_GT_xt(an, at, rx, rz)
    bad = []
    for i, ko in enumerate(kos):
        if not same(zP[i], ko.eval_P_x(float(alpha[i]), rx[i])):
            bad.append((i, "eval_P_x"))
        for g, ref, what in zip(zA, ko.eval_A_xn_and_AT_xt(float(an[i]), float(at[i]), rx[i], ry[i]), ("A zn", "A zt")):
            if not same(g[i], ref):
                bad.append((i, what))
        for g, ref, what in zip(zG, ko.eval_G_xn_and_GT_xt(float(an[i]), float(at[i]), rx[i], rz[i]), ("G zn", "G zt")):
            if not same(g[i], ref):
                bad.append((i, what))
    assert not bad, (tag, bad)


# n crosses the one-wave / workgroup switch at 32 and the panel widths 8 and 16 of block_size_rule with ragged last panels, up to the LDS maximum; (p, m): absent
# blocks, and m crossing the K block of 256 by one and by 44; batch 67 below n = 32 leaves the last workgroup with three of its four waves busy
@pytest.mark.parametrize("n", [1, 4, 31, 32, 33, 64, 100, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_every_member_is_bitwise_the_oracle_s(hip, orc, kind, n):
    batch = 67 if n < 32 else 9
    for p, m in ((0, 0), (7, 0), (3, 5), (0, 300), (40, 257)):
        B = batch_of(orc, n, p, m, batch, seed=1000 * n + 10 * p + m)
        rng = np.random.default_rng(7 * n + p + m + kind)
        k, kos = B.handle(hip, kind), B.oracles(orc, kind)
        assert (k.batch, k.n, k.p, k.m) == (batch, n, p, m)
        check_members(k, kos, rng, (n, p, m))
        check_members(k, kos, rng, (n, p, m, "second factorisation on the same handle"))
        check_members(k.clone(), kos, rng, (n, p, m, "clone"))


@pytest.mark.parametrize("n", [8, 40])
@pytest.mark.parametrize("kind", KINDS)
def test_a_launch_wider_than_the_chip(hip, orc, kind, n):
    B = batch_of(orc, n, 2, 6, 1031, seed=n)
    rng = np.random.default_rng(n + kind)
    k, kos = B.handle(hip, kind), B.oracles(orc, kind)
    flags = check_factor(k, kos, scalings(rng, 1031, n, 6), (n, "wide"), matrices=False)
    assert flags.all()
    check_solve(k, kos, flags, rng, (n, "wide"))


def patterned(shape, seed):
    return np.random.default_rng(seed).integers(1, 1 << 62, size=shape, dtype=np.uint64).view(np.float64)


def test_an_llt_failure_stays_in_its_instance(hip, orc):
    import torch
    n, m, batch, cols = 33, 5, 9, {2: 3, 7: 20}

    def spoil(qs):
        for i, c in cols.items():
            qs[i]["P"][c, c] = -1e6  # the leading c x c block stays definite: c is the first pivot that is not positive
    B = Batch(orc, n, 0, m, batch, seed=31, edit=spoil)
    rng = np.random.default_rng(5)
    k, kos = B.handle(hip, LLT), B.oracles(orc, LLT)
    sc = scalings(rng, batch, n, m, z_lo=-1, z_hi=1)
    assert k.update_scalings_and_factor(*sc) == 7
    flags = check_factor(k, kos, sc, "spoiled")
    assert [i for i in range(batch) if not flags[i]] == [2, 7]
    assert np.array_equal(k.first_bad_col(), [cols.get(i, -1) for i in range(batch)])
    check_solve(k, kos, flags, rng, "spoiled")
    # the blocks of the failed instances keep the bit pattern they held before the call, in host and in device memory
    rhs = rng.standard_normal((batch, n)), np.zeros((batch, 0)), rng.standard_normal((batch, m))
    before = [patterned((batch, n), 1), patterned((batch, 0), 2), patterned((batch, m), 3)]
    out = [a.copy() for a in before]
    k.solve(*rhs, out=out)
    dout = [torch.from_numpy(a.copy()).cuda() for a in before]
    k.solve(*[torch.from_numpy(a).cuda() for a in rhs], out=dout)
    for i in range(batch):
        for o, d, b0 in zip(out, dout, before):
            assert same(o[i], d[i].cpu().numpy())
            assert same(o[i], b0[i]) == (i in cols) or b0.shape[1] == 0, i
    # repaired: all nine are the oracle's again
    R = Batch(orc, n, 0, m, batch, seed=31)
    k.update_data(P=R.P)
    check_members(k, R.oracles(orc, LLT), rng, "repaired")


def test_an_ldlt_failure_is_an_exact_zero_pivot_only(hip, orc):
    def zero(qs):
        qs[3]["P"][0, 0] = 0.0
    B = Batch(orc, 1, 0, 0, 5, seed=77, edit=zero)
    k, kos = B.handle(hip, LDLT), B.oracles(orc, LDLT)
    delta, x_reg, z_reg = scalings(np.random.default_rng(1), 5, 1, 0)
    x_reg[3, 0] = 0.0
    flags = check_factor(k, kos, (delta, x_reg, z_reg), "zero pivot")
    assert list(flags) == [True, True, True, False, True]
    assert list(k.first_bad_col()) == [-1, -1, -1, 0, -1]

    def indefinite(qs):
        for i, q in enumerate(qs):
            d = np.arange(33)
            q["P"][d[i % 3::3], d[i % 3::3]] *= -1.0
    B = Batch(orc, 33, 0, 0, 9, seed=78, edit=indefinite)
    assert all(np.linalg.eigvalsh(q["P"]).min() < 0 for q in B.q)
    check_members(B.handle(hip, LDLT), B.oracles(orc, LDLT), np.random.default_rng(2), "indefinite")


@pytest.mark.parametrize("flags", [1, 2, 4, 7], ids=["P", "A", "G", "PAG"])
def test_update_data_flag_by_flag(hip, orc, flags):
    n, p, m, batch = 33, 7, 5, 9
    B1, B2 = batch_of(orc, n, p, m, batch, seed=5), batch_of(orc, n, p, m, batch, seed=6)
    k = B1.handle(hip, LLT)
    check_members(k, B1.oracles(orc, LLT), np.random.default_rng(3), "before")
    take = lambda bit, name: getattr(B2 if flags & bit else B1, name)
    k.update_data(P=B2.P if flags & 1 else None, A=B2.A if flags & 2 else None, G=B2.G if flags & 4 else None)
    M = Batch.__new__(Batch)
    M.n, M.p, M.m, M.batch = n, p, m, batch
    M.P, M.A, M.G = take(1, "P"), take(2, "A"), take(4, "G")
    M.od = [orc.Data.dense(**dict(B1.q[i], P=(B2 if flags & 1 else B1).q[i]["P"], A=(B2 if flags & 2 else B1).q[i]["A"], G=(B2 if flags & 4 else B1).q[i]["G"]))
            for i in range(batch)]
    check_members(k, M.oracles(orc, LLT), np.random.default_rng(9), ("updated handle against a fresh oracle", flags))
    check_members(M.handle(hip, LLT), M.oracles(orc, LLT), np.random.default_rng(9), ("fresh handle", flags))


def test_a_flagged_null_matrix_is_refused_and_the_handle_stays(hip, orc):
    n, p, m, batch = 33, 7, 5, 9
    B = batch_of(orc, n, p, m, batch, seed=5)
    k, L = B.handle(hip, LLT), hip._lib.load()
    ptr = B.P.ctypes.data  # (never read: the call is refused before anything is copied)
    for options, args in ((1, (None, ptr, ptr)), (2, (ptr, None, ptr)), (4, (ptr, ptr, None)), (7, (ptr, None, ptr))):
        assert L.pq_kkt_batch_update_data_dense(k.h, *args, options, 0) == PQ_ERR_INVALID
        assert L.pq_last_error_string().decode() != ""
    assert L.pq_kkt_batch_update_data_dense(k.h, None, None, None, 0, 0) == 0  # unflagged matrices are ignored and may be null
    check_members(k, B.oracles(orc, LLT), np.random.default_rng(4), "after the refused updates")


def carved(shape, device_like, pad=5):
    """a contiguous tensor of `shape` in the middle of a larger one filled with a pattern; returns (view, whole, copy of the whole before)"""
    import torch
    size = int(np.prod(shape))
    whole = torch.from_numpy(patterned(size + 2 * pad, size + 11).copy()).cuda()
    return whole[pad:pad + size].view(*shape), whole, whole.cpu().numpy().copy()


@pytest.mark.parametrize("n,p,m,batch", [(8, 2, 6, 67), (33, 7, 5, 9), (64, 0, 0, 9)])
@pytest.mark.parametrize("kind", KINDS)
def test_device_memory_equals_host_memory(hip, orc, kind, n, p, m, batch):
    import torch
    L = hip._lib.load()
    B = batch_of(orc, n, p, m, batch, seed=5 if (n, p, m) == (33, 7, 5) else 40 + n)
    rng = np.random.default_rng(n)
    kh = B.handle(hip, kind)
    # the column-major P_utri[i] is the C-contiguous transpose of P[i] as written; its unread triangle -- above the diagonal of that transpose -- is all NaN
    Pt = np.ascontiguousarray(B.P.transpose(0, 2, 1))
    Pt[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = np.nan
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kd = hip.BatchDenseKKT(dev(Pt), dev(B.A), dev(B.G), kkt_solver=kind)
    kd.update_data(P=dev(Pt), A=dev(B.A), G=dev(B.G))
    sc = scalings(rng, batch, n, m)
    rx, ry, rz = rng.standard_normal((batch, n)), rng.standard_normal((batch, p)), rng.standard_normal((batch, m))
    alpha, an, at = rng.standard_normal((3, batch))
    dsc, drhs, dal = [dev(a) for a in sc], [dev(a) for a in (rx, ry, rz)], [dev(a) for a in (alpha, an, at)]
    outs = {name: carved(shape, None) for name, shape in (("lx", (batch, n)), ("ly", (batch, p)), ("lz", (batch, m)), ("zP", (batch, n)), ("Azn", (batch, p)),
                                                          ("Azt", (batch, n)), ("Gzn", (batch, m)), ("Gzt", (batch, n)))}
    view = lambda name: outs[name][0]
    torch.cuda.synchronize()
    c0 = L.pq_debug_alloc_count()
    assert kh.update_scalings_and_factor(*sc) == batch
    ref = list(kh.solve(rx, ry, rz)) + [kh.eval_P_x(alpha, rx)] + list(kh.eval_A_xn_and_AT_xt(an, at, rx, ry)) + list(kh.eval_G_xn_and_GT_xt(an, at, rx, rz))
    c1 = L.pq_debug_alloc_count()
    assert kd.update_scalings_and_factor(*dsc) == batch
    kd.solve(*drhs, out=[view("lx"), view("ly"), view("lz")])
    kd.eval_P_x(dal[0], drhs[0], out=view("zP"))
    kd.eval_A_xn_and_AT_xt(dal[1], dal[2], drhs[0], drhs[1], out=(view("Azn"), view("Azt")))
    kd.eval_G_xn_and_GT_xt(dal[1], dal[2], drhs[0], drhs[2], out=(view("Gzn"), view("Gzt")))
    c2 = L.pq_debug_alloc_count()
    assert c0 == c1 == c2, (c0, c1, c2)
    for name, r in zip(("lx", "ly", "lz", "zP", "Azn", "Azt", "Gzn", "Gzt"), ref):
        v, whole, before = outs[name]
        assert same(v.cpu().numpy(), r), name
        after, pad = whole.cpu().numpy(), 5
        assert same(after[:pad], before[:pad]) and same(after[-pad:], before[-pad:]), (name, "the doubles around the output")
    for i in range(batch):
        assert same(lower(kd.internal_factor(i)), lower(kh.internal_factor(i))) and same(lower(kd.internal_kkt_mat(i)), lower(kh.internal_kkt_mat(i))), i


@pytest.mark.parametrize("kind", KINDS)
def test_the_same_call_gives_the_same_bits(hip, orc, kind):
    B = batch_of(orc, 33, 7, 5, 9, seed=5)
    rng = np.random.default_rng(8)
    k = B.handle(hip, kind)
    sc = scalings(rng, 9, 33, 5)
    rhs = rng.standard_normal((9, 33)), rng.standard_normal((9, 7)), rng.standard_normal((9, 5))
    runs = []
    for _ in range(3):
        assert k.update_scalings_and_factor(*sc) == 9
        runs.append([k.internal_factor(i) for i in range(9)] + list(k.solve(*rhs)))
    for r in runs[1:]:
        assert all(same(a, b) for a, b in zip(r, runs[0]))
    fac_ms, solve_ms, wall_ms = k.last_ms()
    assert fac_ms > 0 and solve_ms > 0 and wall_ms >= fac_ms
