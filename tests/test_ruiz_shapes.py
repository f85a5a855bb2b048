"""CPU checks of tests/ruiz_shapes.py, the shapes and the reference that tests/test_ruiz_kernels_gpu.py holds the device Ruiz equilibration to bit for bit:
ruiz_reference IS the oracle's ruiz_scale_data / ruiz_unscale_data (oracle/orc_solver.c:136-256) on every shape -- after a setup, and after an update that reuses or
recomputes the scaling --, a plain scalar-loop restatement agrees with it on the small ones, the shapes take the passes and the arms they are named after, and the launch
plan reaches every workgroup count and tile edge.

Every shape is a problem the oracle accepts.  Two things the oracle does not produce by itself are put in by hand: an x_b_scaling other than 1 is written into the
oracle's unscaled Data before its setup (the oracle starts every problem at 1 and meets other values only from its second equilibration on), and the sentinel in the
strictly lower triangle of a dense P_utri is compared with the zero-triangle run of the reference (the oracle multiplies those zeros by the cost scaling; the kernels
never touch them)."""
import numpy as np
import pytest
import scipy.sparse as sp

import ruiz_shapes as rs

CASES = [(s.name, i) for s in rs.all_shapes() for i in range(len(s.instances()))]
SMALL = [(nm, i) for nm, i in CASES if rs.shape(nm).N <= 120]


# ------------------------------------------------------------------------------------------------------------------- the oracle
def oracle_data(orc, q):
    """the oracle's unscaled Data of a Problem, holding the very arrays of the Problem (asserted)"""
    n, p, m = q.n, q.p, q.m
    x_l, x_u = np.full(n, -np.inf), np.full(n, np.inf)
    x_l[q.x_l_idx], x_u[q.x_u_idx] = q.x_l, q.x_u
    h_l, h_u = q.h_l.copy(), q.h_u.copy()
    if m and not q.sparse:  # a zero column of G' with the bounds -1 / 1 is what the oracle makes of a constraint without bounds: hand it over as one
        for k in np.nonzero(~q.GT.any(axis=0))[0]:
            assert (h_l[k], h_u[k]) == (-1.0, 1.0)
            h_l[k], h_u[k] = -np.inf, np.inf
    if q.sparse:
        mat = lambda M, cols: sp.csc_matrix((M[2], M[1], M[0]), shape=(n, cols))
        A = mat(q.AT, p).T.tocsc() if p else None
        G = mat(q.GT, m).T.tocsc() if m else None
        od = orc.Data.sparse(mat(q.P, n), q.c, A, q.b if p else None, G, h_l if m else None, h_u if m else None, x_l, x_u)
    else:
        od = orc.Data.dense(q.P, q.c, q.AT.T if p else None, q.b if p else None, q.GT.T if m else None, h_l if m else None, h_u if m else None, x_l, x_u)
    od.vec("x_b_scaling")[:] = q.xbs
    bad = rs.differences(from_oracle(od, q), q)
    assert not bad, ("the oracle's unscaled data is not the shape's", bad)
    return od


def from_oracle(od, like):
    """a Problem from the oracle's Data (copies)"""
    n, p, m = od.n, od.p, od.m
    if like.sparse:
        mats = []
        for nm, M in zip(("P_utri", "AT", "GT"), (like.P, like.AT, like.GT)):
            o = od.csc(nm)
            assert np.array_equal(o.indptr, M[0]) and np.array_equal(o.indices, M[1]), nm
            mats.append((M[0], M[1], np.array(o.data, dtype=np.float64)))
    else:
        mats = [np.array(od.mat(nm), order="F") for nm in ("P_utri", "AT", "GT")]
    _, _, nxl, nxu = od.counts()
    return rs.Problem(like.sparse, n, p, m, *mats, od.vec("c").copy(), od.vec("x_b_scaling").copy(), b=od.vec("b").copy(), h_l=od.vec("h_l").copy(), h_u=od.vec("h_u").copy(),
                      x_l=od.vec("x_l")[:nxl].copy(), x_l_idx=od.idx("x_l"), x_u=od.vec("x_u")[:nxu].copy(), x_u_idx=od.idx("x_u"))


def oracle_setup(orc, q, scale_cost, max_iter, reuse):
    so = orc.Solver()
    st = so.settings
    st.preconditioner_iter, st.preconditioner_scale_cost, st.preconditioner_reuse_on_update = max_iter, int(scale_cost), int(reuse)
    st.kkt_solver = orc.SPARSE_LDLT if q.sparse else orc.DENSE_CHOLESKY
    od = oracle_data(orc, q)
    od.owned = False  # the solver takes ownership
    so.sparse = q.sparse
    assert so.L.orc_solver_setup(so.ptr, od.ptr)
    return so


def oracle_update(so, q2):
    """update of P, A and G to the matrices of q2 (the same patterns)"""
    n, p, m = q2.n, q2.p, q2.m
    if q2.sparse:
        mat = lambda M, cols: sp.csc_matrix((M[2], M[1], M[0]), shape=(n, cols))
        assert so.update(P=mat(q2.P, n), A=mat(q2.AT, p).T.tocsc() if p else None, G=mat(q2.GT, m).T.tocsc() if m else None)
    else:
        assert so.update(P=q2.P, A=q2.AT.T if p else None, G=q2.GT.T if m else None)


reference_chain = rs.chain


@pytest.mark.parametrize("name,i", CASES)
def test_reference_is_the_oracle_bitwise(orc, name, i):
    """setup = compute; update with preconditioner_reuse_on_update = 1: unscale + assign + reuse; with 0: unscale + assign + compute.  Every exposed array, bit for bit
    (the oracle hands out its data, not its scalings: delta, delta_b and c show in the tail, in x_b_scaling and in everything the reuse multiplies with them)."""
    s = rs.shape(name)
    q, q2 = s.instances()[i], s.seconds()[i]
    ref = reference_chain(name, i)
    for reuse, key in ((1, "reuse"), (0, "recompute")):
        so = oracle_setup(orc, q, s.scale_cost, s.max_iter, reuse)
        if reuse:
            bad = rs.differences(ref["compute"][0], from_oracle(so.data(), q))
            assert not bad, (name, i, "setup", bad)
        oracle_update(so, q2)
        bad = rs.differences(ref[key][0], from_oracle(so.data(), q))
        assert not bad, (name, i, "update with reuse_on_update = %d" % reuse, bad)


@pytest.mark.parametrize("name,i", SMALL)
def test_reference_is_the_plain_restatement_bitwise(name, i):
    """the vectorised reference against scalar loops: every mode, the scalings included (which the oracle does not hand out), with the sentinel triangle in place"""
    s = rs.shape(name)
    q = s.instances()[i].with_sentinel_triangle()
    ref = reference_chain(name, i)
    r0, s0, passes, _ = rs.ruiz_reference(q, "compute", s.scale_cost, s.max_iter)
    n0, t0, npasses = rs.ruiz_naive(q, "compute", s.scale_cost, s.max_iter)
    assert passes == npasses == ref["passes"]
    assert not rs.differences(n0, r0, t0, s0), (name, "compute")
    for mode in ("unscale", "reuse"):
        r1, s1, _, _ = rs.ruiz_reference(r0, mode, scal=s0)
        n1, t1, _ = rs.ruiz_naive(r0, mode, scal=s0)
        assert not rs.differences(n1, r1, t1, s1), (name, mode)


@pytest.mark.parametrize("name", [s.name for s in rs.all_shapes() if s.kind == "dense"])
def test_sentinel_triangle_is_neither_read_nor_written(name):
    """the run with the sentinel below the diagonal is the zero-triangle run (the one held to the oracle) on and above the diagonal and in every vector; below it the
    sentinel comes back"""
    s = rs.shape(name)
    q = s.instances()[0]
    ref = reference_chain(name, 0)
    r0, s0, passes, _ = rs.ruiz_reference(q.with_sentinel_triangle(), "compute", s.scale_cost, s.max_iter)
    lower = np.tril_indices(q.n, -1)
    assert (rs.bits(r0.P[lower]) == rs.SENTINEL_BITS).all() and passes == ref["passes"]
    z = r0.copy()
    z.P[lower] = 0.0
    assert not rs.differences(z, ref["compute"][0], s0, ref["compute"][1])
    for mode in ("unscale", "reuse"):
        r1, _, _, _ = rs.ruiz_reference(r0, mode, scal=s0)
        assert (rs.bits(r1.P[lower]) == rs.SENTINEL_BITS).all()
        w, _, _, _ = rs.ruiz_reference(ref["compute"][0], mode, scal=s0)
        r1.P[lower] = 0.0
        assert not rs.differences(r1, w)


# ------------------------------------------------------------------------------------------------------------------- what the shapes claim
def test_pass_counts():
    seen = set()
    for s in rs.all_shapes():
        counts = [reference_chain(s.name, i)["passes"] for i in range(len(s.instances()))]
        print(f"{s.name:22s} passes {counts}")
        if s.passes is not None:
            for c in counts:
                assert {"0": c == 0, "1": c == 1, "mid": 2 <= c <= 9, "10": c == 10}[s.passes], (s.name, counts)
                seen.add((s.kind, s.passes))
        if s.kind == "batch" and len(counts) > 1:
            assert len(set(counts)) == len(counts), (s.name, "the instances of a batch must leave the loop at different passes", counts)
            assert min(counts) == 1 and max(counts) == 10 and any(2 <= c <= 9 for c in counts), (s.name, counts)
    assert {("dense", k) for k in ("0", "1", "mid", "10")} <= seen and {("sparse", k) for k in ("1", "mid", "10")} <= seen
    assert reference_chain("s_N600_iter65", 0)["passes"] > 10  # (the limit of 65 is not what ends it: more than the 10 of every other shape)
    for nm in ("d_conv_mid", "s_N1025_conv_mid"):  # an extra pass after convergence would show: the pass after the last one does not multiply by 1.0 everywhere
        s = rs.shape(nm)
        q = s.instances()[0]
        k = reference_chain(nm, 0)["passes"]
        short, _, _, _ = rs.ruiz_reference(q, "compute", s.scale_cost, k - 1)
        assert rs.differences(short, reference_chain(nm, 0)["compute"][0]), nm


def test_every_arm_of_limit_scaling_is_taken():
    """by the vector scalings: below 1e-4 (-> 1), above 1e4 (-> 1e4), between; by the cost scaling: the mean column norm in all three, the maximum with |c|_inf in the
    upper two (it cannot fall below 1e-4: the first clamp has raised it to at least that)"""
    hit = dict(vec={}, gamma1={}, gamma2={})
    wins = loses = 0
    for s in rs.all_shapes():
        for i in range(len(s.instances())):
            st = reference_chain(s.name, i)["stats"]
            for k in hit:
                for a in st[k]:
                    hit[k].setdefault(a, []).append(s.name)
            wins += st["xb_wins"]; loses += st["xb_loses"]
            if s.kind == "dense" and s.name.startswith("d_n") and s.instances()[0].n >= 4 and s.max_iter:
                assert st["vec"] == {"low", "mid", "high"}, (s.name, st["vec"])
    for k, arms in hit.items():
        print(k, {a: v[:3] for a, v in arms.items()})
    assert set(hit["vec"]) == {"low", "mid", "high"} and set(hit["gamma1"]) == {"low", "mid", "high"} and set(hit["gamma2"]) == {"mid", "high"}
    for nm in ("k_b3_t64", "k_b3_t256"):  # per instance: middle arm | lower clamp, gamma = 1 | upper clamps
        st = [reference_chain(nm, i)["stats"] for i in range(3)]
        assert st[0]["gamma1"] == {"mid"} and st[1]["gamma1"] == {"low"} and "high" in st[2]["gamma1"] and "high" in st[2]["gamma2"]
        assert reference_chain(nm, 1)["compute"][1].c == 1.0 and reference_chain(nm, 2)["compute"][1].c < 1e-4 ** 2
    assert wins > 0 and loses > 0
    for nm in ("d_n32_m1", "d_n257_p33", "d_n513_m33", "d_conv_mid", "s_N513_m0", "s_N1025", "s_N24065", "k_b1_t1024"):  # reuse and unscale multiply by a cost scaling other than 1
        assert reference_chain(nm, 0)["compute"][1].c != 1.0, nm
    for nm in ("d_n33_p33_m32", "d_n513_m33", "s_N511", "s_N24065"):
        st = reference_chain(nm, 0)["stats"]
        assert st["xb_loses"] > 0 and (st["xb_wins"] > 0 or nm == "d_n33_p33_m32"), nm
    assert reference_chain("d_n513_m33", 0)["stats"]["xb_wins"] > 0 and reference_chain("d_n32_m1", 0)["stats"]["xb_wins"] > 0


def test_patterns_are_what_they_claim():
    for s in rs.all_shapes():
        for q in s.instances():
            assert (q.xbs > 0).all()
            if not q.sparse:
                assert not q.P[np.tril_indices(q.n, -1)].any()
                continue
            for (cp, ri, v), cols in ((q.P, q.n), (q.AT, q.p), (q.GT, q.m)):
                assert cp.size == cols + 1 and cp[0] == 0 and (np.diff(cp) >= 0).all() and (np.diff(cp) <= 4).all() and cp[-1] == ri.size == v.size
                for j in range(cols):
                    assert (np.diff(ri[cp[j]:cp[j + 1]]) > 0).all()
            cj = np.repeat(np.arange(q.n), np.diff(q.P[0]))
            assert (q.P[1] <= cj).all()
    q = rs.shape("s_N1025").instances()[0]
    cj = np.repeat(np.arange(q.n), np.diff(q.P[0]))
    assert not (q.P[1] == cj).any() and (np.diff(q.P[0]) == 0).any()          # no diagonal entry at all; empty columns
    q = rs.shape("s_N511").instances()[0]
    cj = np.repeat(np.arange(q.n), np.diff(q.P[0]))
    a = np.abs(q.P[2])
    diag = np.zeros(q.n); np.maximum.at(diag, cj[q.P[1] == cj], a[q.P[1] == cj])
    offr = np.zeros(q.n); np.maximum.at(offr, q.P[1][q.P[1] != cj], a[q.P[1] != cj])
    assert (offr > diag).sum() > q.n // 8                                      # rows whose norm comes from an entry stored in another column (the r != j arm)
    assert np.bincount(q.AT[1], minlength=q.n).max() >= q.p // 3                # one row of A' hit from a third of the columns
    assert (np.diff(q.P[0]) == 0).any()
    for nm in ("d_n33_p33_m32", "d_n255_p32_m33"):
        q = rs.shape(nm).instances()[0]
        assert not q.AT[:, 0].any() and not q.GT[:, -1].any() and q.AT[:, 1].any()
        sc = reference_chain(nm, 0)["compute"][1]
        # (a zero row or column has norm 0, below 1e-4: every pass scales it by 1 -- unless x_b_scaling decides, which it does not for a constraint)
        assert sc.delta[q.n] == 1.0 and sc.delta[q.n + q.p + q.m - 1] == 1.0
    kb = rs.shape("k_b3_t256").instances()
    assert kb[0].x_l_idx.size != kb[0].x_u_idx.size and np.unique(kb[0].x_l_idx).size == kb[0].x_l_idx.size and (np.diff(kb[0].x_l_idx) > 1).any()
    for s in rs.all_shapes():
        if s.kind == "batch":
            for q in s.instances()[1:]:
                for nm in rs.MATS:
                    assert all(np.array_equal(a, b) for a, b in zip(getattr(q, nm)[:2], getattr(s.instances()[0], nm)[:2])), s.name
                assert np.array_equal(q.x_l_idx, s.instances()[0].x_l_idx) and np.array_equal(q.x_u_idx, s.instances()[0].x_u_idx)


def test_product_order_shows_in_the_bits():
    """(v * s_i) * s_j and (v * s_j) * s_i differ for many entries of these data: a bitwise test of the order is not empty"""
    for nm in ("d_n33_p33_m32", "s_N511"):
        q = rs.shape(nm).instances()[0]
        sc = reference_chain(nm, 0)["compute"][1]
        v = q.values("P") if not q.sparse else q.P[2]
        if q.sparse:
            si, sj = sc.delta[q.P[1]], sc.delta[np.repeat(np.arange(q.n), np.diff(q.P[0]))]
        else:
            si, sj = sc.delta[:q.n, None], sc.delta[None, :q.n]
        a, b = (v * si) * sj, (v * sj) * si
        differ = int((rs.bits(a) != rs.bits(b)).sum())
        print(nm, differ, "of", a.size, "products depend on the order")
        assert differ > a.size // 20


def test_summation_order_shows_in_the_bits():
    """the mean column norm summed right to left changes the result on at least one shape of every kernel that forms it: the dense k_rzd_gamma, the sparse kernel on
    the grid, on one workgroup from the solver path, and on the kernel path with one instance and with three (where |c|_inf exceeds the mean the sum is not seen at
    all, hence the shapes with a small c)"""
    for what, nm, i in (("dense, k_rzd_gamma", "d_conv10", 0), ("dense, three row blocks", "d_n513_m33", 0), ("sparse on the grid", "s_N1025", 0),
                        ("sparse on one workgroup, solver path", "s_N512_p0_m0", 0), ("kernel path, batch 1", "k_b1_t1024", 0), ("kernel path, batch 3", "k_b3_t1024_notail", 0)):
        s = rs.shape(nm)
        assert s.scale_cost
        rev, srev, _, _ = rs.ruiz_reference(s.instances()[i], "compute", True, s.max_iter, reverse_sum=True)
        assert rs.differences(rev, reference_chain(nm, i)["compute"][0], srev, reference_chain(nm, i)["compute"][1]), (what, nm)


# ------------------------------------------------------------------------------------------------------------------- the launch plan
def test_launch_plan_reaches_every_branch():
    sparse = {s.name: rs.sparse_plan(s.N, s.max_iter) for s in rs.all_shapes() if s.kind == "sparse"}
    for k, v in sparse.items():
        print(f"{k:22s} N = {rs.shape(k).N:6d} {v}")
    assert sparse["s_N1"] == sparse["s_N511"] == sparse["s_N512_p0_m0"] == ("one_wg", 1, 1, 1024)
    assert sparse["s_N513_m0"] == ("grid", 2, 1, 256) and sparse["s_N1025"] == sparse["s_N1025_conv1"] == sparse["s_N1025_conv_mid"] == ("grid", 3, 1, 256)
    assert sparse["s_N24064"] == ("grid", 47, 1, 256) and sparse["s_N24065"] == ("grid", 48, 1, 256) and sparse["s_N30000"] == ("grid", 48, 1, 256)
    assert rs.shape("s_N30000").N == 30000 and (30000 + 511) // 512 > 48
    assert sparse["s_N600_iter65"] == ("one_wg", 1, 1, 1024) and rs.sparse_plan(600, 64) == ("grid", 2, 1, 256)
    kern = {s.name: rs.sparse_plan(s.N, s.max_iter, batch=len(s.instances()), threads=s.threads, grid_ws=False) for s in rs.all_shapes() if s.kind == "batch"}
    assert {(v[1], v[3]) for v in kern.values()} == {(3, 64), (3, 256), (3, 1024), (1, 1024)} and all(v[0] == "one_wg" for v in kern.values())
    assert rs.shape("k_b3_t64").N < 512 < rs.shape("k_b3_t256").N and rs.shape("k_b1_t1024").N > 512
    assert {s.tail for s in rs.all_shapes() if s.kind == "batch"} == {"full", "absent", "uneven"} and all(s.pad >= 0 for s in rs.all_shapes())
    dense = {s.name: (s.instances()[0], rs.dense_plan(s.instances()[0].n, s.instances()[0].p, s.instances()[0].m)) for s in rs.all_shapes() if s.kind == "dense"}
    ns = {q.n for q, _ in dense.values()}
    assert {1, 31, 32, 33, 255, 256, 257, 513} <= ns
    pm = {(q.p, q.m) for q, _ in dense.values()}
    assert {0, 1, 32, 33} <= {p for p, _ in pm} and {0, 1, 32, 33} <= {m for _, m in pm} and any(p == 0 and m > 0 for p, m in pm) and any(m == 0 and p > 0 for p, m in pm)
    assert {(s.scale_cost, s.max_iter) for s in rs.all_shapes() if s.kind == "dense"} >= {(True, 10), (False, 10), (False, 3), (True, 3), (False, 0)}
    plan = {q.n: pl for q, pl in dense.values()}
    assert plan[1][0] == plan[31][0] == plan[32][0] == ("dense", 1, 1, 256) and plan[33][0] == ("dense", 1, 2, 256) and plan[256][0] == ("dense", 1, 8, 256)
    assert plan[257][0] == ("dense", 2, 9, 256) and plan[513][0] == ("dense", 3, 17, 256)
    assert plan[256][1]["P"][2] == 0 and plan[257][1]["P"][2] == 8   # row block 1 of n = 257: tile columns 0 .. 7 end above row 256; tile column 8 is column 256 alone and is run
    assert plan[513][1]["P"][2] == 8 + 16                             # row block 2 (rows 512 ..): tile columns 0 .. 15
    assert {pl[1]["AT"][1] for pl in plan.values()} >= {1, 2} and {pl[1]["GT"][1] for pl in plan.values()} >= {1, 2}
