"""CPU checks of tests/csc_shapes.py, the shapes and the plain reference that tests/test_csc_ops_gpu.py holds the CSC mat-vec kernels to bit for bit:
every branch of the wave-cooperative column dot is reached under each kernel that instantiates it, the reference in reference-order mode IS the oracle's mat-vecs,
and the order of a sum shows in the bits of these data (otherwise a bitwise test of the order would be empty)."""
import numpy as np
import pytest
import scipy.sparse as sp

import csc_shapes as cs

SHAPES = [s.name for s in cs.all_shapes()]


def test_every_branch_is_reached_under_every_kernel():
    hit = {k: {} for k in cs.KERNEL_COPIES}
    for sh in cs.all_shapes():
        c = sh.copies()
        for kern, names in cs.KERNEL_COPIES.items():
            for nm in names:
                ncols, cp = c[nm][0], c[nm][1]
                if kern == "k_recover_duals" and ncols == 0:
                    continue  # (that half of the grid has no blocks)
                for b in cs.branches_of(ncols, cp):
                    hit[kern].setdefault(b, []).append(f"{sh.name}:{nm}")
    for kern in cs.KERNEL_COPIES:
        for b in cs.BRANCHES:
            print(f"{kern:22s} {b:32s} {', '.join(hit[kern].get(b, [])[:4])}")
    missing = [(k, b) for k in cs.KERNEL_COPIES for b in cs.BRANCHES if not hit[k].get(b)]
    assert not missing, missing


def test_profiles_are_what_they_claim():
    """the columns each profile is named after sit where the docstrings say"""
    st = cs.shape("straddle").copies()
    for nm in ("GT", "A"):
        cp = st[nm][1]
        assert cp[63] - cp[0] == 509 and cp[64] - cp[63] == 7                    # starts at entry 509 of the wave's range, 7 entries
        assert cp[65] - cp[64] == 512 and (cp[64] - cp[64]) % cs.DOT_CHUNK == 0  # 512 entries from a chunk boundary (the wave's first column)
        lo, hi = cp[67] - cp[64], cp[68] - cp[64]
        assert hi - lo == 1300 and lo % cs.DOT_CHUNK != 0 and (hi - 1) // cs.DOT_CHUNK - lo // cs.DOT_CHUNK + 1 == 3
    lg = cs.shape("long").copies()
    for nm in ("GT", "A"):
        cp = lg[nm][1]
        assert [cp[j + 1] - cp[j] for j in (0, 10, 20, 30, 63)] == [2600, 2048, 2049, 2304, 2305]
        assert all(0 < cp[j + 1] - cp[j] <= 6 for j in range(70) if j not in (0, 10, 20, 30, 63))
    assert max(np.diff(lg["Pf"][1])) > cs.SPMV_LONG_COL       # the arrow column of P
    fc = cs.shape("full_chunk_64").copies()
    assert fc["GT"][1][64] == cs.DOT_CHUNK and fc["A"][1][64] == cs.DOT_CHUNK
    e = cs.shape("edges_321").copies()
    for nm in ("GT", "A"):
        ln = np.diff(e[nm][1])
        assert not ln[[0, 63, 64, 320]].any() and not ln[128:192].any() and ln[:128].any() and ln[192:].any()
    for sh in cs.all_shapes():  # rows ascending and distinct in every column of AT and GT
        for cp, ri, _ in (sh.AT, sh.GT):
            for j in range(len(cp) - 1):
                assert (np.diff(ri[cp[j]:cp[j + 1]]) > 0).all()
    assert max(cs.shape("long").n, cs.shape("long").p) < 3000 and sum(len(M[2]) for M in (cs.shape("long").P, cs.shape("long").AT, cs.shape("long").GT)) < 50000


def oracle_kkt(orc, sh, second=False):
    """(data, KKT) of the oracle for a shape; asserts that the oracle holds the very arrays of the shape"""
    P, AT, GT = sh.with_values(second)
    n, p, m = sh.n, sh.p, sh.m
    mat = lambda M, cols: sp.csc_matrix((M[2], M[1], M[0]), shape=(n, cols))
    A = mat(AT, p).T.tocsc() if p else None
    G = mat(GT, m).T.tocsc() if m else None
    od = orc.Data.sparse(mat(P, n), np.zeros(n), A, np.zeros(p) if p else None, G, -np.ones(m) if m else None, np.ones(m) if m else None)
    for nm, M in (("P_utri", P), ("AT", AT), ("GT", GT)):
        o = od.csc(nm)
        assert np.array_equal(o.indptr, M[0]) and np.array_equal(o.indices, M[1]) and np.array_equal(cs.bits(o.data), cs.bits(M[2])), nm
    return od, orc.KKT(od, kind="sparse", mode=0)


def oracle_evals(orc, sh, second=False, k=0):
    """the three eval_* of the oracle on operand vectors k (no factorisation is needed for them)"""
    od, ko = oracle_kkt(orc, sh, second)
    an, at = cs.ALPHAS
    return ko.eval_P_x(an, sh.xs[k]), ko.eval_A_xn_and_AT_xt(an, at, sh.xs[k], sh.ys[k]), ko.eval_G_xn_and_GT_xt(an, at, sh.xs[k], sh.zs[k])


@pytest.mark.parametrize("name", [s.name for s in cs.all_shapes() if s.oracle])
def test_reference_order_reference_is_the_oracle_bitwise(orc, name):
    sh = cs.shape(name)
    for second, k in ((False, 0), (False, 1), (True, 2)):
        oP, (oAn, oAt), (oGn, oGt) = oracle_evals(orc, sh, second, k)
        rP, (rAn, rAt), (rGn, rGt) = cs.evals(sh, True, second, k=k)
        for nm, o, r in (("P x", oP, rP), ("A x", oAn, rAn), ("A' y", oAt, rAt), ("G x", oGn, rGn), ("G' z", oGt, rGt)):
            assert np.array_equal(cs.bits(o), cs.bits(r)), (name, second, nm, int((cs.bits(o) != cs.bits(r)).sum()))


@pytest.mark.parametrize("name", SHAPES)
def test_summation_order_shows_in_the_bits(name):
    """every column summed right to left: per product and in both modes, at least half of the outputs whose column has 3 or more entries change in some bit under
    one of the N_VEC operand vectors the GPU test runs.  (Under a single vector only 20 to 50 % of sums of 3 to 6 terms change when reversed, whatever the seed.)"""
    sh = cs.shape(name)
    c = sh.copies()
    flat = lambda e: (e[0], e[1][0], e[1][1], e[2][0], e[2][1])
    for ref_order in (False, True):
        diff = [np.zeros(c[nm][0], bool) for nm in ("Pf", "AT", "A", "GT", "G")]
        for k in range(cs.N_VEC):
            for d, f, b in zip(diff, flat(cs.evals(sh, ref_order, k=k)), flat(cs.evals(sh, ref_order, reverse=True, k=k))):
                d |= cs.bits(f) != cs.bits(b)
        for nm, d in zip(("Pf", "AT", "A", "GT", "G"), diff):
            rows = np.nonzero(np.diff(c[nm][1]) >= 3)[0]
            if rows.size == 0:
                continue
            changed = int(d[rows].sum())
            print(f"{name} {nm} ref_order={ref_order}: {changed} of {rows.size} rows change")
            assert 2 * changed >= rows.size, (name, nm, ref_order, changed, rows.size)


def test_tree_sum_is_not_the_sequential_sum():
    """the long columns: the strided-plus-tree value and the left-to-right value of the same column differ in bits, so the test of the default mode tells them apart"""
    sh = cs.shape("long")
    GT = sh.copies()["GT"]
    x = [float(a) for a in sh.x]
    for j in (0, 20, 30, 63):
        assert cs.col_tree(GT, j, x) != cs.col_dot(GT, j, x), j
