"""The CSC mat-vec kernels under every sparse backend (piqp_amd/csrc/sparse_ops.hip, CscOperators) against the plain sequential reference of tests/csc_shapes.py,
BIT FOR BIT: the file is built without FMA contraction, so every product is a documented sequence of rounded multiplies and adds and no tolerance is needed (a
contracted build, a dropped or doubled term, another association or another summation order fails here).  One operation at a time through pq_debug_csc_ops -- no
symbolic analysis, no factorisation -- on shapes that reach every branch of the wave-cooperative column dot (tests/test_csc_shapes.py lists them), in the default and
in the reference-order mode; then the same products through real handles of every sparse backend."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import csc_shapes as cs

pytestmark = pytest.mark.gpu

SHAPES = [s.name for s in cs.all_shapes()]
MODES = [False, True]  # reference-order flag
NAN_BITS = 0x7FF8000000000000


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def run(hip, sh, op, ref_order=False, init_second=False, upload_second=False, rows=((), (), ()), **kw):
    """one pq_debug_csc_ops call: (out_x, out_y, out_z, absmax_bits, result); the outputs start as SENTINEL everywhere"""
    L = hip._lib.load()
    P, AT, GT = sh.with_values(init_second)
    keep = [np.ascontiguousarray(a, dtype=t) for M in (P, AT, GT) for a, t in zip(M, (np.int32, np.int32, np.float64))]
    d = hip._lib.SparseData()
    d.n, d.p, d.m = sh.n, sh.p, sh.m
    (d.P_colptr, d.P_rowind, d.P_val, d.AT_colptr, d.AT_rowind, d.AT_val, d.GT_colptr, d.GT_rowind, d.GT_val) = (a.ctypes.data for a in keep)
    d.mem = 0  # PQ_MEM_HOST
    io = hip._lib.CscOpIO()
    if upload_second:
        v2 = [np.ascontiguousarray(v, dtype=np.float64) for v in sh.val2]
        keep += v2
        io.P_val2, io.AT_val2, io.GT_val2 = (_ptr(v) for v in v2)
    io.alpha_n, io.alpha_t = kw.pop("alphas", cs.ALPHAS)
    io.delta, io.delta_inv = sh.delta, sh.delta_inv
    io.with_A, io.with_G = int(kw.pop("with_A", True)), int(kw.pop("with_G", True))
    vec = dict(in_x=sh.x, in_y=sh.y, in_z=sh.z, rhs_x=sh.rhs_x, rhs_y=sh.rhs_y, rhs_z=sh.rhs_z, zinv=sh.zinv, x_reg=sh.x_reg, z_reg=sh.z_reg)
    vec.update(kw)
    for k, v in vec.items():
        v = np.ascontiguousarray(v, dtype=np.float64)
        keep.append(v)
        setattr(io, k, _ptr(v))
    rl = [np.ascontiguousarray(r, dtype=np.int32) for r in rows]
    io.rows_x, io.rows_y, io.rows_z = (_ptr(r) for r in rl)
    io.nx, io.ny, io.nz = (int(r.size) for r in rl)
    out = [np.full(max(k, 1), cs.SENTINEL) for k in (sh.n, sh.p, sh.m)]
    io.out_x, io.out_y, io.out_z = (o.ctypes.data for o in out)
    io.absmax_bits, io.result = 0xDEAD, -1
    hip._lib.check(L.pq_debug_csc_ops(0, C.byref(d), hip._lib.CSC_OPS.index(op), int(ref_order), C.byref(io)), "pq_debug_csc_ops " + op)
    return out[0][:sh.n], out[1][:sh.p], out[2][:sh.m], int(io.absmax_bits), int(io.result)


def same(got, want, what):
    gb, wb = cs.bits(got), cs.bits(want)
    bad = np.nonzero(gb != wb)[0]
    assert bad.size == 0, (what, f"{bad.size} of {gb.size} entries differ in bits; first at {int(bad[0])}: {float(got[bad[0]])!r} != {float(want[bad[0]])!r}")


def untouched(a, what):
    same(a, np.full(a.shape, cs.SENTINEL), what + ": must be left alone")


@functools.lru_cache(maxsize=None)
def ref_evals(name, ref_order, second, k):
    """computed once per process, shared and never written to"""
    return cs.evals(cs.shape(name), ref_order, second, k=k)


def device_evals(hip, sh, ref_order, k, **kw):
    v = dict(in_x=sh.xs[k], in_y=sh.ys[k], in_z=sh.zs[k])
    px, _, _, _, _ = run(hip, sh, "eval_P_x", ref_order, **v, **kw)
    at, an_, zleft, _, _ = run(hip, sh, "eval_A", ref_order, **v, **kw)
    untouched(zleft, "eval_A out_z")
    gt, yleft, gn, _, _ = run(hip, sh, "eval_G", ref_order, **v, **kw)
    untouched(yleft, "eval_G out_y")
    return px, (an_, at), (gn, gt)


def check_evals(got, want, what):
    same(got[0], want[0], what + " P x")
    same(got[1][0], want[1][0], what + " A x"); same(got[1][1], want[1][1], what + " A' y")
    same(got[2][0], want[2][0], what + " G x"); same(got[2][1], want[2][1], what + " G' z")


@pytest.mark.parametrize("ref_order", MODES)
@pytest.mark.parametrize("name", SHAPES)
def test_evals_bitwise_the_reference(hip, orc, name, ref_order):
    sh = cs.shape(name)
    for k in range(cs.N_VEC):
        got = device_evals(hip, sh, ref_order, k)
        check_evals(got, ref_evals(name, ref_order, False, k), f"{name} ref_order={ref_order} vectors {k}:")
        if ref_order and sh.oracle and k < 2:
            from test_csc_shapes import oracle_evals
            check_evals(got, oracle_evals(orc, sh, False, k), f"{name} against the oracle, vectors {k}:")


@pytest.mark.parametrize("ref_order", MODES)
@pytest.mark.parametrize("name", SHAPES)
def test_fold_rhs_and_recover_duals_bitwise_the_reference(hip, name, ref_order):
    sh = cs.shape(name)
    for with_A in (True, False):
        for with_G in (True, False):
            ox, oy, oz, _, _ = run(hip, sh, "fold_rhs", ref_order, with_A=with_A, with_G=with_G)
            same(ox, cs.fold_rhs(sh, with_A, with_G, ref_order), f"{name} fold_rhs with_A={with_A} with_G={with_G} ref_order={ref_order}")
            untouched(oy, "fold_rhs out_y"); untouched(oz, "fold_rhs out_z")
    ly, lz = cs.recover_duals(sh, sh.x)
    for with_A in (True, False):
        for with_G in (True, False):
            ox, oy, oz, _, _ = run(hip, sh, "recover_duals", ref_order, with_A=with_A, with_G=with_G)
            untouched(ox, "recover_duals out_x")
            if with_A:
                same(oy, ly, f"{name} recover_duals lhs_y")
            else:
                untouched(oy, "recover_duals lhs_y with the flag off")
            if with_G:
                same(oz, lz, f"{name} recover_duals lhs_z")
            else:
                untouched(oz, "recover_duals lhs_z with the flag off")


@pytest.mark.parametrize("name", SHAPES)
def test_P_diag(hip, name):
    sh = cs.shape(name)
    same(run(hip, sh, "P_diag")[0], cs.p_diag(sh), name + " P_diag")
    same(run(hip, sh, "P_diag", upload_second=True)[0], cs.p_diag(sh, second=True), name + " P_diag after upload_values")
    if name == "absent_pm_dup_diag":  # the column that lists its diagonal twice gives the LAST one; a column without one gives 0
        cp, ri, v = sh.P
        assert cs.p_diag(sh)[5] == v[cp[6] - 1] != v[cp[6] - 2] and ri[cp[6] - 2] == 5 and cs.p_diag(sh)[3] == 0.0


@pytest.mark.parametrize("ref_order", MODES)
@pytest.mark.parametrize("name", SHAPES)
def test_upload_values_equals_fresh_init(hip, name, ref_order):
    """new values through upload_values into the same pattern (the gathers into the symmetrised and the transposed copies): bitwise a fresh init with them, and the
    reference on them"""
    sh = cs.shape(name)
    up = device_evals(hip, sh, ref_order, 2, upload_second=True)
    check_evals(up, device_evals(hip, sh, ref_order, 2, init_second=True), f"{name}: upload_values against a fresh init:")
    check_evals(up, ref_evals(name, ref_order, True, 2), f"{name}: after upload_values:")
    same(run(hip, sh, "fold_rhs", ref_order, upload_second=True)[0], cs.fold_rhs(sh, True, True, ref_order, second=True), name + " fold_rhs after upload_values")
    _, oy, oz, _, _ = run(hip, sh, "recover_duals", ref_order, upload_second=True)
    ly, lz = cs.recover_duals(sh, sh.x, second=True)
    same(oy, ly, name + " recover_duals lhs_y after upload_values"); same(oz, lz, name + " recover_duals lhs_z after upload_values")


def row_lists(sh):
    """(label, rows_x, rows_y, rows_z): a random third, all rows, no rows, and lengths that put the nx | ny | nz seams inside a wave (250 | 10 | 61: seams at threads
    250 and 260) and on a block edge (256 | 64 | 1) where the shape has that many rows"""
    rng = np.random.default_rng(sh.seed + 1000)
    pick = lambda dim, cnt: rng.permutation(dim)[:cnt].astype(np.int32)
    out = [("third", pick(sh.n, (sh.n + 2) // 3), pick(sh.p, (sh.p + 2) // 3), pick(sh.m, (sh.m + 2) // 3)),
           ("all", pick(sh.n, sh.n), pick(sh.p, sh.p), pick(sh.m, sh.m)),
           ("none", pick(sh.n, 0), pick(sh.p, 0), pick(sh.m, 0))]
    for nx, ny, nz in ((250, 10, 61), (256, 64, 1)):
        if sh.n >= nx and sh.p >= ny and sh.m >= nz:
            out.append((f"{nx}|{ny}|{nz}", pick(sh.n, nx), pick(sh.p, ny), pick(sh.m, nz)))
    return out


def listed_only(got, full, rows, what):
    mask = np.zeros(got.size, bool); mask[rows] = True
    same(got[mask], full[mask], what + ": listed rows")
    untouched(got[~mask], what + ": unlisted rows")


def test_row_lists_reach_the_seams():
    labels = {lab for s in cs.all_shapes() for lab, *_ in row_lists(s)}
    assert {"250|10|61", "256|64|1"} <= labels


@pytest.mark.parametrize("ref_order", MODES)
@pytest.mark.parametrize("name", SHAPES)
def test_rows_kernels_bitwise_the_full_operations(hip, name, ref_order):
    sh = cs.shape(name)
    fold = {(a, g): cs.fold_rhs(sh, a, g, ref_order) for a in (True, False) for g in (True, False)}
    ly, lz = cs.recover_duals(sh, sh.x)
    ex, ey, ez = cs.residual(sh, sh.x, sh.y, sh.z)
    long_cols = max(max(np.diff(c[1]), default=0) for c in sh.copies().values()) > cs.SPMV_LONG_COL
    for lab, rx, ry, rz in row_lists(sh):
        what = f"{name} rows {lab} ref_order={ref_order}"
        for (a, g), full in fold.items():
            if lab != "third" and not (a and g):
                continue
            ox, oy, oz, _, _ = run(hip, sh, "fold_rhs_rows", ref_order, rows=(rx, ry, rz), with_A=a, with_G=g)
            listed_only(ox, full, rx, f"{what} fold_rhs_rows with_A={a} with_G={g}")
            untouched(oy, "fold_rhs_rows out_y"); untouched(oz, "fold_rhs_rows out_z")
        if ref_order:
            continue  # (only the fold has statements of its own in the reference-order mode)
        ox, oy, oz, _, _ = run(hip, sh, "recover_duals_rows", ref_order, rows=(rx, ry, rz))
        untouched(ox, "recover_duals_rows out_x")
        listed_only(oy, ly, ry, what + " recover_duals_rows lhs_y"); listed_only(oz, lz, rz, what + " recover_duals_rows lhs_z")
        ox, oy, oz, absmax, ok = run(hip, sh, "residual_rows", ref_order, rows=(rx, ry, rz))
        if long_cols:  # a column too long for the row form: refused, nothing written
            assert ok == 0 and absmax == 0
            untouched(ox, what + " refused residual_rows"); untouched(oy, what + " refused residual_rows"); untouched(oz, what + " refused residual_rows")
            continue
        assert ok == 1
        listed_only(ox, ex, rx, what + " residual_rows err_x"); listed_only(oy, ey, ry, what + " residual_rows err_y"); listed_only(oz, ez, rz, what + " residual_rows err_z")
        worst = max([0.0] + [float(np.abs(e[r]).max()) for e, r in ((ex, rx), (ey, ry), (ez, rz)) if r.size])
        assert absmax == int(cs.bits(np.array([worst]))[0]), (what, hex(absmax), worst)
        if rx.size:  # one NaN in lhs_x at a listed row
            xn = sh.x.copy(); xn[rx[rx.size // 2]] = np.nan
            assert run(hip, sh, "residual_rows", ref_order, rows=(rx, ry, rz), in_x=xn)[3:] == (NAN_BITS, 1), what
    assert name != "long" or long_cols


def test_debug_entry_refuses_what_a_kernel_would_index_with(hip):
    """a row list or a pattern out of range is an error before anything is launched, and the outputs stay as they were"""
    sh = cs.shape("edges_65")
    for rows in ((np.array([sh.n]), (), ()), ((), np.array([-1]), ()), ((), (), np.array([0, sh.m]))):
        with pytest.raises(RuntimeError, match="row list rows_[xyz] out of range"):
            run(hip, sh, "residual_rows", rows=rows)
    bad = object.__new__(cs.Shape)
    bad.__dict__.update(sh.__dict__)
    cp, ri, v = sh.GT
    ri = ri.copy(); ri[-1] = sh.n
    bad.GT = (cp, ri, v)
    with pytest.raises(RuntimeError, match="row index of GT out of range"):
        run(hip, bad, "eval_G")
    bad.GT = sh.GT
    bad.P = (sh.P[0], np.where(np.arange(sh.P[1].size) == 0, sh.n - 1, sh.P[1]).astype(np.int32), sh.P[2])  # (n - 1, 0): below the diagonal
    with pytest.raises(RuntimeError, match="not upper triangular"):
        run(hip, bad, "eval_P_x")


def test_long_columns_default_mode(hip):
    """columns above SPMV_LONG_COL entries: bitwise the strided-plus-tree reference (test_evals_bitwise_the_reference), the same bits from two calls, and --
    independently of that reference -- within the running-error bound of the tree of the exact value: depth ceil(len / 256) of the strided sums, 8 tree levels, the
    product and the scaling by alpha, each at most 2**-53 relative to sum |val x|.  The exact value is formed in rational arithmetic."""
    sh = cs.shape("long")
    c = sh.copies()
    an, at = cs.ALPHAS
    first, second = device_evals(hip, sh, False, 0), device_evals(hip, sh, False, 0)
    check_evals(first, second, "long: two calls")
    px, (a_n, a_t), (g_n, g_t) = first
    seen = 0
    for nm, got, alpha, x in (("Pf", px, an, sh.xs[0]), ("A", a_t, at, sh.ys[0]), ("GT", g_n, an, sh.xs[0])):
        _, cp, ri, v = c[nm]
        for j in np.nonzero(np.diff(cp) > cs.SPMV_LONG_COL)[0]:
            terms = [Fraction(v[q]) * Fraction(float(x[ri[q]])) for q in range(cp[j], cp[j + 1])]
            exact = Fraction(alpha) * sum(terms)
            ln = cp[j + 1] - cp[j]
            bound = (-(-ln // 256) + 10) * Fraction(1, 2 ** 53) * abs(Fraction(alpha)) * sum(abs(t) for t in terms)
            err = abs(Fraction(float(got[j])) - exact)
            print(f"long {nm} column {j}: {ln} entries, error {float(err):.3e}, bound {float(bound):.3e}")
            assert err <= bound, (nm, int(j), ln, float(err), float(bound))
            seen += 1
    assert seen == 4 + 4 + 1  # 2049, 2304, 2305 and 2600 entries in A and in GT (2048 stays on the wave path), the arrow column of P


# ------------------------------------------------------------------------------------------------------------------- the same products through real handles
@functools.lru_cache(maxsize=None)
def handle_problem():
    from qp_gen import dense_strongly_convex_qp
    from test_sparse_gpu import _sparsify
    return _sparsify(dense_strongly_convex_qp(321, 130, 257, seed=322), 0.05, 321)


def handle_data(hip):
    from test_sparse_gpu import _args
    q = handle_problem()
    d = hip.SparseData(*_args(q))
    return q, d, cs.Shape.from_matrices("handles", d.n, d.p, d.m, d.P_utri, d.AT, d.GT)


def handle_vectors(d):
    rng = np.random.default_rng(9)
    return rng.standard_normal(d.n), rng.standard_normal(d.p), rng.standard_normal(d.m)


def test_multifrontal_handle_evals_bitwise_the_default_mode_reference(hip):
    q, d, sh = handle_data(hip)
    k = hip.SparseKKT(d, kkt_solver=hip.SPARSE_LDLT_MULTIFRONTAL)
    x, y, z = handle_vectors(d)
    an, at = cs.ALPHAS
    got = (k.eval_P_x(an, x), k.eval_A_xn_and_AT_xt(an, at, x, y), k.eval_G_xn_and_GT_xt(an, at, x, z))
    check_evals(got, (cs.eval_P_x(sh, an, x), cs.eval_A(sh, an, at, x, y), cs.eval_G(sh, an, at, x, z)), "multifrontal handle:")


def test_exact_handle_evals_bitwise_the_oracle(hip, orc):
    q, d, sh = handle_data(hip)
    k = hip.SparseKKT(d, kkt_solver=hip.SPARSE_LDLT_EXACT)
    ko = orc.KKT(orc.Data.sparse(**q), kind="sparse", mode=0)
    x, y, z = handle_vectors(d)
    an, at = cs.ALPHAS
    got = (k.eval_P_x(an, x), k.eval_A_xn_and_AT_xt(an, at, x, y), k.eval_G_xn_and_GT_xt(an, at, x, z))
    check_evals(got, (ko.eval_P_x(an, x), ko.eval_A_xn_and_AT_xt(an, at, x, y), ko.eval_G_xn_and_GT_xt(an, at, x, z)), "reference-order handle against the oracle:")
    check_evals(got, (cs.eval_P_x(sh, an, x, True), cs.eval_A(sh, an, at, x, y, True), cs.eval_G(sh, an, at, x, z, True)), "reference-order handle:")


@pytest.mark.parametrize("engine", ["multifrontal", "exact"])
@pytest.mark.parametrize("ksid,mode", [(2, 1), (3, 2), (4, 3)])
def test_condensed_backends_recover_the_duals_from_the_returned_x(hip, monkeypatch, ksid, mode, engine):
    """in the condensed modes the eliminated multipliers are a pure function of the returned lhs_x: y in mode 1, z in mode 2, both in mode 3, bitwise recover_duals
    with zinv = 1 / z_reg as the backend forms it and delta_inv = 1.0 / delta"""
    monkeypatch.setenv("PIQP_AMD_SPARSE_LDLT", engine)  # read when the handle is created
    q, d, sh = handle_data(hip)
    k = hip.SparseKKT(d, kkt_solver=ksid)
    rng = np.random.default_rng(3)
    x_reg = rng.uniform(0.5, 2.0, d.n); z_reg = rng.uniform(0.1, 3.0, d.m); delta = 1.2
    assert k.update_scalings_and_factor(delta, x_reg, z_reg)
    rx, ry, rz = rng.standard_normal(d.n), rng.standard_normal(d.p), rng.standard_normal(d.m)
    lx, ly, lz = k.solve(rx, ry, rz)
    assert np.isfinite(lx).all() and np.isfinite(ly).all() and np.isfinite(lz).all()
    wy, wz = cs.recover_duals(sh, lx, rhs_y=ry, rhs_z=rz, zinv=1.0 / z_reg, delta_inv=1.0 / delta)
    if mode & 1:
        same(ly, wy, f"mode {mode} behind {engine}: lhs_y")
    if mode & 2:
        same(lz, wz, f"mode {mode} behind {engine}: lhs_z")
