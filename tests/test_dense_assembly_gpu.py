"""The dense KKT assembly (k_syrk_lower<EPI_ASSEMBLE / EPI_STORE>, k_syrk_tail_reduce, k_assemble_no_g: csrc/dense_kernels.hip) against a NumPy fp64
reference, ENTRY BY ENTRY, at the smallest shape that reaches each branch of the launcher (tests/assembly_shapes.py; tests/test_syrk_plan.py pins on the CPU that
each shape reaches its branch, and the GPU test asserts the same plan again).

Reference:   E = Pf + diag(x_reg) + (1 / delta) A^T A + (G^T * (1 / z_reg)) @ G
Bound, derived and not measured: every entry of the device result and of the NumPy result is a sum of at most m + p + 2 terms, each formed with at most about six
further roundings (the reciprocals 1 / z and 1 / delta, the scaling of the column operand, the product, the scale by 1 / delta), summed in an arbitrary order.  Each
therefore lies within gamma_k S_ij of the exact value, with k = m + p + 8, gamma_k = k u / (1 - k u), u = 2^-53 and
             S = |Pf| + diag(|x_reg|) + (1 / delta) |A|^T |A| + (|G|^T * (1 / z_reg)) @ |G|,
and the two within 2 gamma_k S_ij of each other.  At m = 520 that is 1.2e-13 S_ij; one dropped, doubled or mis-scaled k index moves an entry by about S_ij / m,
a tile written to the wrong place by O(1).  The NumPy half of the bound is checked on its own against np.longdouble (no GPU needed) for the shapes with n <= 640.

Inputs as in tests/test_dense_gpu.py::test_assembly_split_k_tail_matches_numpy: P = triu(0.01 randn) + 5 I, G and A randn, every row of G with two finite bounds (no
row zeroed), x_reg ~ U(0.5, 2), z_reg ~ U(0.1, 3), delta 0.7 or 1.2."""
import numpy as np
import pytest

from assembly_shapes import GRID, SOLVE_SHAPES, UPDATE_SHAPES, by_dims, shape_id

U = 2.0 ** -53
TOL = 1e-10  # the project's residual bar (tests/test_fullsize_gpu.py)
TS, BK = 128, 16


def gamma(k):
    return k * U / (1.0 - k * U)


class Problem:
    """inputs of one shape (seeded by the shape and a generation number: update_data takes generation 1) and its references"""

    def __init__(self, shape, generation=0):
        n, p, m = shape.n, shape.p, shape.m
        self.shape, self.n, self.p, self.m = shape, n, p, m
        rng = np.random.default_rng([n, p, m, generation])
        self.P = np.triu(rng.standard_normal((n, n)) * 0.01) + np.diag(np.full(n, 5.0))
        self.G = rng.standard_normal((m, n))
        self.A = rng.standard_normal((p, n))
        self.Pf = np.triu(self.P) + np.triu(self.P, 1).T
        self.absG, self.absA = np.abs(self.G), np.abs(self.A)
        # two scalings: the first one's references are computed once and shared by every check of this shape
        self.scalings = [(0.7, rng.uniform(0.5, 2.0, n), rng.uniform(0.1, 3.0, m)), (1.2, rng.uniform(0.5, 2.0, n), rng.uniform(0.1, 3.0, m))]
        self.E, self.S = self.reference(*self.scalings[0])
        self.E.flags.writeable = False
        self.S.flags.writeable = False

    def data(self, hip):
        n, p, m = self.n, self.p, self.m
        return hip.Data(self.P, np.zeros(n), self.A if p else None, np.zeros(p) if p else None, self.G if m else None, -np.ones(m) if m else None,
                        np.ones(m) if m else None)

    def reference(self, delta, x_reg, z_reg, dtype=np.float64):
        """(E, S) in `dtype`; the reciprocals are taken in that precision too"""
        one = dtype(1.0)
        G, A, aG, aA = (M.astype(dtype, copy=False) for M in (self.G, self.A, self.absG, self.absA))
        zi, di = one / z_reg.astype(dtype), one / dtype(delta)
        E = self.Pf.astype(dtype) + np.diag(x_reg.astype(dtype)) + di * (A.T @ A) + (G.T * zi) @ G
        S = np.abs(self.Pf).astype(dtype) + np.diag(np.abs(x_reg).astype(dtype)) + di * (aA.T @ aA) + (aG.T * zi) @ aG
        return E, S

    @property
    def k(self):
        return self.m + self.p + 8


# One Problem per shape for the whole module, whatever order pytest runs the parametrised tests in: the shapes more than one test function uses (the solve
# shapes, and the small ones of the CPU half) stay in this cache, the others live as long as the module-scoped fixture keeps them
_SHARED = {}


@pytest.fixture(scope="module")
def problem(request):
    sh = request.param
    key = (sh.n, sh.p, sh.m)
    if key in _SHARED:
        return _SHARED[key]
    pb = Problem(sh)
    if key in SOLVE_SHAPES or sh.n <= 640:
        _SHARED[key] = pb
    return pb


def on_shapes(shapes):
    return pytest.mark.parametrize("problem", shapes, ids=shape_id, indirect=True)


def describe_worst(pb, K, E, S, scaling, bound):
    """where and what the worst entry of the lower triangle is: its tile, the K slice it would belong to in a split tail, and whether it is the reference with one K
    stage of G' W G missing or doubled -- the three facts that locate the branch in dense_kernels.hip"""
    n, m = pb.n, pb.m
    excess = np.tril(np.abs(K - E) - bound)
    i, j = np.unravel_index(int(np.argmax(excess)), excess.shape)
    diff = K[i, j] - E[i, j]
    msg = f"entry ({i}, {j}) of tile ({i // TS}, {j // TS}): device {float(K[i, j])!r}, reference {float(E[i, j])!r}, diff {diff:.3e}, bound {bound[i, j]:.3e}, S {S[i, j]:.3e}; " \
          f"{int((excess > 0).sum())} entries of the lower triangle over the bound"
    if m:
        zi = 1.0 / scaling[2]
        terms = pb.G[:, i] * zi * pb.G[:, j]
        nkt = -(-m // BK)
        stages = np.array([terms[s * BK:(s + 1) * BK].sum() for s in range(nkt)])
        k_split = pb.shape.assembly[5]
        kt_per = -(-nkt // k_split)
        for s in range(nkt):
            for what, v in (("missing", -stages[s]), ("doubled", stages[s])):
                if abs(diff - v) <= 4 * bound[i, j]:
                    msg += f"; = the reference with K stage {s} (slice {s // kt_per} of {k_split}) {what}"
    return msg


def check_assembly(pb, K, scaling, ref=None):
    """lower triangle within 2 gamma_k S of the reference entry by entry, strict upper triangle exactly zero (internal_kkt_mat assembles into a zeroed buffer)"""
    E, S = ref if ref is not None else pb.reference(*scaling)
    bound = 2.0 * gamma(pb.k) * S
    err = np.abs(K - E)
    rel = float((np.tril(err) / S).max())
    print(f"  {shape_id(pb.shape)}: max |K - E| / S = {rel:.3e} (bound {2.0 * gamma(pb.k):.3e})")
    assert np.isfinite(K).all()
    if not (np.tril(err) <= bound).all():
        pytest.fail(describe_worst(pb, K, E, S, scaling, bound), pytrace=False)
    assert not np.triu(K, 1).any(), "an entry above the diagonal was written"


def plan_of(hip, n, kdim, with_workspace):
    import ctypes as C
    out = (C.c_int * 6)()
    assert hip._lib.load().pq_debug_syrk_plan(n, kdim, int(with_workspace), C.byref(out)) == 0
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------ CPU half: the reference itself
@on_shapes([s for s in GRID if s.n <= 640])
def test_numpy_reference_is_within_its_half_of_the_bound(problem):
    """|E_fp64 - E_longdouble| <= gamma_k S entry by entry (x87 extended precision: u = 2^-64, its own error is 2000 times below the bound), for both scalings"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    for sc in problem.scalings:
        E, S = problem.reference(*sc)
        El, _ = problem.reference(*sc, dtype=np.longdouble)
        err = np.abs(E.astype(np.longdouble) - El)
        print(f"  {shape_id(problem.shape)}: max |E - E_ld| / S = {float((err / S).max()):.3e} (bound {gamma(problem.k):.3e})")
        assert (err <= gamma(problem.k) * S).all()


# (the residual ratios LAPACK reaches at these shapes are recorded beside SOLVE_SHAPES in tests/assembly_shapes.py)
def right_hand_sides(pb):
    rng = np.random.default_rng([pb.n, pb.p, pb.m, 99])
    return rng.standard_normal(pb.n), rng.standard_normal(pb.p), rng.standard_normal(pb.m)


def reduced_rhs(pb, scaling, rx, ry, rz):
    delta, _, z_reg = scaling
    return rx + pb.G.T @ (rz / z_reg) + pb.A.T @ ry / delta


@on_shapes([by_dims(d) for d in SOLVE_SHAPES])
def test_solve_shapes_are_well_conditioned(problem):
    """LAPACK on the reference matrix meets the reduced system's residual with at least a factor 10 to spare of TOL"""
    sc = problem.scalings[0]
    b = reduced_rhs(problem, sc, *right_hand_sides(problem))
    x = np.linalg.solve(problem.E, b)
    ratio = np.abs(problem.E @ x - b).max() / np.abs(b).max()
    print(f"  {shape_id(problem.shape)}: |E x - b|_inf / |b|_inf = {ratio:.3e}")
    assert 10.0 * ratio <= TOL


# ------------------------------------------------------------------------------------------------------------------ GPU half
@pytest.mark.gpu
@on_shapes(GRID)
def test_assembly_componentwise(hip, problem):
    """one handle per shape: plan, bound, zero upper triangle, a second scaling, the bitwise repeat of the first, and (UPDATE_SHAPES) fresh data on the same handle.
    The branch each shape is here for and its plan are the `branch`, `assembly` and `ata` fields of tests/assembly_shapes.py, asserted first."""
    pb, sh = problem, problem.shape
    if sh.assembly is not None:
        assert plan_of(hip, sh.n, sh.m, True) == sh.assembly, sh.branch
    if sh.ata is not None:
        assert plan_of(hip, sh.n, sh.p, False) == sh.ata, sh.branch
    k = hip.DenseKKT(pb.data(hip))
    first, second = pb.scalings
    assert k.update_scalings_and_factor(*first)
    K1 = k.internal_kkt_mat()
    check_assembly(pb, K1, first, ref=(pb.E, pb.S))
    # other delta, x_reg, z_reg on the same handle: stale split-K partial slots or a stale 1 / z_reg would show
    assert k.update_scalings_and_factor(*second)
    check_assembly(pb, k.internal_kkt_mat(), second)
    # the first arguments again: bit for bit the first result (the tail's slots are fixed per (tile, slice) and summed in slice order)
    assert k.update_scalings_and_factor(*first)
    assert np.array_equal(k.internal_kkt_mat(), K1)
    if (sh.n, sh.p, sh.m) in UPDATE_SHAPES:
        pb2 = Problem(sh, generation=1)
        k.update_data(pb2.data(hip), hip.KKT_UPDATE_P | hip.KKT_UPDATE_A | hip.KKT_UPDATE_G)
        assert k.update_scalings_and_factor(*pb2.scalings[0])
        check_assembly(pb2, k.internal_kkt_mat(), pb2.scalings[0], ref=(pb2.E, pb2.S))


@pytest.mark.gpu
@pytest.mark.parametrize("kkt_solver", [0, 16])
@on_shapes([by_dims(d) for d in SOLVE_SHAPES])
def test_factor_and_solve_residual(hip, problem, kkt_solver):
    """factor + solve at the same shapes, residual of the reduced system formed with the NumPy matrix E (independent of the device assembly), as
    tests/test_fullsize_gpu.py::test_c2_dense_factor_columns_and_solve_vs_oracle does it, with the same bar"""
    pb = problem
    sc = delta, x_reg, z_reg = pb.scalings[0]
    k = hip.DenseKKT(pb.data(hip), kkt_solver=kkt_solver)
    assert k.update_scalings_and_factor(*sc)
    rx, ry, rz = right_hand_sides(pb)
    lx, ly, lz = k.solve(rx, ry, rz)
    b = reduced_rhs(pb, sc, rx, ry, rz)
    res = np.abs(pb.E @ lx - b).max()
    print(f"  {shape_id(pb.shape)} kkt_solver {kkt_solver}: |E lx - b|_inf / |b|_inf = {res / np.abs(b).max():.3e}")
    assert res <= TOL * np.abs(b).max()
    if pb.m:
        Glx = pb.G @ lx
        assert np.abs(Glx - z_reg * lz - rz).max() <= TOL * max(1.0, np.abs(rz).max(), np.abs(Glx).max())
    if pb.p:
        Alx = pb.A @ lx
        assert np.abs(Alx - delta * ly - ry).max() <= TOL * max(1.0, np.abs(ry).max(), np.abs(Alx).max())
