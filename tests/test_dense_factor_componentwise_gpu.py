"""The dense factorisation (launch_factor_panels: potrf_block, k_trsm_panel, the fused launch per panel and k_chol_persistent), the triangular sweeps (launch_trsv)
and the mat-vec kernels (k_gemv_n_partial, k_reduce_partials, k_gemv_t) of csrc/dense_kernels.hip, each held ENTRY BY ENTRY to a rounding bound that is derived
below and not measured, at the smallest size that reaches each branch of their launchers (tests/factor_shapes.py; tests/test_factor_plan.py pins on the CPU that
each size reaches its branch).  Handles with p = m = 0, so K = Pf + diag(x_reg), asserted bit for bit first.  u = 2^-53, gamma_k = k u / (1 - k u).

FACTOR.  F = tril(internal_factor()).  Cholesky: R = K - F F^T, S = |F| |F|^T; L D L^T: L the unit lower part, D = diag(F), R = K - L D L^T, S = |L| |D| |L|^T.
Asserted on the lower triangle: |R_ij| <= c_ij S_ij, everything finite, with (j the 0-based column, q = j + 1 the number of terms of its sum)
    c_ij = gamma_(q + 4) + gamma_(q + 2) + [row i in a later 128-block than column j] 2 gamma_17 K16.
 * gamma_(q + 4), the factorisation: Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3 gives gamma_(q + 1) for the q-term sum of column j formed in any
   order (the matrix-core products are fused multiply-adds; tiles, stages, panels and multi-panel visits only regroup the sum), the division and the square root.
   The device multiplies by the reciprocal pivot instead of dividing (one more rounding), and in L D L^T scales the operand by D before the product and the solved
   panel by 1 / D after it (two more).
 * gamma_(q + 2), the host: F F^T in fp64 is a q-term sum in any order (gamma_q), one more product per term with D, the subtraction from K.
 * 2 gamma_17 K16, the explicit inverses: below the diagonal 128-block a row t of the panel is not substituted against the 16 x 16 diagonal piece D of L but
   multiplied by its inverse (k_trsm_panel and the panel tasks of the fused / persistent launches: x = t W^T, W = fl(D^-1) from potrf_block).  W^T comes from a
   substitution Z D^T = I, so |W^T D^T - I| <= gamma_16 |W^T| |D^T|; the product adds |x - t W^T| <= gamma_16 |t| |W^T|.  Hence
   |x D^T - t| <= 2 gamma_16 |t| |W^T| |D^T|, and with |t| <= |x| |D^T| to first order, <= 2 gamma_17 |x| (|D|^T |D^-T| |D|^T).  A substitution would leave
   gamma_16 |x| |D|^T, which is part of S; the inverse leaves M = |D|^T |D^-T| |D|^T in its place.  K16 is the assumption that (|X| blockdiag(M))_ij <= K16 S_ij on
   those entries (X = L D): factor_growth computes the left side, and the assumption is asserted for the reference factor of every shape on the CPU and for the
   device's factor in the GPU test.  Inside the diagonal 128-block potrf_block substitutes (tile_trsm_rt_follow): no such term.
Inputs: C = B^T B / n, B standard normal, seeded by n, passed as its upper triangle, x_reg = 0.5: dense, condition number 9, off-diagonal entries of L of order n^-1/2.
The cap is a condition and not a measurement: c_ij <= 8 gamma_(n + 1) at every shape (asserted); one dropped 16-column stage moves an entry by about 16 / n of S_ij,
>= 5e-3 at n = 2944, where the cap is 3e-12.

SWEEPS.  One factorisation, five solves, the device's factor downloaded once: r = L D L^T x - b, s = |L| |D| |L^T| |x| + |b|, both O(n^2) in fp64 on the host;
asserted |r_i| <= c s_i: the sweeps alone, whatever the factorisation's own error, with
    c = 2 gamma_(n + 2) + 2 gamma_(n + 1) + (nblk < 8: 4 gamma_17 K16;  nblk >= 8: 2 (gamma_129 + gamma_17 K16) K128).
 * 2 gamma_(n + 2): a substitution solves (L + dL) y = b with |dL| <= gamma_n |L| in any order of the row sums (Higham Thm 8.5; the helper workgroups' slices and the
   hand-over only regroup them), reciprocal pivots and the 1 / D between the sweeps one rounding each; two sweeps, and |y| <= |D| |L^T| |x| to first order.
 * 2 gamma_(n + 1): r formed on the host, two products of at most n terms and a subtraction.
 * the diagonal step.  nblk < 8: eight steps x_g = W_g b_g with the inverted 16 x 16 pieces, the term of the panel solve above in each sweep.  nblk >= 8: one
   product y = V b with V = the inverse of the 128-row block, formed in double-double from the W_g and rounded once (k_block_inverse_dd):
   |D V - I| <= u |D| |V| + gamma_17 K16 |D| |V| (the pieces' W_g in double, as above), the product adds gamma_128 |V| |b|, so
   |D y - b| <= (gamma_129 + gamma_17 K16) |D| |D^-1| |D| |y|.  K16 / K128 is the assumption that these terms, pushed through the rest of the residual
   (SweepCheck.statistic: forward G |y|, backward |L| |D| G^T |x|, G = blockdiag(|D| |D^-1| |D|)) stay below K times 2 s; asserted with every solve.
Inputs: K = diag(d) + V V^T, d ~ U(1, 2), V standard normal n x 8 scaled by 8^-1/2: O(n^2) to form, L fully dense.  c <= 8 gamma_(n + 1) is asserted here too.
Which schedule the probe at handle creation chose (one XCD by ticket, local hand-over) cannot be seen from Python: 896, 897 and 4096 are therefore also run in a
fresh process with PIQP_AMD_DEBUG=no_one_xcd, and 4096 with sweep_local=0 (tests/workers/dense_sweeps.py prints what it knows: the token, the ratios, the growth).

MAT-VEC.  eval_P_x, eval_A_xn_and_AT_xt, eval_G_xn_and_GT_xt and the y / z outputs of solve against np.longdouble: every output is a sum of k products (k the
length of the dot product) in any order, with at most three more roundings (alpha or 1 / delta, the product with it, beta c or the scale by 1 / z_reg):
|out - ref| <= gamma_(k + 3) (|alpha| |M| |v| + |beta| |c|) |scale|; the reference's own error (u = 2^-64) is 2000 times smaller.

The CPU half (no gpu mark) holds NumPy's and the oracle's factors to the textbook part of the same statistic in np.longdouble, checks K16 / K128 and the plain
condition numbers of the diagonal pieces at every shape for both recipes, holds SciPy's triangular solves to their part of the sweep bound, and shows that both
checks are live: a reference whose residual is off by one 16-column stage of one tile, or one column block out of L (L^T x), fails and is named."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import factor_bounds as fb
from factor_bounds import K16, K128, gamma
from factor_shapes import FACTOR_SHAPES, SWEEP_SHAPES, SWEEP_VARIANTS, UPDATE_SHAPES, by_n, shape_id

NB = 128
# what the plain 2-norm condition numbers of the diagonal pieces of the reference L may be (16 x 16 / 128 x 128).  Factor recipe: cond(K) = 9 bounds every piece of
# the Cholesky factor by 3.  Sweep recipe: the eigenvalues of a 128-row diagonal block of K lie in [1, 2 + |V_k|^2], |V_k|^2 about (128^1/2 + 8^1/2)^2 / 8 = 25, so a
# Cholesky piece stays under 27^1/2 = 5.2; the unit lower pieces of L D L^T differ from it by the scaling with the pivots' roots (measured: within 10 %)
COND16, COND128 = 4.0, 8.0


# ------------------------------------------------------------------------------------------------------------------ shared, unchanged inputs
class FactorProblem:
    def __init__(self, n, generation=0):
        self.n = n
        self.Pf, self.x_regs = fb.factor_input(n, generation)
        self.K = [fb.kkt_matrix(self.Pf, x) for x in self.x_regs]
        for a in [self.Pf] + self.K + self.x_regs:
            a.flags.writeable = False
        self.bound_c = fb.factor_bound(n)


_PROBLEMS = {}


def factor_problem(n):
    """one per shape for the module; the large ones are dropped when the next shape comes"""
    if n not in _PROBLEMS:
        for k in [k for k in _PROBLEMS if k > 640]:
            del _PROBLEMS[k]
        _PROBLEMS[n] = FactorProblem(n)
    return _PROBLEMS[n]


def kind7_visits(T):
    from test_factor_plan import plan
    visits = {}
    for kind, rnd, a, b, gate in plan(T):
        if kind == 7:
            visits.setdefault((int(a), int(b)), []).append((int(rnd), int(gate) + 1))
    return visits


def check_factor(shape, K, F, ldlt, label, product_hook=None):
    """|R_ij| <= c_ij S_ij on the lower triangle, all finite, the growth assumption; returns (largest |R| / (c S), growth).  product_hook(R): the mutation test"""
    n = shape.n
    R, S = fb.factor_statistic(K, F, ldlt)
    if product_hook is not None:
        product_hook(R)
    c = fb.factor_bound(n)
    assert np.tril(c).max() <= fb.factor_cap(n), "the derived constant exceeds the cap 8 gamma_(n + 1)"
    bound = c * S
    rho = fb.factor_growth(F, ldlt, S) if n > NB else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.nanmax(np.tril(np.abs(R)) / bound))
    print(f"  {label}: max |R| / (c S) = {ratio:.3f}, max |R| / S = {float(np.nanmax(np.tril(np.abs(R)) / S)):.3e} (cap {fb.factor_cap(n):.3e}); growth {rho:.3f} (assumed <= {K16})")
    assert np.isfinite(F).all() and np.isfinite(R).all(), f"{label}: not finite"
    assert rho <= K16, f"{label}: the input is worse conditioned than the derivation assumes: growth {rho:.3f}"
    if not (np.tril(np.abs(R)) <= bound).all():
        pytest.fail(f"{label}: " + fb.describe_factor_failure(K, F, ldlt, R, S, bound, kind7_visits(shape.T) if shape.persistent else None), pytrace=False)
    return ratio, rho


def scipy_or_numpy_solve(L, b, trans, unit):
    try:
        from scipy.linalg import solve_triangular
        return solve_triangular(L, b, lower=True, trans="T" if trans else "N", unit_diagonal=unit)
    except ImportError:
        return np.linalg.solve(L.T if trans else L, b)


# ------------------------------------------------------------------------------------------------------------------ CPU half
def test_constants_stay_under_the_cap():
    for s in FACTOR_SHAPES:
        assert np.tril(fb.factor_bound(s.n)).max() <= fb.factor_cap(s.n), s.n
    for s in SWEEP_SHAPES:
        assert fb.sweep_bound(s.n, s.inverse) <= fb.factor_cap(s.n), s.n
        assert fb.sweep_reference_part(s.n) < fb.sweep_bound(s.n, s.inverse)


@pytest.mark.parametrize("shape", [s for s in FACTOR_SHAPES if s.n <= 640], ids=shape_id)
def test_reference_factors_meet_the_textbook_part(orc, shape):
    """np.linalg.cholesky and the oracle's factor (both modes), statistic formed in np.longdouble: |R| <= gamma_(q + 1) S (Cholesky) / gamma_(q + 2) S (L D L^T: one more
    product per term); and the same statistic formed in fp64 moves by at most the host part gamma_(q + 2) S"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    n = shape.n
    pb = factor_problem(n)
    K = pb.K[0]
    od = orc.Data.dense(P=pb.Pf, c=np.zeros(n))
    refs = [("numpy", False, np.linalg.cholesky(K))]
    for ldlt in (False, True):
        ko = orc.KKT(od, use_ldlt=ldlt)
        assert ko.update_scalings_and_factor(1.0, pb.x_regs[0], np.zeros(0))
        assert np.array_equal(np.tril(ko.internal_kkt_mat()), np.tril(K))
        refs.append(("oracle", ldlt, np.tril(ko.internal_factor())))
    q = np.arange(1, n + 1)
    for name, ldlt, F in refs:
        Rl, Sl = fb.factor_statistic(K, F, ldlt, dtype=np.longdouble)
        R, S = fb.factor_statistic(K, F, ldlt)
        part = gamma(q + (2.0 if ldlt else 1.0))
        print(f"  {n} {name} ldlt={ldlt}: max |R| / (gamma S) = {float((np.tril(np.abs(Rl)) / (part * Sl)).max()):.3f}, host part "
              f"{float((np.tril(np.abs(R - Rl)) / (fb.factor_host_part(n) * Sl)).max()):.3f}")
        assert (np.tril(np.abs(Rl)) <= part * Sl).all(), (name, ldlt)
        assert (np.tril(np.abs(R.astype(np.longdouble) - Rl)) <= fb.factor_host_part(n) * Sl).all(), (name, ldlt)


@pytest.mark.parametrize("shape", FACTOR_SHAPES, ids=shape_id)
def test_factor_inputs_are_as_well_conditioned_as_the_derivation_assumes(shape):
    """the growth K16 and the plain condition numbers of the 16 x 16 / 128 x 128 diagonal pieces of the reference L, both modes, both regularisations"""
    pb = factor_problem(shape.n)
    for K in pb.K:
        C = np.linalg.cholesky(K)
        for ldlt in (False, True):
            F = fb.ldlt_of_cholesky(C) if ldlt else C
            _, S = fb.factor_statistic(K, F, ldlt)
            rho = fb.factor_growth(F, ldlt, S) if shape.n > NB else 0.0
            c16, c128 = fb.piece_conditions(F, ldlt, 16), fb.piece_conditions(F, ldlt, NB)
            print(f"  {shape.n} ldlt={ldlt}: growth {rho:.3f}, cond of the pieces {c16:.2f} / {c128:.2f}")
            assert rho <= K16 and c16 <= COND16 and c128 <= COND128


@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=shape_id)
def test_sweep_inputs_and_the_reference_solves(shape):
    """reference L of the sweep recipe: the pieces' condition numbers, and substitution in fp64 (SciPy, or NumPy's general solve on the triangles) within its part
    2 gamma_n + 2 gamma_(n + 1) of the bound with the growth under K16 / K128"""
    n = shape.n
    Pf, x_reg = fb.sweep_input(n)
    C = np.linalg.cholesky(fb.kkt_matrix(Pf, x_reg))
    del Pf
    for ldlt in (False, True):
        F = fb.ldlt_of_cholesky(C) if ldlt else C
        assert fb.piece_conditions(F, ldlt, 16) <= COND16 and fb.piece_conditions(F, ldlt, NB) <= COND128
        chk = fb.SweepCheck(F, ldlt, shape.inverse)
        for q, b in enumerate(fb.right_hand_sides(n)):
            y = scipy_or_numpy_solve(chk.L, b, False, ldlt)
            x = scipy_or_numpy_solve(chk.L, y / chk.d if ldlt else y, True, ldlt)
            ratio, rho, msg = chk.check(x, b, f"{n} ldlt={ldlt} reference solve {q}")
            assert msg is None, msg
            assert ratio * chk.bound <= fb.sweep_reference_part(n)


def test_factor_check_is_live_on_a_mutated_reference():
    """the reference factor at n = 1408, its residual R = K - F F^T changed on tile (10, 9) by one 16-column stage (70: columns 1120..1135, panel 8) of the product, as a
    device that never subtracted that stage from the tile would leave it (F F^T then exceeds K by the stage), then by panel 1 with the other sign (subtracted
    twice): the check fails, and names the tile, the stage or panel, and for the panel the kind-7 visit (panels 1..2) it lies in"""
    shape = by_n(1408)
    pb = factor_problem(1408)
    F = np.linalg.cholesky(pb.K[0])
    check_factor(shape, pb.K[0], F, False, "unmutated")
    tile = (slice(10 * NB, 11 * NB), slice(9 * NB, 10 * NB))

    def drop_stage(R):
        R[tile] -= F[tile[0], 1120:1136] @ F[tile[1], 1120:1136].T

    def double_panel(R):
        R[tile] += F[tile[0], NB:2 * NB] @ F[tile[1], NB:2 * NB].T

    with pytest.raises(pytest.fail.Exception) as e:
        check_factor(shape, pb.K[0], F, False, "stage dropped", drop_stage)
    print(" ", e.value.msg)
    assert "of tile (10, 9)" in e.value.msg and "= 16-column stage 70 missing" in e.value.msg and "= panel 8 missing" not in e.value.msg
    with pytest.raises(pytest.fail.Exception) as e:
        check_factor(shape, pb.K[0], F, False, "panel doubled", double_panel)
    print(" ", e.value.msg)
    assert "of tile (10, 9)" in e.value.msg and "= panel 1 doubled (inside the kind-7 visit of panels 1..2 of that tile)" in e.value.msg


def test_sweep_check_is_live_on_a_mutated_reference():
    """n = 6529 (H = 3: a block row's products are shared by three helpers and the owner): the product of block row 40 with column block 17 -- part of one helper's
    slice -- left out of L (L^T x): the check fails and names the block row and the column block"""
    shape = by_n(6529)
    Pf, x_reg = fb.sweep_input(shape.n)
    chk = fb.SweepCheck(np.linalg.cholesky(fb.kkt_matrix(Pf, x_reg)), False, True)
    b = fb.right_hand_sides(shape.n)[0]
    x = scipy_or_numpy_solve(chk.L, scipy_or_numpy_solve(chk.L, b, False, False), True, False)
    assert chk.check(x, b, "unmutated")[2] is None

    def without_a_slice(L, w):
        y = L @ w
        y[40 * NB:41 * NB] -= L[40 * NB:41 * NB, 17 * NB:18 * NB] @ w[17 * NB:18 * NB]
        return y

    msg = chk.check(x, b, "slice dropped", without_a_slice)[2]
    print(" ", msg)
    assert msg is not None and "of block row 40" in msg and "= the product with column block 17 missing" in msg


# ------------------------------------------------------------------------------------------------------------------ GPU half
@pytest.mark.gpu
@pytest.mark.parametrize("shape,kkt_solver", [(s, ks) for s in FACTOR_SHAPES for ks in (0, 16)], ids=lambda v: shape_id(v) if hasattr(v, "n") else str(v))
def test_factor_componentwise(hip, shape, kkt_solver):
    """one handle per case: K bit for bit, the bound, a second regularisation, the first again bitwise (flag words, generation counters and fuse tokens re-arm), and
    for the persistent shapes 384 and 1408 fresh data on the same handle.  The branch the shape is here for is its `branch` in tests/factor_shapes.py."""
    n, ldlt = shape.n, kkt_solver == 16
    pb = factor_problem(n)
    label = f"{n} kkt_solver {kkt_solver}"
    k = hip.DenseKKT(fb.data_of(hip, pb.Pf), kkt_solver=kkt_solver)
    none = np.zeros(0)
    assert k.update_scalings_and_factor(1.0, pb.x_regs[0], none)
    assert np.array_equal(np.tril(k.internal_kkt_mat()), np.tril(pb.K[0])), "K is not Pf + diag(x_reg) bit for bit"
    F1 = np.tril(k.internal_factor())
    check_factor(shape, pb.K[0], F1, ldlt, label)
    assert k.update_scalings_and_factor(1.0, pb.x_regs[1], none)
    assert np.array_equal(np.tril(k.internal_kkt_mat()), np.tril(pb.K[1]))
    check_factor(shape, pb.K[1], np.tril(k.internal_factor()), ldlt, label + ", second x_reg")
    assert k.update_scalings_and_factor(1.0, pb.x_regs[0], none)
    assert np.array_equal(np.tril(k.internal_factor()), F1), "the first regularisation again is not bitwise the first result"
    if n in UPDATE_SHAPES:
        pb2 = FactorProblem(n, generation=1)
        k.update_data(fb.data_of(hip, pb2.Pf), hip.KKT_UPDATE_P)
        assert k.update_scalings_and_factor(1.0, pb2.x_regs[0], none)
        assert np.array_equal(np.tril(k.internal_kkt_mat()), np.tril(pb2.K[0]))
        check_factor(shape, pb2.K[0], np.tril(k.internal_factor()), ldlt, label + ", update_data")


def assert_sweeps(out, label):
    assert out["factor_ok"], label
    assert out["kkt_bitwise"], f"{label}: K is not Pf + diag(x_reg) bit for bit"
    assert not out["failures"], f"{label}: " + " | ".join(out["failures"])
    assert out["repeat_bitwise"], f"{label}: the fifth solve is not bitwise the first"
    assert len(out["ratios"]) == 5 and max(out["ratios"]) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kkt_solver", [(s, ks) for s in SWEEP_SHAPES for ks in (0, 16)], ids=lambda v: shape_id(v) if hasattr(v, "n") else str(v))
def test_sweeps_componentwise(hip, shape, kkt_solver):
    """|r_i| <= c s_i for five solves in a row on one handle against the factor downloaded once; the fifth repeats the first bit for bit"""
    assert fb.sweep_bound(shape.n, shape.inverse) <= fb.factor_cap(shape.n)
    label = f"{shape.n} kkt_solver {kkt_solver}"
    out = fb.run_sweeps(hip, shape, kkt_solver, label)
    print(f"  {label}: largest |r| / s = {max(out['ratios']):.2e} x bound, growth {max(out['growth']):.3f}")
    assert_sweeps(out, label)


CHILD_TIMEOUT = 300  # seconds: a child imports the library, forms K (n <= 4096) and runs five solves -- about ten seconds
_child_lost = []


@pytest.mark.gpu
@pytest.mark.parametrize("n,token", SWEEP_VARIANTS, ids=lambda v: str(v))
def test_sweeps_componentwise_with_a_schedule_switched_off(hip, n, token):
    """the same check in a fresh process per (shape, token, kkt_solver) with PIQP_AMD_DEBUG=no_one_xcd (no ticket mode, no local hand-over) or sweep_local=0 (the
    helpers' hand-over through memory only).  The worker prints the token, the ratios and the growth; which schedule the default run took is not observable.  A
    child that ends by signal or timeout ends the variant runs: the remaining ones are skipped, nothing more is started on the device."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workers", "dense_sweeps.py")
    for ks in (0, 16):
        if _child_lost:
            pytest.skip(f"not started: the child {_child_lost[0]} ended by signal or timeout")
        label = f"{n} kkt_solver {ks} PIQP_AMD_DEBUG={token}"
        env = dict(os.environ)
        env["PIQP_AMD_DEBUG"] = token
        try:
            r = subprocess.run([sys.executable, worker, str(n), str(ks), token.replace("=", ""), "lowrank"], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            _child_lost.append(label)
            pytest.fail(f"{label}: no result after {CHILD_TIMEOUT} s", pytrace=False)
        print(r.stdout[-3000:])
        if r.returncode < 0:
            _child_lost.append(label)
            pytest.fail(f"{label}: ended by signal {-r.returncode}: {r.stderr[-2000:]}", pytrace=False)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        assert r.returncode == 0 and line, (label, r.stdout[-2000:], r.stderr[-2000:])
        assert_sweeps(json.loads(line[0][7:]), label)


MATVEC_SHAPES = [(1, 1, 1), (2, 0, 31), (513, 32, 33), (514, 257, 0), (512, 0, 300), (1025, 1, 289)]


@pytest.mark.gpu
@pytest.mark.parametrize("dims", MATVEC_SHAPES, ids=lambda d: "-".join(map(str, d)))
def test_matvec_componentwise(hip, dims):
    """(513, 32, 33): odd ld, the scalar path, a second row block of one row; (514, 257, 0): a second 256-column chunk of one column; (512, 0, 300): 10 slices, the
    reduce's k += 8 loop runs twice for two groups; (1025, 1, 289): odd ld, three row blocks, 10 slices"""
    n, p, m = dims
    ld = np.longdouble
    rng = np.random.default_rng([n, p, m, 5])
    P = np.triu(rng.standard_normal((n, n)) * 0.01) + np.diag(np.full(n, 5.0))
    Pf = np.triu(P) + np.triu(P, 1).T
    A, G = rng.standard_normal((p, n)), rng.standard_normal((m, n))
    k = hip.DenseKKT(hip.Data(P, np.zeros(n), A if p else None, np.zeros(p) if p else None, G if m else None, -np.ones(m) if m else None, np.ones(m) if m else None))
    delta, x_reg, z_reg = 0.7, rng.uniform(0.5, 2.0, n), rng.uniform(0.1, 3.0, m)
    assert k.update_scalings_and_factor(delta, x_reg, z_reg)

    def hold(name, out, M, v, alpha, c=None, beta=0.0, scale=None):
        """out = (alpha M v + beta c) scale within gamma_(k + 3), k = len(v)"""
        out = np.asarray(out)
        ref = ld(alpha) * (M.astype(ld) @ v.astype(ld))
        mag = abs(alpha) * (np.abs(M) @ np.abs(v))
        if c is not None:
            ref, mag = ref + ld(beta) * c.astype(ld), mag + abs(beta) * np.abs(c)
        if scale is not None:
            ref, mag = ref * scale.astype(ld), mag * np.abs(scale)
        err = np.abs(out.astype(ld) - ref).astype(np.float64)
        bound = gamma(len(v) + 3) * mag
        assert out.shape == ref.shape and np.isfinite(out).all(), name
        if out.size:
            print(f"  {n}-{p}-{m} {name}: max err / (|M| |v|) = {float((err[mag > 0] / mag[mag > 0]).max(initial=0.0)):.3e} (bound {gamma(len(v) + 3):.3e})")
            bad = np.nonzero(~(err <= bound))[0]
            assert bad.size == 0, f"{name}: {bad.size} entries over the bound, first {bad[0]}: err {err[bad[0]]:.3e}, bound {bound[bad[0]]:.3e}"

    x, y, z = rng.standard_normal(n), rng.standard_normal(p), rng.standard_normal(m)
    hold("eval_P_x", k.eval_P_x(-1.5, x), Pf, x, -1.5)
    zn, zt = k.eval_A_xn_and_AT_xt(-1.0, 2.0, x, y)
    hold("A xn", zn, A, x, -1.0)
    hold("A^T xt", zt, A.T, y, 2.0)
    zn, zt = k.eval_G_xn_and_GT_xt(0.5, -3.0, x, z)
    hold("G xn", zn, G, x, 0.5)
    hold("G^T xt", zt, G.T, z, -3.0)
    rx, ry, rz = rng.standard_normal(n), rng.standard_normal(p), rng.standard_normal(m)
    lx, ly, lz = k.solve(rx, ry, rz)
    # lhs_y = (A lhs_x - rhs_y) / delta and lhs_z = (G lhs_x - rhs_z) / z_reg, from the device's own lhs_x
    hold("lhs_y", ly, A, lx, 1.0, c=ry, beta=-1.0, scale=np.full(p, 1.0 / delta))
    hold("lhs_z", lz, G, lx, 1.0, c=rz, beta=-1.0, scale=1.0 / z_reg)
