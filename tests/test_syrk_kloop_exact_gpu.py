"""The K loop of syrk_lower_body (csrc/dense_kernels.hip) with ZERO tolerance, on data whose every product and partial sum is an exactly representable integer.

tests/test_dense_assembly_gpu.py holds the assembly to a componentwise bound at every launch shape; a bound leaves room for a loop that takes a weight from the
wrong K stage, drops or doubles a stage, or advances an operand address by the wrong stride on a few entries.  Here none of that has room:

  P = 2^20 I + small symmetric integers, G (and A) with entries in {-3 .. 3}, x_reg integer, z_reg[k] = 2^-e(k) with e(k) in {0 .. 3}, so that 1 / z_reg[k] is
  exactly 1, 2, 4 or 8.  Two exponent patterns run on every handle:
    "plain"  e(k) = (k + shift) mod 4: neighbouring columns differ.  Its period divides the 4 columns between a 4-wave workgroup's loads of one wave and
             the 16 columns of a stage, so ONE wave sees one weight in all its slots and stages: this pattern alone cannot see a weight taken from the wrong
             slot, stage or split-K slice;
    "mixed"  e(k) = (k + k // 4 + k // 16 + k // 64) mod 4: also differs 4 columns on (the next slot of a wave), 16 columns on (the same slot of the next stage)
             and 64 columns on (slices of the split-K tail), which the CPU half asserts.

Every weighted operand fl(w_k * g) is an integer of at most 5 bits, every product an integer, every partial sum an integer far below 2^53: the result does not
depend on the summation order and must EQUAL the NumPy integer result.  The premise itself (bound on the partial sums, float64 evaluation == int64 evaluation) is
asserted on the CPU below, so that a change of the recipe cannot make the GPU test vacuous.

Shapes (n, p, m): the smallest that reach each case of the loop (BK = 16 columns per stage, two LDS slots, the 16-wave shape up to kdim 256, the 4-wave shape
above; tests/assembly_shapes.py and tests/test_syrk_plan.py pin the plans)."""
import numpy as np
import pytest

TS, BK = 128, 16

CASES = [
    # n, p, m, what the shape is here for
    (128, 0, 16, "one stage, no prefetch"),
    (128, 0, 17, "second stage of one column, checked path"),
    (129, 0, 32, "odd ld, edge tiles, two full stages"),
    (256, 0, 48, "three stages, both LDS slots reused"),
    (384, 0, 256, "last kdim of the 16-wave shape"),
    (384, 0, 257, "first kdim of the 4-wave shape"),
    (4096, 0, 128, "split-K tail: slices start at kt_begin != 0"),
    (384, 300, 0, "EPI_STORE from A into ATA"),
]
DELTA = 0.5  # 1 / delta = 2 exactly


def case_id(c):
    return f"n{c[0]}_p{c[1]}_m{c[2]}"


class Case:
    def __init__(self, n, p, m):
        self.n, self.p, self.m = n, p, m
        rng = np.random.default_rng([n, p, m, 7])
        U = np.triu(rng.integers(-2, 3, (n, n)), 1)
        self.Pf = U + U.T + np.diag(np.full(n, 2 ** 20) + rng.integers(0, 4, n))  # int64, symmetric
        self.G = rng.integers(-3, 4, (m, n))
        self.A = rng.integers(-3, 4, (p, n))
        self.x_reg = rng.integers(1, 6, n)
        self._E = {}

    def exponents(self, shift):
        """shift 0 / 1: the plain pattern and its shift by one; "mixed": see the module docstring"""
        k = np.arange(self.m)
        return (k + k // 4 + k // 16 + k // 64) % 4 if shift == "mixed" else (k + shift) % 4

    def z_reg(self, shift):
        return 2.0 ** -self.exponents(shift)

    def weights(self, shift):
        return 2 ** self.exponents(shift)  # 1 / z_reg as integers

    def expected(self, shift, dtype=np.float64, cols=None):
        """Pf + diag(x_reg) + (1 / delta) A^T A + G^T diag(1 / z_reg) G in `dtype` (all columns, or the columns `cols`)"""
        sel = slice(None) if cols is None else cols  # (all columns: plain slices, no gather of 4096^2 entries)
        cols = np.arange(self.n) if cols is None else cols
        E = self.Pf[:, sel].astype(dtype)
        E[cols, np.arange(len(cols))] += self.x_reg[cols].astype(dtype)
        G, A = self.G.astype(dtype), self.A.astype(dtype)
        if self.p:
            E += dtype(round(1 / DELTA)) * (A.T @ A[:, sel])
        if self.m:
            E += (G.T * self.weights(shift).astype(dtype)) @ G[:, sel]
        return E

    def reference(self, shift):
        """what internal_kkt_mat must return: the lower triangle of the float64 evaluation, zeros above; computed once per (case, shift) and read-only"""
        if shift not in self._E:
            E = np.tril(self.expected(shift))
            E.flags.writeable = False
            self._E[shift] = E
        return self._E[shift]

    def data(self, hip):
        n, p, m = self.n, self.p, self.m
        f = np.float64
        return hip.Data(self.Pf.astype(f), np.zeros(n), self.A.astype(f) if p else None, np.zeros(p) if p else None, self.G.astype(f) if m else None,
                        -np.ones(m) if m else None, np.ones(m) if m else None)


_CASES = {}


@pytest.fixture(scope="module")
def case(request):
    key = request.param[:3]
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


on_cases = pytest.mark.parametrize("case", CASES, ids=case_id, indirect=True)


# ------------------------------------------------------------------------------------------------------------------ CPU half: the premise
@on_cases
def test_recipe_is_exact_integer_arithmetic(case):
    """no partial sum can leave the exactly representable integers, and NumPy's float64 evaluation is the int64 one (all columns; at n = 4096 a few tile-boundary
    columns and every 509th, the int64 product of NumPy being slow)"""
    c = case
    for shift in (0, 1, "mixed"):
        w = c.weights(shift)
        assert np.array_equal(1.0 / c.z_reg(shift), w.astype(np.float64)) and set(np.unique(w)) <= {1, 2, 4, 8}
        if c.m >= 4:
            assert len(set(w[:4])) == 4 and (w[:-1] != w[1:]).sum() >= 3 * (c.m - 1) // 4  # neighbouring columns differ (mixed: but for one pair in four)
        if shift == "mixed":
            # in EVERY stage a column's weight differs from that of the next slot of its wave (4 on) and, but in the last stage, of the same slot a stage on
            for k0 in range(0, c.m, BK):
                st = np.arange(k0, min(k0 + BK, c.m))
                assert not len(st[st + 4 < c.m]) or (w[st[st + 4 < c.m]] != w[st[st + 4 < c.m] + 4]).any()
                assert not len(st[st + BK < c.m]) or (w[st[st + BK < c.m]] != w[st[st + BK < c.m] + BK]).all()
            if c.m > 64:
                assert (w[:-64] != w[64:]).all()
        # the largest absolute value any partial sum, in any order, can reach
        worst = np.abs(c.Pf).max() + c.x_reg.max() + round(1 / DELTA) * (np.abs(c.A).sum(axis=0).max() * 3 if c.p else 0) + (8 * 3 * np.abs(c.G).sum(axis=0).max() if c.m else 0)
        assert worst < 2 ** 53 and np.abs(c.G).max(initial=0) <= 3 and np.abs(c.A).max(initial=0) <= 3
        cols = None if c.n <= 512 else np.unique(np.concatenate([np.arange(0, c.n, 509), [TS - 1, TS, c.n // 2 - 1, c.n // 2, c.n - 1]]))
        Ei = c.expected(shift, dtype=np.int64, cols=cols)
        Ef = c.expected(shift, cols=cols)
        assert np.abs(Ei).max() <= worst
        assert np.array_equal(Ef, Ei.astype(np.float64)) and np.array_equal(Ef.astype(np.int64), Ei)
        if cols is None:
            assert np.array_equal(Ei, Ei.T) and np.array_equal(c.reference(shift), np.tril(Ef))


# ------------------------------------------------------------------------------------------------------------------ GPU half
def check_exact(c, K, shift):
    E = c.reference(shift)
    if np.array_equal(K, E):
        return
    assert not np.triu(K, 1).any(), "an entry above the diagonal was written"
    bad = np.argwhere(K != E)
    i, j = bad[0]
    pytest.fail(f"{len(bad)} entries of the lower triangle differ from the integer result; first ({i}, {j}) of tile ({i // TS}, {j // TS}): device {K[i, j]!r}, "
                f"exact {E[i, j]!r}, difference {K[i, j] - E[i, j]!r}", pytrace=False)


@pytest.mark.gpu
@on_cases
def test_assembly_equals_the_integer_result(hip, case):
    c = case
    k = hip.DenseKKT(c.data(hip))
    assert k.update_scalings_and_factor(DELTA, c.x_reg.astype(np.float64), c.z_reg(0))
    check_exact(c, k.internal_kkt_mat(), 0)
    if c.m:
        assert k.update_scalings_and_factor(DELTA, c.x_reg.astype(np.float64), c.z_reg("mixed"))
        check_exact(c, k.internal_kkt_mat(), "mixed")
    if (c.n, c.m) == (4096, 128):
        # the weight pattern shifted by one on the same handle: every column of every stage and slice gets another weight
        assert k.update_scalings_and_factor(DELTA, c.x_reg.astype(np.float64), c.z_reg(1))
        check_exact(c, k.internal_kkt_mat(), 1)
