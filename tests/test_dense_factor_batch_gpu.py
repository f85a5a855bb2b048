"""pq_dense_factor_batch_* / piqp_amd.BatchLLT, piqp_amd.BatchLDLTNoPivot (csrc/dense_factor_batch.hip): Eigen::LLT and piqp::dense::LDLTNoPivot for a batch of small
matrices in one launch, held PER MATRIX and BIT FOR BIT to the CPU oracle's restatement of the two classes (oracle/orc_dense.c: orc_llt_compute,
orc_ldlt_no_pivot_compute and their solve_inplace routines) -- no tolerance anywhere except where the reference's own test (ldlt_test.cpp:22-77) sets one."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PQ_ERR_INVALID = -1
KINDS = ["llt", "ldlt"]
SIZES = [1, 4, 8, 31, 32, 33, 40, 64, 127, 128]


def upper_triangular_spd(n, seed, shift=1e-2):
    """a symmetric positive definite matrix of which only the UPPER triangle is kept (rand::dense_positive_definite_upper_triangular_rand, utils/random_utils.hpp)"""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.standard_normal((n, n)), 1)
    S = U + U.T
    S += (shift + abs(np.linalg.eigvalsh(S).min())) * np.eye(n)
    return np.triu(S), S


def is_approx(a, b, prec):
    """Eigen's isApprox: |a - b| <= prec * min(|a|, |b|) in the Euclidean norm"""
    return np.linalg.norm(a - b) <= prec * min(np.linalg.norm(a), np.linalg.norm(b))


def batch_size(n):
    return 67 if n >= 32 else 1031  # 1031: more workgroups than compute units, and no multiple of the matrices a workgroup holds


@functools.lru_cache(maxsize=None)
def spd_batch(n, batch, seed0=0):
    """[batch, n, n] symmetric positive definite, every matrix different (shared by the tests, never modified)"""
    S = np.stack([upper_triangular_spd(n, seed0 + 7919 * n + i)[1] for i in range(batch)])
    S.setflags(write=False)
    return S


def orc_factor(orc, kind, S):
    """(return value, lower triangle left behind) of orc_llt_compute / orc_ldlt_no_pivot_compute on the full symmetric S"""
    n = S.shape[0]
    a = np.asfortranarray(np.array(S, dtype=np.float64))
    if kind == "llt":
        ret = orc.lib().orc_llt_compute(a.ctypes.data_as(orc._dp), n, n)
    else:
        w = np.zeros(n)
        ret = orc.lib().orc_ldlt_no_pivot_compute(a.ctypes.data_as(orc._dp), n, n, w.ctypes.data_as(orc._dp))
    return ret, np.tril(a)


def orc_solve(orc, kind, Lo, b):
    n = Lo.shape[0]
    a = np.asfortranarray(Lo)
    x = np.array(b, dtype=np.float64)
    fn = orc.lib().orc_llt_solve_inplace if kind == "llt" else orc.lib().orc_ldlt_no_pivot_solve_inplace
    fn(a.ctypes.data_as(orc._dp), n, n, x.ctypes.data_as(orc._dp))
    return x


@functools.lru_cache(maxsize=None)
def _oracle_factors(kind, n, batch):
    from oracle import pyorc
    out = []
    for S in spd_batch(n, batch):
        ret, Lo = orc_factor(pyorc, kind, S)
        assert ret == -1
        out.append(Lo)
    return out


def make(hip, kind, *args, **kw):
    return (hip.BatchLLT if kind == "llt" else hip.BatchLDLTNoPivot)(*args, **kw)


def stored(f, kind, i):
    return f.matrixLLT(i) if kind == "llt" else f.matrixLDLT(i)


# ---- 1. bitwise against the oracle
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_factor_of_the_batch_is_the_oracles_bit_for_bit(hip, orc, kind, n):
    batch = batch_size(n)
    S = spd_batch(n, batch)
    ref = _oracle_factors(kind, n, batch)
    f = make(hip, kind, batch, n).compute(S)
    assert f.n_success == batch
    assert not f.info().any() and (f.first_bad_col() == -1).all()
    wrong = [i for i in range(batch) if not np.array_equal(stored(f, kind, i), ref[i])]
    assert wrong == []
    # a batch of one
    one = make(hip, kind, 1, n).compute(S[batch - 1:])
    assert one.n_success == 1 and np.array_equal(stored(one, kind, 0), ref[batch - 1])


# ---- 2. both triangles
@pytest.mark.parametrize("n", [8, 31, 40, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_upper_is_lower_transposed(hip, kind, n):
    batch = 6
    S = spd_batch(n, batch, 1)
    lo = make(hip, kind, batch, n, hip.LOWER).compute(np.tril(S))
    up = make(hip, kind, batch, n, hip.UPPER).compute(np.triu(S))
    assert lo.n_success == batch and up.n_success == batch
    for i in range(batch):
        ml, mu = stored(lo, kind, i), stored(up, kind, i)
        assert np.array_equal(mu, ml.T)
        assert np.array_equal(np.triu(ml, 1), np.zeros((n, n))) and np.array_equal(np.tril(mu, -1), np.zeros((n, n)))
        assert np.array_equal(up.matrixU(i), lo.matrixL(i).T)


# ---- 3. only the named triangle, only the matrix
@pytest.mark.parametrize("uplo", ["lower", "upper"])
@pytest.mark.parametrize("n", [8, 40])
@pytest.mark.parametrize("kind", KINDS)
def test_device_input_with_padding_gaps_and_nan_everywhere_else(hip, kind, n, uplo):
    import torch
    batch, nrhs = 7, 3
    lda = n + 5
    stride = lda * n + 11
    S = spd_batch(n, batch, 2)
    UPLO = hip.LOWER if uplo == "lower" else hip.UPPER
    clean = make(hip, kind, batch, n, UPLO, max_nrhs=nrhs).compute(S)
    buf = np.full(batch * stride, np.nan)
    for i in range(batch):
        blk = buf[i * stride:i * stride + lda * n].reshape(n, lda)  # blk[c, r] = element (r, c) of the column-major matrix
        T = np.tril(S[i]) if uplo == "lower" else np.triu(S[i])
        keep = np.tril(np.ones((n, n), bool)) if uplo == "lower" else np.triu(np.ones((n, n), bool))
        blk[:, :n] = np.where(keep, T, np.nan).T
    t = torch.from_numpy(buf).cuda()
    f = make(hip, kind, batch, n, UPLO, max_nrhs=nrhs).compute_colmajor(t, lda=lda, stride=stride)
    assert f.n_success == batch
    for i in range(batch):
        assert np.array_equal(stored(f, kind, i), stored(clean, kind, i))
    assert np.array_equal(t.cpu().numpy().view(np.int64), buf.view(np.int64))  # the input is only read
    # solve in place on the device: right-hand sides with padding rows and a gap between blocks, canaries behind the last block
    ldx = n + 3
    xstride = ldx * nrhs + 7
    ncanary = 16
    xb = np.full((batch - 1) * xstride + ldx * nrhs + ncanary, np.nan)
    xb[-ncanary:] = 12345.0 + np.arange(ncanary)
    B = np.random.default_rng(4).standard_normal((batch, nrhs, n))
    for i in range(batch):
        xb[i * xstride:i * xstride + ldx * nrhs].reshape(nrhs, ldx)[:, :n] = B[i]
    before = xb.copy()
    xt = torch.from_numpy(xb).cuda()
    f.solveInPlace(xt.data_ptr(), nrhs=nrhs, ldx=ldx, stride=xstride, on_device=True)
    after = xt.cpu().numpy()
    assert np.array_equal(after[-ncanary:], before[-ncanary:])
    want = clean.solve(B)
    mask = np.zeros(after.shape, bool)
    for i in range(batch):
        got = after[i * xstride:i * xstride + ldx * nrhs].reshape(nrhs, ldx)[:, :n]
        assert np.array_equal(got, want[i])
        mask[i * xstride:i * xstride + ldx * nrhs].reshape(nrhs, ldx)[:, :n] = True
    assert np.array_equal(after.view(np.int64)[~mask], before.view(np.int64)[~mask])  # padding rows, gaps and canaries: untouched


# ---- 4. failures stay private
def test_llt_failures_stay_private(hip, orc):
    batch, n = 9, 40
    S = np.array(spd_batch(n, batch, 3))
    S[2, 17, 17] = -S[2, 17, 17]
    S[7, 0, 0] = -S[7, 0, 0]
    ref = [orc_factor(orc, "llt", S[i]) for i in range(batch)]
    assert [r[0] >= 0 for r in ref] == [i in (2, 7) for i in range(batch)]
    f = hip.BatchLLT(batch, n, max_nrhs=2)
    assert f.compute(S).n_success == 7
    assert f.info().tolist() == [1 if i in (2, 7) else 0 for i in range(batch)]
    assert f.first_bad_col().tolist() == [r[0] for r in ref]
    for i in range(batch):
        if i not in (2, 7):
            assert np.array_equal(f.matrixLLT(i), ref[i][1])
    B = np.random.default_rng(5).standard_normal((batch, 2, n))
    X = f.solve(B)
    for i in range(batch):
        if i in (2, 7):
            assert np.array_equal(X[i], B[i])
        else:
            for c in range(2):
                assert np.array_equal(X[i, c], orc_solve(orc, "llt", ref[i][1], B[i, c]))
    # the same handle, healthy data
    good = spd_batch(n, batch, 3)
    assert f.compute(good).n_success == batch and not f.info().any()
    for i in range(batch):
        assert np.array_equal(f.matrixLLT(i), orc_factor(orc, "llt", good[i])[1])


def test_ldlt_no_pivot_fails_on_an_exact_zero_pivot_only(hip, orc):
    """ldlt_no_pivot.hpp:307: a quasi-definite matrix is factored with its negative pivots kept; only an exact zero pivot is a NumericalIssue"""
    nh, p = 25, 15
    n, batch = nh + p, 5
    rng = np.random.default_rng(6)
    K = []
    for i in range(batch):
        H = upper_triangular_spd(nh, 900 + i)[1]
        A = rng.standard_normal((p, nh))
        K.append(np.block([[H, A.T], [A, -np.eye(p)]]))
    K = np.stack(K)
    K[3, 0, 0] = 0.0  # an exact zero leading pivot
    ref = [orc_factor(orc, "ldlt", K[i]) for i in range(batch)]
    assert [r[0] for r in ref] == [-1, -1, -1, 0, -1]
    f = hip.BatchLDLTNoPivot(batch, n)
    assert f.compute(K).n_success == batch - 1
    assert f.info().tolist() == [0, 0, 0, 1, 0] and f.first_bad_col().tolist() == [-1, -1, -1, 0, -1]
    for i in (0, 1, 2, 4):
        assert np.array_equal(f.matrixLDLT(i), ref[i][1])
        d = f.vectorD(i)
        assert (d[:nh] > 0).all() and (d[nh:] < 0).all()
    B = rng.standard_normal((batch, n))
    X = f.solve(B)
    assert np.array_equal(X[3], B[3])
    for i in (0, 1, 2, 4):
        assert np.array_equal(X[i], orc_solve(orc, "ldlt", ref[i][1], B[i]))
        assert is_approx(B[i], K[i] @ X[i], 1e-8)
    assert hip.BatchLLT(batch, n).compute(K).n_success == 0
    K[3, 0, 0] = 1.0
    assert f.compute(K).n_success == batch


# ---- 5. solves
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("nrhs", [1, 3, 17])
@pytest.mark.parametrize("n", [8, 33, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_every_solution_column_is_the_oracles_bit_for_bit(hip, orc, kind, n, nrhs, mem):
    batch = 5
    S = spd_batch(n, batch, 4)
    ref = [orc_factor(orc, kind, S[i])[1] for i in range(batch)]
    f = make(hip, kind, batch, n, max_nrhs=17).compute(S)
    assert f.n_success == batch
    ldx = n + 3
    B = np.random.default_rng(n + nrhs).standard_normal((batch, nrhs, n))
    X = np.full((batch, nrhs, ldx), 3.25)
    X[:, :, :n] = B
    if mem == "device":
        import torch
        Xt = torch.from_numpy(X).cuda()
        f.solveInPlace(Xt)
        X = Xt.cpu().numpy()
    else:
        f.solveInPlace(X)
    assert (X[:, :, n:] == 3.25).all()
    for i in range(batch):
        for c in range(nrhs):
            assert np.array_equal(X[i, c, :n], orc_solve(orc, kind, ref[i], B[i, c])), (i, c)


@pytest.mark.parametrize("uplo", ["lower", "upper"])
def test_ldlt_test_cpp_solve_for_every_matrix_of_a_batch(hip, uplo):
    """ldlt_test.cpp:22-49 (SolveLower) / :51-77 (SolveUpper), dim = 50: compute twice, info() == Success, b.isApprox(P_full * x, 1e-8)"""
    dim, batch = 50, 6
    pairs = [upper_triangular_spd(dim, 40 + i) for i in range(batch)]
    P = np.stack([p[0] for p in pairs])
    if uplo == "lower":
        P = np.ascontiguousarray(P.transpose(0, 2, 1))  # P.transposeInPlace()
    ldlt = hip.BatchLDLTNoPivot(batch, dim, hip.LOWER if uplo == "lower" else hip.UPPER)
    ldlt.compute(P)
    assert not ldlt.info().any()
    ldlt.compute(P)
    assert not ldlt.info().any()
    b = np.random.default_rng(8).standard_normal((batch, dim))
    x = b.copy()
    ldlt.solveInPlace(x)
    for i in range(batch):
        assert is_approx(b[i], pairs[i][1] @ x[i], 1e-8)


def test_solve_argument_checks(hip):
    n, batch = 8, 3
    L = hip._lib.load()
    f = hip.BatchLLT(batch, n, max_nrhs=2)
    x = np.zeros((batch, 3, n))
    assert L.pq_dense_factor_batch_solve_in_place(f.h, x.ctypes.data, n, 1, n, 0) == PQ_ERR_INVALID  # before any compute
    assert "before compute" in L.pq_last_error_string().decode()
    info = np.zeros(batch, dtype=np.int32)
    assert L.pq_dense_factor_batch_info(f.h, info.ctypes.data, None) == PQ_ERR_INVALID
    f.compute(spd_batch(n, batch, 5))
    assert L.pq_dense_factor_batch_info(f.h, info.ctypes.data, None) == 0  # first_bad_col is nullable
    assert L.pq_dense_factor_batch_solve_in_place(f.h, x.ctypes.data, n, 3, 3 * n, 0) == PQ_ERR_INVALID  # nrhs > max_nrhs
    assert L.pq_dense_factor_batch_solve_in_place(f.h, x.ctypes.data, n - 1, 1, n, 0) == PQ_ERR_INVALID  # ldx < n
    assert L.pq_dense_factor_batch_solve_in_place(f.h, x.ctypes.data, n, 2, 2 * n, 0) == 0


# ---- 6. no allocation after create
@pytest.mark.parametrize("kind", KINDS)
def test_no_allocation_after_create(hip, kind):
    import torch
    L = hip._lib.load()
    n, batch, nrhs = 40, 9, 3
    S = spd_batch(n, batch, 3)
    St = torch.from_numpy(np.array(S)).cuda()
    Xt = torch.zeros((batch, nrhs, n), dtype=torch.float64, device="cuda") + 1.0
    f = make(hip, kind, batch, n, max_nrhs=nrhs)
    before = L.pq_debug_alloc_count()
    for _ in range(2):
        f.compute(S)
        f.info(); f.first_bad_col()
        f.solve(np.ones((batch, nrhs, n)))
        stored(f, kind, batch - 1)
        f.compute_colmajor(St)
        f.solveInPlace(Xt)
        stored(f, kind, 0)
        f.last_ms()
    assert L.pq_debug_alloc_count() == before
    dev_ms, wall_ms = f.last_ms()
    assert 0.0 < dev_ms <= wall_ms


# ---- 7. determinism
@pytest.mark.parametrize("n", [31, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_two_computes_give_the_same_bits(hip, kind, n):
    batch = 67
    S = spd_batch(n, batch)
    f = make(hip, kind, batch, n).compute(S)
    first = [stored(f, kind, i) for i in range(batch)]
    f.compute(S)
    assert all(np.array_equal(stored(f, kind, i), first[i]) for i in range(batch))
