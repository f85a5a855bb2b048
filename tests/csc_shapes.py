"""Shapes and the plain reference for the CSC mat-vec layer under every sparse backend (piqp_amd/csrc/sparse_ops.hip, CscOperators).

A shape is built from COLUMN-LENGTH PROFILES, each the smallest that reaches one branch of the wave-cooperative column dot (wave_col_dot: 64 columns per wave, streamed
through LDS in chunks of DOT_CHUNK = 512 entries; columns above SPMV_LONG_COL = 2048 entries go to the tree-sum kernel in the default mode):

    GT (n x m)  carries the profile on its own columns        -> k_recover_duals and k_spmv_cols<false> meet it on GT,
    A  (p x n)  carries the profile on ITS columns, AT = A'   -> k_fold_rhs, k_spmv_cols<true> and k_spmv_cols<false> meet it on the transposed copy the library derives,

so n is at least the longest column and the profile of A is padded with empty columns up to n.  AT (from A) and G (from GT) come out with short columns.  P_utri has a
diagonal (absent in a few columns), a few entries above it and, where asked for, an arrow column that gives the symmetrised copy Pf one long column.

The reference restates every kernel as a plain Python loop over Python floats: one rounded product and one rounded add per term, in the order the kernel's comment
documents.  sparse_ops.hip is built with -ffp-contract=off, so the device results are these values bit for bit (tests/test_csc_ops_gpu.py); tests/test_csc_shapes.py
holds the reference itself against the oracle and checks that every branch is reached and that the summation order shows in the bits.
"""
import numpy as np

DOT_CHUNK = 512       # sparse_ops.hip
SPMV_LONG_COL = 2048  # sparse_ops.hip
WAVE = 64
N_VEC = 4
ALPHAS = (-1.5, 0.7)  # (alpha_n, alpha_t) of the eval_* comparisons
SENTINEL = -7.25e77   # what the tests pre-fill outputs with: no product of the data below comes near it


# ------------------------------------------------------------------------------------------------------------------------------------------------- generator
def _values(rng, cnt):
    """+-10**U(-3, 3): magnitudes six decades apart, so the order of a sum shows in its bits"""
    return np.where(rng.random(cnt) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3.0, 3.0, cnt)


def csc_from_lengths(rows, lens, rng):
    """CSC (colptr, rowind, val) with len(lens) columns; column j has min(lens[j], rows) distinct ascending rows"""
    cp = [0]
    ri = []
    for ln in lens:
        ln = min(int(ln), rows)
        ri.append(np.sort(rng.choice(rows, ln, replace=False)).astype(np.int32) if ln else np.zeros(0, np.int32))
        cp.append(cp[-1] + ln)
    ri = np.concatenate(ri) if ri else np.zeros(0, np.int32)
    return np.asarray(cp, np.int32), ri.astype(np.int32), _values(rng, cp[-1])


def transpose_csc(rows, cols, cp, ri, val):
    """(colptr, rowind, val, tmap) of the transpose; entries of a column ascending by row (= CscOperators' transpose_with_map); tmap[q_in_T] = q_in_M"""
    nnz = int(cp[cols])
    tp = np.zeros(rows + 1, np.int64)
    for q in range(nnz):
        tp[ri[q] + 1] += 1
    tp = np.cumsum(tp)
    nx = tp[:-1].copy()
    ti = np.zeros(nnz, np.int32); tm = np.zeros(nnz, np.int64)
    for j in range(cols):
        for q in range(cp[j], cp[j + 1]):
            t = nx[ri[q]]; nx[ri[q]] += 1
            ti[t] = j; tm[t] = q
    return tp.astype(np.int32), ti, np.asarray(val)[tm] if nnz else np.zeros(0), tm


def _p_utri(n, rng, arrow=0, no_diag=(), dup_diag=()):
    """upper triangle: up to 8 entries above the diagonal per column (the reference-order product splits a symmetrised column into the sum above the diagonal and the
    rest, and each part needs 3 terms or more before its order shows), the diagonal last (twice in dup_diag columns, absent in no_diag ones); the LAST column is an
    arrow with `arrow` entries above the diagonal"""
    cp = [0]; ri = []
    for j in range(n):
        k = min(j, int(rng.integers(0, 9)))
        if arrow and j == n - 1:
            k = min(j, arrow)
        r = list(np.sort(rng.choice(j, k, replace=False))) if k else []
        if j not in no_diag:
            r.append(j)
            if j in dup_diag:
                r.append(j)
        ri += r
        cp.append(cp[-1] + len(r))
    val = _values(rng, cp[-1])
    return np.asarray(cp, np.int32), np.asarray(ri, np.int32), val


def symmetrise(n, cp, ri):
    """(colptr, rowind, src) of Pf as CscOperators::init builds it: column j lists first the stored upper entries of column j in stored order, then the mirrored
    entries (row j of the columns to its right) by ascending column; src = position in P_utri"""
    cnt = np.zeros(n + 1, np.int64)
    for j in range(n):
        for q in range(cp[j], cp[j + 1]):
            cnt[j + 1] += 1
            if ri[q] != j:
                cnt[ri[q] + 1] += 1
    fp = np.cumsum(cnt)
    nx = fp[:-1].copy()
    fi = np.zeros(fp[n], np.int32); src = np.zeros(fp[n], np.int64)
    for j in range(n):
        for q in range(cp[j], cp[j + 1]):
            t = nx[j]; nx[j] += 1
            fi[t] = ri[q]; src[t] = q
    for j in range(n):
        for q in range(cp[j], cp[j + 1]):
            i = ri[q]
            if i != j:
                t = nx[i]; nx[i] += 1
                fi[t] = j; src[t] = q
    return fp.astype(np.int32), fi, src


class Shape:
    """one problem: P_utri (n x n upper), AT (n x p), GT (n x m) as raw CSC arrays, a second set of values on the same patterns, and the vectors every test uses"""

    def __init__(self, name, n, p, m, lens_A, lens_GT, seed, arrow=0, no_diag=(), dup_diag=(), oracle=True):
        rng = np.random.default_rng(seed)
        self.name, self.n, self.p, self.m, self.seed, self.oracle = name, n, p, m, seed, oracle
        lens_A = list(lens_A) + [0] * (n - len(lens_A))
        assert len(lens_A) == n and len(lens_GT) == m
        self.P = _p_utri(n, rng, arrow, no_diag, dup_diag)
        A = csc_from_lengths(p, lens_A, rng) if p else (np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
        self.AT = transpose_csc(p, n, *A)[:3] if p else (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
        self.GT = csc_from_lengths(n, lens_GT, rng) if m else (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
        self.val2 = tuple(_values(rng, len(M[2])) for M in (self.P, self.AT, self.GT))
        v = lambda k: rng.standard_normal(k) * 10.0 ** rng.uniform(-1.0, 1.0, k)
        # N_VEC operand vectors for the three eval_*: reversing a sum of 3 to 6 such terms changes its bits in only 20 to 50 % of the cases, so one vector would
        # leave most short columns unable to tell the order; under four, more than half of the rows with 3 or more entries do (tests/test_csc_shapes.py asserts it)
        self.xs, self.ys, self.zs = [v(n) for _ in range(N_VEC)], [v(p) for _ in range(N_VEC)], [v(m) for _ in range(N_VEC)]
        self.x, self.y, self.z = self.xs[0], self.ys[0], self.zs[0]
        self.rhs_x, self.rhs_y, self.rhs_z = v(n), v(p), v(m)
        self.x_reg, self.z_reg = rng.uniform(0.5, 2.0, n), rng.uniform(0.1, 3.0, m)
        self.zinv = 1.0 / self.z_reg
        self.delta = 1.2
        self.delta_inv = 1.0 / self.delta
        self._copies = {}

    @classmethod
    def from_matrices(cls, name, n, p, m, P_utri, AT, GT):
        """the matrices of an existing problem (scipy CSC, sorted rows) for the reference functions; no vectors, no second values"""
        sh = object.__new__(cls)
        sh.name, sh.n, sh.p, sh.m, sh.oracle = name, n, p, m, True
        sh.P, sh.AT, sh.GT = ((np.asarray(M.indptr, np.int32), np.asarray(M.indices, np.int32), np.asarray(M.data, np.float64)) for M in (P_utri, AT, GT))
        sh._copies = {}
        return sh

    def with_values(self, second):
        """the three matrices with the first or the second set of values"""
        if not second:
            return self.P, self.AT, self.GT
        return tuple((M[0], M[1], v) for M, v in zip((self.P, self.AT, self.GT), self.val2))

    def copies(self, second=False):
        """the five device copies as CscOperators holds them: dict name -> (ncols, colptr, rowind, val) with Pf, AT, A, GT, G"""
        if second not in self._copies:
            P, AT, GT = self.with_values(second)
            fp, fi, src = symmetrise(self.n, P[0], P[1])
            A = transpose_csc(self.n, self.p, *AT)[:3]
            G = transpose_csc(self.n, self.m, *GT)[:3]
            c = {"Pf": (self.n, fp, fi, P[2][src] if len(src) else np.zeros(0)), "AT": (self.p,) + tuple(AT), "A": (self.n,) + A, "GT": (self.m,) + tuple(GT), "G": (self.n,) + G}
            self._copies[second] = {k: (nc, [int(a) for a in cp], [int(a) for a in ri], [float(a) for a in vv]) for k, (nc, cp, ri, vv) in c.items()}
        return self._copies[second]


def _edge_lens(ncols, rng):
    lens = rng.integers(0, 7, ncols)
    if ncols == 321:
        lens[[0, 63, 64, 320]] = 0
        lens[128:192] = 0  # an empty wave
    return lens


def _straddle_lens(rng):
    # wave 0: 63 columns of 509 entries together, then one of 7 entries that starts at entry 509 of the wave's range and crosses the chunk boundary at 512
    w0 = [9] * 5 + [8] * 58 + [7]
    assert sum(w0[:63]) == 509 and len(w0) == 64
    # wave 1: 512 entries from the chunk boundary on; then 3 + 100 entries, so the 1300-entry column starts at 615 (mid-chunk) and ends at 1915: chunks 1, 2 and 3
    w1 = [512, 3, 100, 1300] + list(rng.integers(0, 7, 60))
    return w0 + w1 + [5, 2]  # 130 columns


def _long_lens(rng):
    lens = list(rng.integers(1, 7, 70))
    lens[0] = 2600   # first in its wave
    lens[10] = 2048  # the last length on the wave path
    lens[20] = 2049  # the first on the tree path
    lens[30] = 2304  # 9 x 256: every thread of the tree kernel sums 9 terms
    lens[63] = 2305  # last in its wave; one thread sums a 10th term
    return lens


def _build_all():
    out = []
    for k, nc in enumerate((1, 63, 64, 65, 255, 256, 257, 321)):
        rng = np.random.default_rng(100 + nc)
        out.append(Shape(f"edges_{nc}", nc, nc, nc, _edge_lens(nc, rng), _edge_lens(nc, rng), seed=200 + nc, no_diag=(0, nc // 2) if nc > 1 else ()))
    out.append(Shape("full_chunk_64", 64, 64, 64, [8] * 64, [8] * 64, seed=11))
    out.append(Shape("full_chunk_65", 65, 65, 65, [8] * 64 + [1], [8] * 64 + [1], seed=12))
    rng = np.random.default_rng(13)
    out.append(Shape("straddle", 1400, 1400, 130, _straddle_lens(rng), _straddle_lens(rng), seed=14, arrow=600))
    rng = np.random.default_rng(15)
    out.append(Shape("long", 2700, 2700, 70, _long_lens(rng), _long_lens(rng), seed=16, arrow=2100))
    rng = np.random.default_rng(17)
    out.append(Shape("absent_p", 130, 0, 70, [], rng.integers(0, 7, 70), seed=18))
    out.append(Shape("absent_m", 130, 70, 0, rng.integers(0, 7, 130), [], seed=19))
    # the oracle's KKT assembly expects distinct rows in a column of P_utri, so the column that lists its diagonal twice stays out of the oracle comparison
    out.append(Shape("absent_pm_dup_diag", 70, 0, 0, [], [], seed=20, no_diag=(3,), dup_diag=(5, 69), oracle=False))
    return out


_ALL = None


def all_shapes():
    """built once per process and shared: nobody writes to a Shape"""
    global _ALL
    if _ALL is None:
        _ALL = _build_all()
    return _ALL


def shape(name):
    return next(s for s in all_shapes() if s.name == name)


# -------------------------------------------------------------------------------------------------------------------------------------------------- branches
KERNEL_COPIES = {  # which device copies each instantiation of wave_col_dot runs on
    "k_spmv_cols<false>": ("Pf", "AT", "A", "GT", "G"),  # default mode (max_len = SPMV_LONG_COL); reference-order mode on AT and GT (max_len = 0)
    "k_spmv_cols<true>": ("A", "G"),                     # reference-order mode, the scatter products
    "k_fold_rhs": ("G", "A"),
    "k_recover_duals": ("AT", "GT"),
}
BRANCHES = ("cnt==512", "exactly_one_full_chunk", "column_crosses_chunk", "column_over_3_chunks", "empty_wave", "ncols%64!=0", "long_column_in_streaming_wave")


def branches_of(ncols, cp):
    """the branches of wave_col_dot a matrix with this colptr reaches.  long_column_in_streaming_wave: a column of more than SPMV_LONG_COL entries in a wave
    that also holds shorter non-empty ones -- the wave streams it; k_spmv_cols in the default mode must not add it (it belongs to k_spmv_long_cols), the fold, the
    recovery and the reference-order products sum it in place."""
    hit = set()
    if ncols % WAVE:
        hit.add("ncols%64!=0")
    for j0 in range(0, ncols, WAVE):
        j1 = min(j0 + WAVE, ncols)
        wlo, whi = cp[j0], cp[j1]
        if whi == wlo:
            hit.add("empty_wave")
            continue
        if whi - wlo >= DOT_CHUNK:
            hit.add("cnt==512")
        if whi - wlo == DOT_CHUNK:
            hit.add("exactly_one_full_chunk")
        lens = [cp[j + 1] - cp[j] for j in range(j0, j1)]
        if max(lens) > SPMV_LONG_COL and any(0 < ln <= SPMV_LONG_COL for ln in lens):
            hit.add("long_column_in_streaming_wave")
        for j in range(j0, j1):
            lo, hi = cp[j], cp[j + 1]
            if hi > lo:
                chunks = (hi - 1 - wlo) // DOT_CHUNK - (lo - wlo) // DOT_CHUNK + 1
                if chunks >= 2:
                    hit.add("column_crosses_chunk")
                if chunks >= 3:
                    hit.add("column_over_3_chunks")
    return hit


# ------------------------------------------------------------------------------------------------------------------------------------------------- reference
def col_dot(M, j, op, reverse=False):
    """sum over column j of val[q] * op[row[q]], left to right (right to left with reverse): the statement of wave_col_dot and col_dot_seq"""
    _, cp, ri, v = M
    s = 0.0
    rng_ = range(cp[j + 1] - 1, cp[j] - 1, -1) if reverse else range(cp[j], cp[j + 1])
    for q in rng_:
        s += v[q] * op[ri[q]]
    return s


def col_tree(M, j, x, reverse=False):
    """k_spmv_long_cols: thread t sums the entries t, t + 256, ... of the column in order, then the 256 partial sums are halved in a fixed tree"""
    _, cp, ri, v = M
    qs = list(range(cp[j], cp[j + 1]))
    if reverse:
        qs.reverse()
    part = [0.0] * 256
    for t in range(256):
        s = 0.0
        for q in qs[t::256]:
            s += v[q] * x[ri[q]]
        part[t] = s
    w = 128
    while w > 0:
        for t in range(w):
            part[t] += part[t + w]
        w >>= 1
    return part[0]


def spmv(M, x, alpha, ref_order=False, scatter=False, reverse=False):
    """CscOperators' spmv(): default mode alpha * S with the long columns on the tree; reference-order mode alpha * S or, scatter, the sum of val * (alpha x)"""
    ncols = M[0]
    x = [float(a) for a in x]
    y = np.zeros(ncols)
    if ref_order and scatter:
        ax = [alpha * a for a in x]
        for j in range(ncols):
            y[j] = col_dot(M, j, ax, reverse)
        return y
    for j in range(ncols):
        if not ref_order and M[1][j + 1] - M[1][j] > SPMV_LONG_COL:
            y[j] = alpha * col_tree(M, j, x, reverse)
        else:
            y[j] = alpha * col_dot(M, j, x, reverse)
    return y


def eval_P_x(sh, alpha, x, ref_order=False, second=False, reverse=False):
    Pf = sh.copies(second)["Pf"]
    if not ref_order:
        return spmv(Pf, x, alpha, reverse=reverse)
    # k_sym_spmv_ref: row r collects val * (alpha x_j) over the entries at or right of the diagonal and alpha * (sum of val * x_i over those above it)
    n, cp, ri, v = Pf
    x = [float(a) for a in x]
    z = np.zeros(n)
    for r in range(n):
        acc = 0.0; s = 0.0
        qs = range(cp[r + 1] - 1, cp[r] - 1, -1) if reverse else range(cp[r], cp[r + 1])
        for q in qs:
            i = ri[q]
            if i < r:
                s += v[q] * x[i]
            else:
                acc += v[q] * (alpha * x[i])
        z[r] = acc + alpha * s
    return z


def eval_A(sh, an, at, xn, xt, ref_order=False, second=False, reverse=False):
    """(zn = an A xn [p], zt = at A' xt [n])"""
    c = sh.copies(second)
    return spmv(c["AT"], xn, an, ref_order, False, reverse), spmv(c["A"], xt, at, ref_order, True, reverse)


def eval_G(sh, an, at, xn, xt, ref_order=False, second=False, reverse=False):
    c = sh.copies(second)
    return spmv(c["GT"], xn, an, ref_order, False, reverse), spmv(c["G"], xt, at, ref_order, True, reverse)


def evals(sh, ref_order, second=False, reverse=False, k=0):
    """the three eval_* on operand vectors k with ALPHAS: (P x, (A x, A' y), (G x, G' z))"""
    an, at = ALPHAS
    return (eval_P_x(sh, an, sh.xs[k], ref_order, second, reverse), eval_A(sh, an, at, sh.xs[k], sh.ys[k], ref_order, second, reverse),
            eval_G(sh, an, at, sh.xs[k], sh.zs[k], ref_order, second, reverse))


def fold_rhs(sh, with_A, with_G, ref_order=False, second=False, reverse=False):
    """k_fold_rhs: (rhs_x + S_G) + delta_inv * S_A with the operand zinv[i] * rhs_z[i] under G; k_fold_rhs_ref: the terms added INTO rhs_x one after the other, first
    G(i, j) (zinv_i rhs_z_i), then A(i, j) (delta_inv rhs_y_i).  No column is ever split."""
    c = sh.copies(second)
    G, A = c["G"], c["A"]
    di = sh.delta_inv
    zr = [float(a) * float(b) for a, b in zip(sh.zinv, sh.rhs_z)]
    ry = [float(a) for a in sh.rhs_y]
    out = np.zeros(sh.n)
    if ref_order:
        dy = [di * a for a in ry]
        for j in range(sh.n):
            s = float(sh.rhs_x[j])
            if with_G:
                for q in range(G[1][j], G[1][j + 1]):
                    s += G[3][q] * zr[G[2][q]]
            if with_A:
                for q in range(A[1][j], A[1][j + 1]):
                    s += A[3][q] * dy[A[2][q]]
            out[j] = s
        return out
    for j in range(sh.n):
        sg = col_dot(G, j, zr, reverse) if with_G else 0.0
        sa = col_dot(A, j, ry, reverse) if with_A else 0.0
        out[j] = (float(sh.rhs_x[j]) + sg) + di * sa
    return out


def recover_duals(sh, x, second=False, reverse=False, rhs_y=None, rhs_z=None, zinv=None, delta_inv=None):
    """k_recover_duals: lhs_y = delta_inv * S - delta_inv * rhs_y, lhs_z = (S - rhs_z) * zinv (the same statements in both modes)"""
    c = sh.copies(second)
    rhs_y = sh.rhs_y if rhs_y is None else rhs_y
    rhs_z = sh.rhs_z if rhs_z is None else rhs_z
    zinv = sh.zinv if zinv is None else zinv
    di = sh.delta_inv if delta_inv is None else delta_inv
    x = [float(a) for a in x]
    ly, lz = np.zeros(sh.p), np.zeros(sh.m)
    for k in range(sh.p):
        ly[k] = di * col_dot(c["AT"], k, x, reverse) - di * float(rhs_y[k])
    for i in range(sh.m):
        lz[i] = (col_dot(c["GT"], i, x, reverse) - float(rhs_z[i])) * float(zinv[i])
    return ly, lz


def residual(sh, lx, ly, lz, second=False):
    """k_residual_rows on every row = the statements of k_err_x / k_err_yz: err_x = rhs_x - ((((P x) + x_reg x) + A' y) + G' z), err_y = rhs_y - (A x - delta y),
    err_z = rhs_z - (G x - z_reg z), every column sum left to right"""
    c = sh.copies(second)
    lx = [float(a) for a in lx]; ly = [float(a) for a in ly]; lz = [float(a) for a in lz]
    ex, ey, ez = np.zeros(sh.n), np.zeros(sh.p), np.zeros(sh.m)
    for i in range(sh.n):
        v = 1.0 * col_dot(c["Pf"], i, lx)
        v += float(sh.x_reg[i]) * lx[i]
        v += 1.0 * col_dot(c["A"], i, ly) if sh.p else 0.0
        v += 1.0 * col_dot(c["G"], i, lz) if sh.m else 0.0
        ex[i] = float(sh.rhs_x[i]) - v
    for j in range(sh.p):
        v = 1.0 * col_dot(c["AT"], j, lx)
        v -= sh.delta * ly[j]
        ey[j] = float(sh.rhs_y[j]) - v
    for k in range(sh.m):
        v = 1.0 * col_dot(c["GT"], k, lx)
        v -= float(sh.z_reg[k]) * lz[k]
        ez[k] = float(sh.rhs_z[k]) - v
    return ex, ey, ez


def p_diag(sh, second=False):
    """the LAST diagonal entry a column of P_utri lists, 0 where it lists none"""
    cp, ri, v = sh.with_values(second)[0]
    d = np.zeros(sh.n)
    for j in range(sh.n):
        for q in range(cp[j], cp[j + 1]):
            if ri[q] == j:
                d[j] = v[q]
    return d


def bits(a):
    """the bit patterns of a float64 array (what every comparison of these tests is made on)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
