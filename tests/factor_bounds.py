"""Inputs, statistics and bounds of tests/test_dense_factor_componentwise_gpu.py, shared with tests/workers/dense_sweeps.py (which runs the sweep check in a
fresh process under a PIQP_AMD_DEBUG schedule).  The derivation of every constant is in the docstring of the test module; nothing here is measured on a device."""
import numpy as np

U = 2.0 ** -53
NB, PIECE = 128, 16
# what the derivation assumes of the inputs, asserted on the CPU for every shape and recipe and again on the device's own factor: the growth of the explicitly
# inverted 16 x 16 pieces / 128 x 128 blocks, i.e. how much larger |D| |D^-1| |D| is than |D| where it enters the statistic.  An off-diagonal entry (c, d) of
# |D| |D^-1| |D| holds |D_cd| three times to first order (through D_dd D^-1_dd, D_dd D^-1_cd D_cc and D^-1_cc D_cc), a diagonal one once: 3 is the value of a piece with
# small off-diagonal entries; 5 and 4 leave 2 and 1 for the second-order terms of these inputs (the sweeps' figure is taken against s, which also holds |b|)
K16, K128 = 5.0, 4.0


def gamma(k):
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------------------------------------------------------------------------- inputs
def factor_input(n, generation=0):
    """(Pf, x_regs): Pf = B^T B / n with B standard normal n x n (dense, condition number of order 10 with the 0.5 added, off-diagonal entries of L of order
    n^-1/2), two regularisations: the constant 0.5 and a second one in (0.5, 1)"""
    rng = np.random.default_rng([n, generation])
    B = rng.standard_normal((n, n))
    C = B.T @ B / n
    Pf = np.triu(C) + np.triu(C, 1).T
    return Pf, [np.full(n, 0.5), rng.uniform(0.5, 1.0, n)]


def sweep_input(n):
    """(Pf, x_reg) with K = Pf + diag(x_reg) = diag(d) + V V^T, d ~ U(1, 2), V = 8^-1/2 x standard normal n x 8: O(n^2) to form, and its L is fully dense (a banded or
    sparse L would hide a wrong index: zero times the wrong x is still zero)"""
    rng = np.random.default_rng([n, 7])
    d0 = rng.uniform(0.5, 1.5, n)
    V = rng.standard_normal((n, 8)) * 8.0 ** -0.5
    C = V @ V.T
    Pf = np.triu(C) + np.triu(C, 1).T
    Pf[np.diag_indices(n)] += d0
    return Pf, np.full(n, 0.5)


def right_hand_sides(n):
    """four right-hand sides; the fifth solve repeats the first"""
    rng = np.random.default_rng([n, 11])
    return [rng.standard_normal(n) * s for s in (1.0, 3.0, 0.01, 1.0)]


def data_of(hip, Pf):
    return hip.Data(Pf, np.zeros(Pf.shape[0]))


def full_from_lower(Kl):
    return np.tril(Kl) + np.tril(Kl, -1).T


def split_factor(F, ldlt):
    """(L, d): Cholesky: L = tril(F), d None; L D L^T: unit lower L and d = diag(F)"""
    L = np.tril(F)
    if not ldlt:
        return L, None
    d = np.diag(L).copy()
    np.fill_diagonal(L, 1.0)
    return L, d


def ldlt_of_cholesky(C):
    """the L D L^T factor (as F: D on the diagonal, unit L below) that belongs to a Cholesky factor C"""
    dg = np.diag(C)
    F = C / dg
    np.fill_diagonal(F, dg * dg)
    return F


# ---------------------------------------------------------------------------------------------------------------------------------- factor
def factor_statistic(K, F, ldlt, dtype=np.float64):
    """(R, S) = (K - L D L^T, |L| |D| |L|^T) (D = I for Cholesky), formed in `dtype`"""
    L, d = split_factor(F, ldlt)
    L = L.astype(dtype, copy=False)
    Ld = L if d is None else L * d.astype(dtype)
    R = K.astype(dtype, copy=False) - Ld @ L.T
    aL = np.abs(L)
    S = (aL if d is None else aL * np.abs(d).astype(dtype)) @ aL.T
    return R, S


def factor_device_part(n):
    """per column (0-based j, q = j + 1 terms): gamma_(q + 4), the factorisation's own sum"""
    return gamma(np.arange(1, n + 1) + 4.0)


def factor_host_part(n):
    """per column: gamma_(q + 2), forming K - L D L^T in fp64"""
    return gamma(np.arange(1, n + 1) + 2.0)


def off_block(n):
    """entries whose row lies in a later 128-block than their column: solved with the inverted 16 x 16 pieces (k_trsm_panel, panel_follow)"""
    b = np.arange(n) // NB
    return b[:, None] > b[None, :]


def factor_bound(n):
    """c_ij of the lower triangle (an n x n array; the upper triangle is not meant)"""
    c = np.broadcast_to(factor_device_part(n) + factor_host_part(n), (n, n)).copy()
    c[off_block(n)] += 2.0 * gamma(PIECE + 1) * K16
    return c


def factor_cap(n):
    return 8.0 * gamma(n + 1)


def piece_growth_matrix(D):
    """|D| |D^-1| |D| of a lower triangular piece"""
    a = np.abs(D)
    return a @ np.abs(np.linalg.inv(D)) @ a


def factor_growth(F, ldlt, S):
    """rho_16: max over the off-block entries (i, c) of (|X| M)_ic / S_ic, X = L D the panel before its scaling by 1 / D, M = blockdiag(|D_k|^T |D_k|^-T |D_k|^T) over
    the 16 x 16 diagonal pieces D_k of L: what the explicit inverses cost, relative to the statistic"""
    n = F.shape[0]
    L, d = split_factor(F, ldlt)
    X = np.abs(L) if d is None else np.abs(L) * np.abs(d)
    rho = 0.0
    for c0 in range(0, n, PIECE):
        c1 = min(n, c0 + PIECE)
        r0 = (c0 // NB + 1) * NB
        if r0 >= n:
            break
        M = piece_growth_matrix(L[c0:c1, c0:c1]).T
        rho = max(rho, float((X[r0:, c0:c1] @ M / S[r0:, c0:c1]).max()))
    return rho


def piece_conditions(F, ldlt, size):
    """the largest 2-norm condition number among the size x size diagonal pieces of L"""
    L, _ = split_factor(F, ldlt)
    n = L.shape[0]
    return max(float(np.linalg.cond(L[a:min(n, a + size), a:min(n, a + size)])) for a in range(0, n, size))


def describe_factor_failure(K, F, ldlt, R, S, bound, visits=None):
    """the worst entry, and the FIRST entry over the bound in elimination order (column by column: what lies behind it inherits its error) with its 128-tile and
    the panel / 16-column stage whose contribution equals the difference when missing or doubled; visits: {(tile row, tile column): [(first panel, end panel)]} of
    the kind-7 tasks of a persistent shape"""
    n = F.shape[0]
    L, d = split_factor(F, ldlt)
    over = np.tril(np.abs(R) > bound) | np.tril(~np.isfinite(R))
    ratio = np.where(np.tril(np.ones_like(over)), np.abs(R) / np.maximum(bound, 1e-300), 0.0)
    wi, wj = np.unravel_index(int(np.nanargmax(ratio)), ratio.shape)
    cols = np.nonzero(over.any(axis=0))[0]
    j = int(cols[0])
    i = int(np.nonzero(over[:, j])[0][0])
    msg = f"{int(over.sum())} entries of the lower triangle over the bound; worst ({wi}, {wj}) of tile ({wi // NB}, {wj // NB}): |R| = {abs(R[wi, wj]):.3e} = " \
          f"{ratio[wi, wj]:.3g} x bound; first in elimination order ({i}, {j}) of tile ({i // NB}, {j // NB}): R = {R[i, j]:.3e}, bound {bound[i, j]:.3e}, S {S[i, j]:.3e}"
    terms = L[i, :j + 1] * L[j, :j + 1] * (1.0 if d is None else d[:j + 1])
    for width, name in ((NB, "panel"), (PIECE, "16-column stage")):
        for s in range(-(-(j + 1) // width)):
            v = terms[s * width:(s + 1) * width].sum()
            for what, w in (("missing", -v), ("doubled", v)):
                if abs(v) > 8.0 * bound[i, j] and abs(R[i, j] - w) <= 4.0 * bound[i, j] + 1e-3 * abs(v):
                    msg += f"; = {name} {s} {what}"
                    if width == NB and visits is not None:
                        inside = [v7 for v7 in visits.get((i // NB, j // NB), []) if v7[0] <= s < v7[1]]
                        msg += f" (inside the kind-7 visit of panels {inside[0][0]}..{inside[0][1] - 1} of that tile)" if inside else " (in no kind-7 visit of that tile)"
    return msg


# ---------------------------------------------------------------------------------------------------------------------------------- sweeps
def sweep_bound(n, inverse):
    """c of |r_i| <= c s_i"""
    c = 2.0 * gamma(n + 2) + 2.0 * gamma(n + 1)
    return c + (2.0 * (gamma(NB + 1) + gamma(PIECE + 1) * K16) * K128 if inverse else 4.0 * gamma(PIECE + 1) * K16)


def sweep_reference_part(n):
    """substitution in fp64 (2 gamma_n) and r formed in fp64 (2 gamma_(n + 1))"""
    return 2.0 * gamma(n) + 2.0 * gamma(n + 1)


class SweepCheck:
    """r = L D L^T x - b and s = |L| |D| |L^T| |x| + |b| against one factor (O(n^2) per solve), with the growth of the diagonal pieces the sweeps invert explicitly:
    128-row blocks in the inverse form, 16 x 16 pieces in the substitution form"""

    def __init__(self, F, ldlt, inverse):
        self.n = n = F.shape[0]
        self.L, self.d = split_factor(F, ldlt)
        self.aL = np.abs(self.L)
        self.inverse = inverse
        size = NB if inverse else PIECE
        self.pieces = [(a, min(n, a + size), piece_growth_matrix(self.L[a:min(n, a + size), a:min(n, a + size)])) for a in range(0, n, size)]
        self.bound = sweep_bound(n, inverse)
        self.limit = K128 if inverse else K16

    def statistic(self, x, b, product=None):
        """(r, s, rho); product(L, w): the forward product L w (the hook of the mutation test)"""
        L, d, aL = self.L, self.d, self.aL
        w = L.T @ x
        aw = aL.T @ np.abs(x)
        if d is not None:
            w, aw = d * w, np.abs(d) * aw
        r = (L @ w if product is None else product(L, w)) - b
        s = aL @ aw + np.abs(b)
        ef, eb = np.empty(self.n), np.empty(self.n)
        for a, e, G in self.pieces:
            ef[a:e] = G @ np.abs(w[a:e])
            eb[a:e] = G.T @ np.abs(x[a:e])
        if d is not None:
            eb = np.abs(d) * eb
        rho = float(((ef + aL @ eb) / (2.0 * s)).max())
        return r, s, rho

    def describe(self, r, s, x):
        i = int(np.argmax(np.abs(r) / s))
        w = self.L.T @ x
        if self.d is not None:
            w = self.d * w
        msg = f"row {i} of block row {i // NB}: r = {r[i]:.3e}, s = {s[i]:.3e}, |r| / s = {abs(r[i]) / s[i]:.3e}, bound {self.bound:.3e}; " \
              f"{int((np.abs(r) > self.bound * s).sum())} rows over the bound"
        for jb in range(i // NB + 1):
            v = float(self.L[i, jb * NB:(jb + 1) * NB] @ w[jb * NB:(jb + 1) * NB])
            for what, q in (("missing", -v), ("doubled", v)):
                if abs(v) > 8.0 * self.bound * s[i] and abs(r[i] - q) <= 4.0 * self.bound * s[i] + 1e-3 * abs(v):
                    msg += f"; = the product with column block {jb} {what}"
        return msg

    def check(self, x, b, label="", product=None):
        """(ratio as a multiple of the bound, rho, None or the failure message)"""
        r, s, rho = self.statistic(x, b, product)
        ratio = float((np.abs(r) / s).max()) / self.bound
        print(f"  {label}: max |r| / s = {ratio * self.bound:.3e} = {ratio:.3f} x bound {self.bound:.3e}; growth {rho:.3f} (assumed <= {self.limit})")
        if not (np.isfinite(x).all() and np.isfinite(r).all()):
            return ratio, rho, "not finite"
        if rho > self.limit:
            return ratio, rho, f"the input is worse conditioned than the derivation assumes: growth {rho:.3f} > {self.limit}"
        if not (np.abs(r) <= self.bound * s).all():
            return ratio, rho, self.describe(r, s, x)
        return ratio, rho, None


def kkt_matrix(Pf, x_reg):
    """Pf + diag(x_reg): one addition per diagonal entry"""
    K = Pf.copy()
    K[np.diag_indices(K.shape[0])] += x_reg
    return K


def run_sweeps(hip, shape, kkt_solver, label):
    """one handle (p = m = 0), one factorisation, five solves in a row (the fifth repeats the first), every solve checked against the factor downloaded once.
    Returns a dict that survives json: factor_ok, kkt_bitwise, repeat_bitwise, ratios (multiples of the bound), growth, failures (messages)"""
    n, ldlt = shape.n, kkt_solver == 16
    Pf, x_reg = sweep_input(n)
    k = hip.DenseKKT(data_of(hip, Pf), kkt_solver=kkt_solver)
    out = dict(factor_ok=bool(k.update_scalings_and_factor(1.0, x_reg, np.zeros(0))), ratios=[], growth=[], failures=[])
    out["kkt_bitwise"] = bool(np.array_equal(np.tril(k.internal_kkt_mat()), np.tril(kkt_matrix(Pf, x_reg))))
    del Pf
    chk = SweepCheck(k.internal_factor(), ldlt, shape.inverse)
    rhs = right_hand_sides(n)
    xs = []
    for q, b in enumerate(rhs + rhs[:1]):
        x, _, _ = k.solve(b, np.zeros(0), np.zeros(0))
        xs.append(x)
        ratio, rho, msg = chk.check(x, b, f"{label} solve {q}")
        out["ratios"].append(ratio)
        out["growth"].append(rho)
        if msg:
            out["failures"].append(f"solve {q}: {msg}")
    out["repeat_bitwise"] = bool(np.array_equal(xs[0], xs[-1]))
    return out
