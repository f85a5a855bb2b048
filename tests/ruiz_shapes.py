"""Shapes and the CPU reference for the device Ruiz equilibration (piqp_amd/csrc/ruiz_kernels.hip), shared by tests/test_ruiz_shapes.py (CPU: the reference IS the
oracle's ruiz_scale_data / ruiz_unscale_data bit for bit, the shapes reach what they claim) and tests/test_ruiz_kernels_gpu.py (the kernels are the reference bit for
bit, through pq_debug_ruiz).

ruiz_reference restates oracle/orc_solver.c:102-256 in NumPy, one IEEE operation per oracle operation and in the oracle's order: dense and sparse data, the three modes
(compute, reuse, unscale) and the tail (b, h_l, h_u and the compressed x_l / x_u).  Norms are maxima (exact in any order); the one sum, the mean column norm of the
cost scaling, is accumulated left to right (np.cumsum).  The strictly lower triangle of a dense P_utri is never read and never written.  ruiz_naive is a second,
deliberately plain scalar-loop restatement of the same routine for small problems.

Values mix magnitudes so that another order of the products shows in the bits: mantissas uniform in [1, 2), exponents uniform in -20 .. 20 (mixed()).  Every shape is a
named, seeded record; its doc says which branch it is there for, and tests/test_ruiz_shapes.py asserts that it gets there."""
import functools
import math

import numpy as np

SENTINEL_BITS = 0x7FF8DEADBEEF5AFE  # PQ_RUIZ_SENTINEL_BITS: a quiet NaN of fixed payload
SENTINEL = float(np.array([SENTINEL_BITS], dtype=np.uint64).view(np.float64)[0])
GUARD = 8                           # PQ_RUIZ_GUARD
MODES = ("compute", "reuse", "unscale")
TR, TC = 256, 32                    # the dense tile of ruiz_kernels.hip
ROWS_PER_WG, MAX_WG, GRID_MAX_ITER = 512, 48, 64  # launch_ruiz_sparse
MATS = ("P", "AT", "GT")


def bits(a):
    """the bit patterns, matrices in column-major order"""
    return np.asarray(a, dtype=np.float64).flatten(order="F").view(np.uint64)


def limit_scaling(d):
    return np.where(d < 1e-4, 1.0, np.where(d > 1e4, 1e4, d))


def arm(d):
    return "low" if d < 1e-4 else ("high" if d > 1e4 else "mid")


def mixed(rng, size, lo=-20, hi=20):
    return rng.choice([-1.0, 1.0], size) * rng.uniform(1.0, 2.0, size) * np.exp2(rng.integers(lo, hi + 1, size).astype(np.float64))


class Problem:
    """one instance.  dense: P (n x n, upper triangle; column-major), AT (n x p), GT (n x m).  sparse: P, AT, GT are (colptr, rowind, values) of the upper triangle of
    P, of A' and of G'.  c, xbs (x_b_scaling).  Tail: b (p), h_l, h_u (m), x_l / x_u compressed to the listed variables x_l_idx / x_u_idx; tail=False: no tail."""

    def __init__(self, sparse, n, p, m, P, AT, GT, c, xbs, b=None, h_l=None, h_u=None, x_l=None, x_l_idx=None, x_u=None, x_u_idx=None):
        self.sparse, self.n, self.p, self.m = sparse, n, p, m
        self.P, self.AT, self.GT = P, AT, GT
        self.c, self.xbs = np.array(c, dtype=np.float64), np.array(xbs, dtype=np.float64)
        f = lambda a, k: np.zeros(k) if a is None else np.array(a, dtype=np.float64)
        g = lambda a: np.zeros(0, np.int32) if a is None else np.array(a, dtype=np.int32)
        self.x_l_idx, self.x_u_idx = g(x_l_idx), g(x_u_idx)
        self.b, self.h_l, self.h_u = f(b, p), f(h_l, m), f(h_u, m)
        self.x_l, self.x_u = f(x_l, self.x_l_idx.size), f(x_u, self.x_u_idx.size)

    def values(self, nm):
        M = getattr(self, nm)
        return M[2] if self.sparse else M

    def copy(self, **kw):
        q = object.__new__(Problem)
        q.__dict__.update(self.__dict__)
        for k in ("c", "xbs", "b", "h_l", "h_u", "x_l", "x_u"):
            setattr(q, k, getattr(self, k).copy())
        for nm in MATS:
            M = getattr(self, nm)
            setattr(q, nm, (M[0], M[1], M[2].copy()) if self.sparse else M.copy(order="F"))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def with_matrices(self, other):
        """the same vectors and tail around the matrix values of `other` (an update of P, A and G)"""
        q = self.copy()
        for nm in MATS:
            M = getattr(other, nm)
            setattr(q, nm, (M[0], M[1], M[2].copy()) if self.sparse else M.copy(order="F"))
        return q

    def with_sentinel_triangle(self):
        q = self.copy()
        if not self.sparse:
            q.P[np.tril_indices(self.n, -1)] = SENTINEL
        return q


class Scalings:
    def __init__(self, delta, delta_inv, delta_b, delta_b_inv, c):
        self.delta, self.delta_inv, self.delta_b, self.delta_b_inv, self.c = delta, delta_inv, delta_b, delta_b_inv, float(c)


def unit_scalings(n, p, m):
    return Scalings(np.ones(n + p + m), np.ones(n + p + m), np.ones(n), np.ones(n), 1.0)


# ------------------------------------------------------------------------------------------------------------------- the reference
def _cols_of(M, cols):
    return np.repeat(np.arange(cols), np.diff(M[0]))


def _sym_norms(q):
    """inf-norms of the rows of the symmetric matrix that the stored upper triangle stands for"""
    n = q.n
    if not q.sparse:
        iu = np.triu(np.ones((n, n), dtype=bool))
        return np.abs(np.where(iu, q.P, q.P.T)).max(axis=1)
    cp, ri, v = q.P
    out = np.zeros(n)
    a = np.abs(v)
    np.maximum.at(out, _cols_of(q.P, n), a)
    np.maximum.at(out, ri, a)  # (for r == j the second maximum changes nothing)
    return out


def _rows_cols(q, nm, cols):
    """inf-norms of the rows (n) and the columns of A' or G'"""
    M = getattr(q, nm)
    if cols == 0:
        return np.zeros(q.n), np.zeros(0)
    if not q.sparse:
        a = np.abs(M)
        return a.max(axis=1), a.max(axis=0)
    rn, cn = np.zeros(q.n), np.zeros(cols)
    a = np.abs(M[2])
    np.maximum.at(rn, M[1], a)
    np.maximum.at(cn, _cols_of(M, cols), a)
    return rn, cn


def _scale(q, s, pre=None):
    """scale_P_scalar (with pre), scale_P and the two scale_T with the scaling s (n + p + m): sparse rows then columns, dense P columns then rows"""
    n, p, m = q.n, q.p, q.m
    if q.sparse:
        cp, ri, v = q.P
        if pre is not None:
            v = v * pre
        q.P = (cp, ri, (v * s[ri]) * s[_cols_of(q.P, n)])
        for nm, cols, o in (("AT", p, n), ("GT", m, n + p)):
            M = getattr(q, nm)
            if cols:
                setattr(q, nm, (M[0], M[1], (M[2] * s[M[1]]) * s[o + _cols_of(M, cols)]))
        return
    iu = np.triu(np.ones((n, n), dtype=bool))
    P = q.P if pre is None else np.where(iu, q.P * pre, q.P)
    q.P = np.asfortranarray(np.where(iu, (P * s[None, :n]) * s[:n, None], P))
    if p:
        q.AT = np.asfortranarray((s[:n, None] * q.AT) * s[None, n:n + p])
    if m:
        q.GT = np.asfortranarray((s[:n, None] * q.GT) * s[None, n + p:])


def _scale_P_scalar(q, g):
    if q.sparse:
        q.P = (q.P[0], q.P[1], q.P[2] * g)
    else:
        iu = np.triu(np.ones((q.n, q.n), dtype=bool))
        q.P = np.asfortranarray(np.where(iu, q.P * g, q.P))


def ruiz_reference(prob, mode="compute", scale_cost=False, max_iter=10, scal=None, eps=1e-3, reverse_sum=False):
    """-> (scaled Problem, Scalings, passes, stats) from copies of `prob`; `scal` is read by reuse and unscale.  stats: the arms of limit_scaling taken by the vector
    scalings ('vec') and by the two clamps of the cost scaling ('gamma1', 'gamma2'), and how often x_b_scaling won ('xb_wins') or lost ('xb_loses') the maximum.
    reverse_sum: the mean column norm summed right to left -- NOT the oracle's order; tests/test_ruiz_shapes.py uses it to show that the order is visible."""
    assert mode in MODES
    q = prob.copy()
    n, p, m = q.n, q.p, q.m
    N = n + p + m
    stats = dict(vec=set(), gamma1=set(), gamma2=set(), xb_wins=0, xb_loses=0)
    passes = 0
    if mode == "compute":
        delta, delta_b, rc = np.ones(N), np.ones(n), 1.0
        di, dib = np.zeros(N), np.zeros(n)
        for _ in range(max_iter):
            dev = max(float(np.max(np.abs(1.0 - di))), float(np.max(np.abs(1.0 - dib))))
            if not dev > eps:
                break
            passes += 1
            v = _sym_norms(q)
            ra, ca = _rows_cols(q, "AT", p)
            rg, cg = _rows_cols(q, "GT", m)
            v = np.maximum(np.maximum(v, ra), rg)
            stats["xb_wins"] += int((q.xbs > v).sum()); stats["xb_loses"] += int((q.xbs < v).sum())
            di = np.concatenate([np.maximum(v, q.xbs), ca, cg])
            dib = q.xbs.copy()
            stats["vec"] |= {arm(x) for x in di} | {arm(x) for x in dib}
            di = 1.0 / np.sqrt(limit_scaling(di))
            dib = 1.0 / np.sqrt(limit_scaling(dib))
            _scale(q, di)
            q.c = q.c * di[:n]
            q.xbs = q.xbs * (dib * di[:n])
            delta = delta * di
            delta_b = delta_b * dib
            if scale_cost:
                cm = _sym_norms(q)
                gamma = float(np.cumsum(cm[::-1] if reverse_sum else cm)[-1]) / float(n)  # left to right
                stats["gamma1"].add(arm(gamma))
                gamma = float(limit_scaling(gamma))
                gamma = max(gamma, float(np.max(np.abs(q.c))))
                stats["gamma2"].add(arm(gamma))
                gamma = 1.0 / float(limit_scaling(gamma))
                _scale_P_scalar(q, gamma)
                q.c = q.c * gamma
                rc = rc * gamma
        out = Scalings(delta, 1.0 / delta, delta_b, 1.0 / delta_b, rc)
        s, sb = out.delta, out.delta_b
    else:
        out = Scalings(scal.delta.copy(), scal.delta_inv.copy(), scal.delta_b.copy(), scal.delta_b_inv.copy(), scal.c)
        s, sb, cs = (out.delta, out.delta_b, out.c) if mode == "reuse" else (out.delta_inv, out.delta_b_inv, 1.0 / out.c)
        _scale(q, s, pre=cs)
        q.c = q.c * (cs * s[:n])
        q.xbs = q.xbs * (sb * s[:n])
    q.b = q.b * s[n:n + p]
    q.h_l = q.h_l * s[n + p:]
    q.h_u = q.h_u * s[n + p:]
    q.x_l = q.x_l * sb[q.x_l_idx]
    q.x_u = q.x_u * sb[q.x_u_idx]
    return q, out, passes, stats


def ruiz_numpy(P_utri, AT, GT, c, x_b_scaling, max_iter, scale_cost, epsilon=1e-3):
    """the dense first run in the form the batched-solver tests use: -> scaled (P_utri, AT, GT, c, x_b_scaling) and (delta, delta_b, c_scale)"""
    P, AT, GT = (np.array(a, dtype=np.float64, order="F") for a in (P_utri, AT, GT))
    q, s, _, _ = ruiz_reference(Problem(False, P.shape[0], AT.shape[1], GT.shape[1], P, AT, GT, c, x_b_scaling), "compute", scale_cost, max_iter, eps=epsilon)
    return (q.P, q.AT, q.GT, q.c, q.xbs), (s.delta, s.delta_b, np.array([s.c]))


# ------------------------------------------------------------------------------------------------------------------- the plain restatement
def ruiz_naive(prob, mode="compute", scale_cost=False, max_iter=10, scal=None, eps=1e-3):
    """orc_solver.c:102-256 statement by statement on Python floats (small problems only).  Same return values as ruiz_reference, without the stats.  The strictly lower
    triangle of a dense P is left alone (the oracle multiplies its zeros by the cost scaling)."""
    q = prob.copy()
    n, p, m = q.n, q.p, q.m
    N = n + p + m
    lim = lambda d: 1.0 if d < 1e-4 else (1e4 if d > 1e4 else d)
    if q.sparse:
        ent = {nm: [(int(r), j, k) for j in range(len(getattr(q, nm)[0]) - 1) for k, r in
                    zip(range(getattr(q, nm)[0][j], getattr(q, nm)[0][j + 1]), getattr(q, nm)[1][getattr(q, nm)[0][j]:getattr(q, nm)[0][j + 1]])] for nm in MATS}
        val = {nm: [float(x) for x in getattr(q, nm)[2]] for nm in MATS}
    else:
        ent = dict(P=[(i, j, i + j * n) for j in range(n) for i in range(j + 1)], AT=[(i, j, i + j * n) for j in range(p) for i in range(n)],
                   GT=[(i, j, i + j * n) for j in range(m) for i in range(n)])
        val = {nm: [float(x) for x in getattr(q, nm).flatten(order="F")] for nm in MATS}
    c, xbs = [float(x) for x in q.c], [float(x) for x in q.xbs]

    def sym_norms():
        out = [0.0] * n
        for i, j, k in ent["P"]:
            a = abs(val["P"][k])
            out[j] = max(out[j], a)
            if i != j:
                out[i] = max(out[i], a)
        return out

    def scale_all(s, pre):
        P = val["P"]
        if pre is not None:
            for _, _, k in ent["P"]:
                P[k] *= pre
        if q.sparse:
            for i, j, k in ent["P"]:
                P[k] *= s[i]
            for i, j, k in ent["P"]:
                P[k] *= s[j]
        else:
            for i, j, k in ent["P"]:
                P[k] *= s[j]
            for i, j, k in ent["P"]:
                P[k] *= s[i]
        for nm, o in (("AT", n), ("GT", n + p)):
            V = val[nm]
            for i, j, k in ent[nm]:
                V[k] = (s[i] * V[k]) * s[o + j]

    passes = 0
    if mode == "compute":
        delta, delta_b, rc = [1.0] * N, [1.0] * n, 1.0
        di, dib = [0.0] * N, [0.0] * n
        for _ in range(max_iter):
            dev = 0.0
            for x in di + dib:
                dev = max(dev, abs(1.0 - x))
            if not dev > eps:
                break
            passes += 1
            di = sym_norms() + [0.0] * (p + m)
            for nm, o in (("AT", n), ("GT", n + p)):
                for i, j, k in ent[nm]:
                    a = abs(val[nm][k])
                    di[i] = max(di[i], a)
                    di[o + j] = max(di[o + j], a)
            for i in range(n):
                di[i] = max(di[i], xbs[i])
                dib[i] = xbs[i]
            di = [1.0 / math.sqrt(lim(x)) for x in di]
            dib = [1.0 / math.sqrt(lim(x)) for x in dib]
            scale_all(di, None)
            for i in range(n):
                c[i] *= di[i]
                xbs[i] *= dib[i] * di[i]
                delta_b[i] *= dib[i]
            for i in range(N):
                delta[i] *= di[i]
            if scale_cost:
                gamma = 0.0
                for x in sym_norms():
                    gamma += x
                gamma /= float(n)
                gamma = lim(gamma)
                cinf = 0.0
                for x in c:
                    cinf = max(cinf, abs(x))
                gamma = 1.0 / lim(max(gamma, cinf))
                for _, _, k in ent["P"]:
                    val["P"][k] *= gamma
                for i in range(n):
                    c[i] *= gamma
                rc *= gamma
        out = Scalings(np.array(delta), np.array([1.0 / x for x in delta]), np.array(delta_b), np.array([1.0 / x for x in delta_b]), rc)
        s, sb = delta, delta_b
    else:
        out = Scalings(scal.delta.copy(), scal.delta_inv.copy(), scal.delta_b.copy(), scal.delta_b_inv.copy(), scal.c)
        s, sb, cs = (out.delta, out.delta_b, out.c) if mode == "reuse" else (out.delta_inv, out.delta_b_inv, 1.0 / out.c)
        s, sb = [float(x) for x in s], [float(x) for x in sb]
        scale_all(s, cs)
        for i in range(n):
            c[i] *= cs * s[i]
            xbs[i] *= sb[i] * s[i]
    for nm in MATS:
        if q.sparse:
            M = getattr(q, nm)
            setattr(q, nm, (M[0], M[1], np.array(val[nm], dtype=np.float64)))
        else:
            M = getattr(q, nm).flatten(order="F")
            for _, _, k in ent[nm]:
                M[k] = val[nm][k]
            setattr(q, nm, M.reshape(getattr(q, nm).shape, order="F"))
    q.c, q.xbs = np.array(c), np.array(xbs)
    q.b = np.array([float(q.b[i]) * s[n + i] for i in range(p)])
    q.h_l = np.array([float(q.h_l[i]) * s[n + p + i] for i in range(m)])
    q.h_u = np.array([float(q.h_u[i]) * s[n + p + i] for i in range(m)])
    q.x_l = np.array([float(q.x_l[k]) * sb[int(q.x_l_idx[k])] for k in range(q.x_l_idx.size)])
    q.x_u = np.array([float(q.x_u[k]) * sb[int(q.x_u_idx[k])] for k in range(q.x_u_idx.size)])
    return q, out, passes


FIELDS = ("P", "AT", "GT", "c", "xbs", "b", "h_l", "h_u", "x_l", "x_u")
SCAL_FIELDS = ("delta", "delta_inv", "delta_b", "delta_b_inv")


def differences(got, want, got_s=None, want_s=None):
    """names of the arrays of two (Problem, Scalings) pairs that differ in any bit, with the count and the first place"""
    bad = []
    pairs = [(k, got.values(k) if k in MATS else getattr(got, k), want.values(k) if k in MATS else getattr(want, k)) for k in FIELDS]
    if got_s is not None:
        pairs += [(k, getattr(got_s, k), getattr(want_s, k)) for k in SCAL_FIELDS] + [("c_scale", np.array([got_s.c]), np.array([want_s.c]))]
    for k, g, w in pairs:
        gb, wb = bits(g), bits(w)
        if gb.shape != wb.shape:
            bad.append((k, "shape", gb.shape, wb.shape))
            continue
        d = np.nonzero(gb != wb)[0]
        if d.size:
            i = int(d[0])
            bad.append((k, f"{d.size} of {gb.size} entries differ in bits; first at {i}: {float(gb[i:i + 1].view(np.float64)[0])!r} != {float(wb[i:i + 1].view(np.float64)[0])!r}"))
    return bad


# ------------------------------------------------------------------------------------------------------------------- the launch plan
def sparse_plan(N, max_iter, batch=1, threads=1024, grid_ws=True, cus=256):
    """launch_ruiz_sparse: (kernel, grid x, grid y, threads); at least 48 CUs assumed"""
    g = max(1, min(min(cus if cus > 0 else 64, MAX_WG), (N + ROWS_PER_WG - 1) // ROWS_PER_WG))
    if batch == 1 and grid_ws and max_iter <= GRID_MAX_ITER and g > 1:
        return ("grid", g, 1, 256)
    return ("one_wg", batch, 1, threads)


def dense_plan(n, p, m):
    """DeviceRuiz::run, dense: the launch reported (the tile grid of P) and, per matrix, (row blocks, column blocks, tiles that return at once below the diagonal)"""
    up = lambda a, b: (a + b - 1) // b
    rb = up(n, TR)
    grids = dict(P=(rb, up(n, TC), sum(1 for r in range(rb) for cb in range(up(n, TC)) if r * TR > cb * TC + TC - 1)),
                 AT=(rb, max(1, up(p, TC)), 0), GT=(rb, max(1, up(m, TC)), 0))
    return ("dense", rb, up(n, TC), TR), grids


# ------------------------------------------------------------------------------------------------------------------- problems
def _tail(rng, n, p, m, kind, seed):
    """b, h_l, h_u and compressed box bounds: 'full' every variable bounded both ways, 'uneven' n_x_l != n_x_u with scattered index lists, 'none' no box bounds.  The
    index lists depend on the seed alone (the instances of a batch share them), the values come from rng."""
    irng = np.random.default_rng(seed + 2)
    b, h_l = mixed(rng, p, -6, 6), -np.abs(mixed(rng, m, -6, 6))
    h_u = np.abs(mixed(rng, m, -6, 6))
    if kind == "full":
        li, ui = np.arange(n), np.arange(n)
    elif kind == "uneven":
        li, ui = np.sort(irng.permutation(n)[:max(1, n // 3)]), np.sort(irng.permutation(n)[:max(1, (2 * n) // 3)])
    else:
        li, ui = np.zeros(0, int), np.zeros(0, int)
    return dict(b=b, h_l=h_l, h_u=h_u, x_l=-np.abs(mixed(rng, li.size, -6, 6)), x_l_idx=li, x_u=np.abs(mixed(rng, ui.size, -6, 6)), x_u_idx=ui)


def dense_problem(n, p, m, seed, style="mixed", box="uneven", c_exp=(-10, 10)):
    """style 'mixed': magnitudes over 2^-20 .. 2^20, rows with norm below 1e-4 and above 1e4, column 0 of A' and column m - 1 of G' (a disabled constraint) zero,
    x_b_scaling above the row norm for some variables and below it for others, |c| over 2^c_exp (a small c leaves the cost scaling to the mean column norm of P,
    whose summation order then shows); 'equilibrated': every row and column norm and x_b_scaling exactly 1; 'near': a
    diagonal P within a few per cent of 1 coupled by off-diagonal entries of A' and G', x_b_scaling = 1"""
    rng = np.random.default_rng(seed)
    iu = np.triu(np.ones((n, n), dtype=bool))
    if style == "mixed":
        P = np.where(iu, mixed(rng, (n, n)), 0.0)
        AT, GT = mixed(rng, (n, p)), mixed(rng, (n, m))
        if n >= 4:
            tiny, huge = 1, n - 2
            for M in (P, AT, GT):  # one variable whose whole row (and column of P) stays below 1e-4, one far above 1e4
                M[tiny, :] *= 0.0
            P[:, tiny] *= 0.0
            P[tiny, tiny] = 2.0 ** -15
            P[huge, huge] = 1.5 * 2.0 ** 22
        if p:
            AT[:, 0] = 0.0
        if m:
            GT[:, m - 1] = 0.0
        c = mixed(rng, n, *c_exp)
        xbs = np.abs(mixed(rng, n, -12, 12))
        if n >= 4:
            xbs[1] = 2.0 ** -16
    elif style == "equilibrated":
        P = np.where(iu, rng.uniform(-1.0, 1.0, (n, n)), 0.0)
        P[np.diag_indices(n)] = rng.choice([-1.0, 1.0], n)
        AT, GT = rng.uniform(-1.0, 1.0, (n, p)), rng.uniform(-1.0, 1.0, (n, m))
        for M, k in ((AT, p), (GT, m)):
            for j in range(k):
                M[rng.integers(n), j] = 1.0
        c, xbs = rng.uniform(-1.0, 1.0, n), np.ones(n)
    else:
        assert style == "near"
        P = np.diag(1.0 + rng.uniform(-0.05, 0.05, n))
        AT, GT = np.zeros((n, p)), np.zeros((n, m))
        for M, k in ((AT, p), (GT, m)):
            for j in range(k):
                M[rng.permutation(n)[:min(n, 3)], j] = 1.0 + rng.uniform(-0.03, 0.03, min(n, 3))
        c, xbs = rng.uniform(-3.0, 3.0, n), np.ones(n)
    t = _tail(rng, n, p, m, box, seed)
    if style == "mixed" and m:
        t["h_l"][m - 1], t["h_u"][m - 1] = -1.0, 1.0  # what data.hpp:144-169 leaves of a constraint without bounds
    return Problem(False, n, p, m, np.asfortranarray(P), np.asfortranarray(AT), np.asfortranarray(GT), c, xbs, **t)


def sparse_pattern(n, p, m, seed, no_diag=False, hot_row=True):
    """banded patterns with at most 4 entries per column (the oracle's symbolic analysis of them stays cheap).  P: rows j - 3 .. j; columns = 5 mod 7 are empty, and
    with no_diag no column stores its diagonal.  A', G': rows around j n / cols; with hot_row every third column of A' also holds row n // 2 (atomic maxima of many
    columns on one row)."""
    rng = np.random.default_rng(seed)

    def build(cols, rows_of):
        cp, ri = [0], []
        for j in range(cols):
            r = sorted(set(int(x) for x in rows_of(j)))
            ri += r
            cp.append(len(ri))
        return np.array(cp, dtype=np.int32), np.array(ri, dtype=np.int32)

    def p_rows(j):
        if n > 7 and j % 7 == 5:
            return []
        lo = max(0, j - 3)
        r = [x for x in rng.integers(lo, j + 1, 2)] + ([] if no_diag else [j])
        return [x for x in r if not (no_diag and x == j)]

    def t_rows(cols, hot):
        def f(j):
            ctr = (j * n) // max(cols, 1)
            r = [min(n - 1, max(0, ctr + int(d))) for d in rng.integers(-3, 4, 3)]
            if hot and j % 3 == 0:
                r.append(n // 2)
            return r
        return f

    return build(n, p_rows), build(p, t_rows(p, hot_row)), build(m, t_rows(m, False))


def sparse_problem(n, p, m, seed, style="mixed", box="uneven", no_diag=False, c_exp=(-10, 10)):
    """style as in dense_problem; 'mixed' also makes the off-diagonal entries of P dominate their rows (every fourth column: 2^24 above the diagonal)"""
    rng = np.random.default_rng(seed + 1)
    (Pp, Pi), (Ap, Ai), (Gp, Gi) = sparse_pattern(n, p, m, seed, no_diag=no_diag)
    cj = np.repeat(np.arange(n), np.diff(Pp))
    if style == "mixed":
        Pv, Av, Gv = mixed(rng, Pi.size), mixed(rng, Ai.size), mixed(rng, Gi.size)
        off = (Pi != cj) & (cj % 4 == 0)
        Pv[off] = np.sign(Pv[off]) * np.exp2(24.0) * rng.uniform(1.0, 2.0, int(off.sum()))
        c, xbs = mixed(rng, n, *c_exp), np.abs(mixed(rng, n, -12, 12))
    elif style == "equilibrated":
        Pv, Av, Gv = rng.uniform(-1.0, 1.0, Pi.size), rng.uniform(-1.0, 1.0, Ai.size), rng.uniform(-1.0, 1.0, Gi.size)
        Pv[Pi == cj] = 1.0
        for cp, v in ((Ap, Av), (Gp, Gv)):
            v[cp[:-1][np.diff(cp) > 0]] = -1.0  # the first entry of every column
        c, xbs = rng.uniform(-1.0, 1.0, n), np.ones(n)
    else:
        assert style == "near"
        Pv = np.where(Pi == cj, 1.0 + rng.uniform(-0.05, 0.05, Pi.size), 0.01 * rng.uniform(-1.0, 1.0, Pi.size))
        Av, Gv = 1.0 + rng.uniform(-0.03, 0.03, Ai.size), 1.0 + rng.uniform(-0.03, 0.03, Gi.size)
        c, xbs = rng.uniform(-3.0, 3.0, n), np.ones(n)
    return Problem(True, n, p, m, (Pp, Pi, Pv), (Ap, Ai, Av), (Gp, Gi, Gv), c, xbs, **_tail(rng, n, p, m, box, seed))


def second_values(prob, seed):
    """another set of matrix values in the same patterns (what an update brings): mixed magnitudes over 2^-6 .. 2^6, zeros stay zeros"""
    rng = np.random.default_rng(seed + 77)
    q = prob.copy()
    for nm in MATS:
        v = q.values(nm)
        new = np.where(v != 0.0, mixed(rng, v.shape, -6, 6), 0.0)
        if q.sparse:
            M = getattr(q, nm)
            setattr(q, nm, (M[0], M[1], new))
        else:
            setattr(q, nm, np.asfortranarray(new))
    return q


# ------------------------------------------------------------------------------------------------------------------- shapes
class Shape:
    """name; kind 'dense' / 'sparse' (solver path) / 'batch' (kernel path); doc: the branch it is there for; make() -> the list of instances (one unless 'batch');
    scale_cost, max_iter; passes: the pass counts the instances must take ('0', '1', 'mid' = 2 .. 9, '10', None = not claimed); threads, tail ('full' / 'absent' /
    'uneven') and pad (doubles of stride beyond the layout) for the kernel path; also_kernel: a solver-path shape that is run through the kernel path too"""

    def __init__(self, name, kind, doc, make, scale_cost, max_iter, passes=None, threads=1024, tail="absent", pad=0, also_kernel=False):
        self.name, self.kind, self.doc, self._make = name, kind, doc, make
        self.scale_cost, self.max_iter, self.passes, self.threads, self.tail, self.pad, self.also_kernel = scale_cost, max_iter, passes, threads, tail, pad, also_kernel

    @functools.lru_cache(maxsize=None)
    def instances(self):
        r = self._make()
        return tuple(r) if isinstance(r, (list, tuple)) else (r,)

    @functools.lru_cache(maxsize=None)
    def seconds(self):
        return tuple(second_values(q, 1000 + i) for i, q in enumerate(self.instances()))

    @property
    def N(self):
        q = self.instances()[0]
        return q.n + q.p + q.m


def _gamma_batch(n, p, m, seed):
    """three instances of one pattern: equilibrated (1 pass, the cost scaling's middle arm), P around 2^-30 with |c| <= 1 (the mean column norm falls below 1e-4:
    lower clamp, gamma = 1) and P around 2^40 with |c| around 2^30 (both upper clamps, gamma = 1e-4); their pass counts differ"""
    a = sparse_problem(n, p, m, seed, "equilibrated", box="uneven")
    rng = np.random.default_rng(seed + 5)
    b = sparse_problem(n, p, m, seed, "near", box="uneven")
    b.P = (b.P[0], b.P[1], b.P[2] * 2.0 ** -30)
    b.c = rng.uniform(-1.0, 1.0, n) * 2.0 ** -3
    c = sparse_problem(n, p, m, seed, "mixed", box="uneven")
    c.P = (c.P[0], c.P[1], c.P[2] * 2.0 ** 40)
    c.c = mixed(rng, n, 28, 32)
    return [a, b, c]


@functools.lru_cache(maxsize=None)
def all_shapes():
    S, D, SP = Shape, dense_problem, sparse_problem
    out = [
        # ---- dense, tile 256 x 32
        S("d_n1", "dense", "n = 1: one thread of one tile, no constraints", lambda: D(1, 0, 0, 11), True, 10),
        S("d_n31_p1", "dense", "n = 31, p = 1, m = 0: a partial tile column, one-column A'", lambda: D(31, 1, 0, 12), False, 3),
        S("d_n32_m1", "dense", "n = 32, p = 0, m = 1: exactly one tile column, G' without A'", lambda: D(32, 0, 1, 13), True, 10),
        S("d_n33_p33_m32", "dense", "n = 33: a second, one-column tile column; p = 33 and m = 32: tile-column edges of A' and G'", lambda: D(33, 33, 32, 14), False, 10),
        S("d_n255_p32_m33", "dense", "n = 255: one row short of the row block; max_iter = 3", lambda: D(255, 32, 33, 15), True, 3),
        S("d_n256_iter0", "dense", "n = 256: exactly one row block; max_iter = 0: no pass, unit scalings", lambda: D(256, 1, 1, 16), False, 0, passes="0"),
        S("d_n257_p33", "dense", "n = 257: a second row block of one row, its tiles strictly below the diagonal return at once, column 256 is a one-column tile", lambda: D(257, 33, 0, 17), True, 10),
        S("d_n513_m33", "dense", "n = 513: three row blocks, 17 tile columns", lambda: D(513, 0, 33, 18), True, 10),
        S("d_conv1", "dense", "already equilibrated: exactly 1 pass", lambda: D(40, 5, 7, 19, "equilibrated"), True, 10, passes="1"),
        S("d_conv_mid", "dense", "converges in 2 .. 9 passes: the launches after that must all return on the done flag", lambda: D(300, 33, 32, 20, "near"), True, 10, passes="mid"),
        S("d_conv10", "dense", "mixed magnitudes: runs into the limit of 10 passes", lambda: D(64, 32, 1, 21, c_exp=(-30, -20)), True, 10, passes="10"),
        # ---- sparse, solver path: N = n + p + m decides the launch
        S("s_N1", "sparse", "N = 1: one workgroup", lambda: SP(1, 0, 0, 31), True, 10, also_kernel=True),
        S("s_N511", "sparse", "N = 511: one workgroup", lambda: SP(300, 111, 100, 32), False, 10, also_kernel=True),
        S("s_N512_p0_m0", "sparse", "N = 512, p = m = 0: still one workgroup; a small c: the cost scaling is the mean column norm", lambda: SP(512, 0, 0, 33, c_exp=(-30, -20)), True, 10, also_kernel=True),
        S("s_N513_m0", "sparse", "N = 513, m = 0: the grid kernel on g = 2 workgroups", lambda: SP(256, 257, 0, 34), True, 10, also_kernel=True),
        S("s_N1025", "sparse", "N = 1025: g = 3; P stores no diagonal entry", lambda: SP(500, 200, 325, 35, no_diag=True, c_exp=(-30, -20)), True, 10, passes="10", also_kernel=True),
        S("s_N1025_conv1", "sparse", "g = 3, already equilibrated: exactly 1 pass", lambda: SP(500, 200, 325, 36, "equilibrated"), True, 10, passes="1", also_kernel=True),
        S("s_N1025_conv_mid", "sparse", "g = 3, converges in 2 .. 9 passes: every workgroup must leave the loop at the same pass", lambda: SP(500, 200, 325, 37, "near"), True, 10, passes="mid", also_kernel=True),
        S("s_N600_iter65", "sparse", "max_iter = 65 with N > 512: more passes than the grid workspace has slots, falls back to one workgroup", lambda: SP(300, 150, 150, 38), False, 65),
        S("s_N24064", "sparse", "N = 24 064: g = 47", lambda: SP(12000, 6000, 6064, 39), False, 10),
        S("s_N24065", "sparse", "N = 24 065: g = 48", lambda: SP(12001, 6000, 6064, 40), True, 10),
        S("s_N30000", "sparse", "N = 30 000: g = 48, capped", lambda: SP(15000, 5000, 10000, 41, no_diag=True), True, 3),
        # ---- sparse, kernel path: batch instances of one pattern, strided, with the tail
        S("k_b3_t64", "batch", "batch 3, 64 threads, N = 72 < 512, full tail; pass counts differ, the cost scaling takes its lower, middle and upper arm", lambda: _gamma_batch(40, 12, 20, 51), True, 10,
          threads=64, tail="full", pad=13),
        S("k_b3_t256", "batch", "batch 3, 256 threads, N = 650 > 512, n_x_l != n_x_u with scattered index lists", lambda: _gamma_batch(300, 150, 200, 52), True, 10, threads=256, tail="uneven", pad=5),
        S("k_b3_t1024_notail", "batch", "batch 3, 1024 threads, null tail pointers; a small c in instance 0", lambda: _same_pattern(40, 12, 20, 53), True, 10, threads=1024, tail="absent", pad=1),
        S("k_b1_t1024", "batch", "batch 1, 1024 threads, N = 650 > 512: the kernel behind PIQP_AMD_DEBUG=ruiz_one_wg", lambda: [SP(300, 150, 200, 54, box="full", c_exp=(-30, -20))], True, 10, threads=1024, tail="full", pad=0),
    ]
    assert len({s.name for s in out}) == len(out)
    return tuple(out)


def _same_pattern(n, p, m, seed):
    """three instances of ONE pattern (the seed fixes it) in the three styles"""
    return [sparse_problem(n, p, m, seed, st, box="none", c_exp=(-30, -20)) for st in ("mixed", "near", "equilibrated")]


def shape(name):
    return next(s for s in all_shapes() if s.name == name)


@functools.lru_cache(maxsize=None)
def chain(name, i, sentinel=False):
    """the reference on instance i of a shape, computed once per process, shared by the tests and never written to: compute -> unscale -> the second matrices assigned
    -> reuse, and -> compute again.  sentinel: dense P_utri carries the sentinel below its diagonal throughout."""
    s = shape(name)
    q, q2 = s.instances()[i], s.seconds()[i]
    if sentinel:
        q, q2 = q.with_sentinel_triangle(), q2.with_sentinel_triangle()
    r0, s0, passes, stats = ruiz_reference(q, "compute", s.scale_cost, s.max_iter)
    r1, _, _, _ = ruiz_reference(r0, "unscale", scal=s0)
    assigned = r1.with_matrices(q2)
    r2, s2, _, _ = ruiz_reference(assigned, "reuse", scal=s0)
    r3, s3, passes3, _ = ruiz_reference(assigned, "compute", s.scale_cost, s.max_iter)
    return dict(start=q, compute=(r0, s0), unscale=(r1, s0), assigned=assigned, reuse=(r2, s2), recompute=(r3, s3), passes=passes, stats=stats, passes3=passes3)
