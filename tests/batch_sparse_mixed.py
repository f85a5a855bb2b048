"""Batches of small sparse QPs of one pattern in which every instance has a set of finite bounds of its own, for the tests of the batched sparse solver with
per-instance bound sets (piqp_amd.BatchSparseSolver(bounds="per_instance"), pq_batch_set_bound_sets).

mixed_sparse_batch(dim, B, salt=0) starts from _random_sparse_qp_batch(dim, B, seed=dim) of tests/test_batch_ldlt_gpu.py.  The generator's own infinities are made
finite first -- h_l = h_u - 1.5 and x_u = x_l + 3.0, only where it had put infinities (finite_sparse_batch) --, so every bound that is then switched off leaves a
feasible problem.  The kinds of instance i come from default_rng((dim * 7919 + i) * 31 + salt): row = integers(0, 4, m) first, then var = integers(0, 4, n); kind 0
keeps both bounds, 1 the lower only, 2 the upper only, 3 neither (a row of G with neither is one SparseSolver drops).  Five instances are forced, f = (i + salt) % B:
    f = 0   (0, 0)  every row and every variable two-sided
    f = 1   (1, 3)  rows lower only, no box at all
    f = 2   (2, 0)  rows upper only, every variable boxed on both sides
    f = 3   (3, 1)  every row of G dropped, lower boxes only
    f = 4   (3, 3)  no finite bound at all
salt changes the patterns only: the bounds of salt = 1 are an update of the instance of salt = 0."""
import numpy as np
import scipy.sparse as sp

from test_batch_ldlt_gpu import _random_sparse_qp_batch

FORCED = {0: (0, 0), 1: (1, 3), 2: (2, 0), 3: (3, 1), 4: (3, 3)}  # f -> (kind of every row, kind of every variable)
LISTS = ("h_l", "h_u", "x_l", "x_u")

_finite = {}


def finite_sparse_batch(dim, B):
    """the generator's batch with every bound finite (computed once per key; nobody changes it)"""
    if (dim, B) not in _finite:
        bt = dict(_random_sparse_qp_batch(dim, B, seed=dim))
        bt["h_l"] = np.where(np.isfinite(bt["h_l"]), bt["h_l"], bt["h_u"] - 1.5)
        bt["x_u"] = np.where(np.isfinite(bt["x_u"]), bt["x_u"], bt["x_l"] + 3.0)
        _finite[(dim, B)] = bt
    return _finite[(dim, B)]


def kinds(dim, B, i, salt=0):
    """(row kinds [m], variable kinds [n]) of instance i"""
    n, m = dim, dim // 2
    rng = np.random.default_rng((dim * 7919 + i) * 31 + salt)
    row = rng.integers(0, 4, m)
    var = rng.integers(0, 4, n)
    f = (i + salt) % B
    if f in FORCED:
        row[:], var[:] = FORCED[f]
    return row, var


def with_kinds(bt, row, var):
    """bt with the bounds switched off as the kinds [B, m] / [B, n] say"""
    out = dict(bt)
    out["h_l"] = np.where(row <= 1, bt["h_l"], -np.inf)
    out["h_u"] = np.where((row == 0) | (row == 2), bt["h_u"], np.inf)
    out["x_l"] = np.where(var <= 1, bt["x_l"], -np.inf)
    out["x_u"] = np.where((var == 0) | (var == 2), bt["x_u"], np.inf)
    return out


def mixed_sparse_batch(dim, B, salt=0):
    """a dict with the keys of _random_sparse_qp_batch"""
    ks = [kinds(dim, B, i, salt) for i in range(B)]
    return with_kinds(finite_sparse_batch(dim, B), np.array([k[0] for k in ks]), np.array([k[1] for k in ks]))


def forced_lists(n, m, f):
    """the (h_l_idx, h_u_idx, x_l_idx, x_u_idx) SparseSolver holds for the forced instance f (a dropped row is in both row lists, with the bounds -1 / 1)"""
    rows, cols, none = list(range(m)), list(range(n)), []
    return {0: (rows, rows, cols, cols), 1: (rows, none, none, none), 2: (none, rows, cols, cols), 3: (rows, rows, cols, none), 4: (rows, rows, none, none)}[f]


def sub_batch(bt, idx):
    """the instances idx of a batch, as a batch"""
    idx = np.asarray(idx)
    out = {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in bt.items()}
    out["B"] = len(idx)
    return out


def instance_args(bt, i):
    """dict(P=..., c=..., ...) of instance i, for orc.Solver.setup / orc.Data.sparse"""
    mat = lambda M, v: sp.csc_matrix((v[i], M.indices, M.indptr), shape=M.shape)
    return dict(P=mat(bt["P"], bt["Pv"]), c=bt["c"][i], A=mat(bt["A"], bt["Av"]), b=bt["b"][i], G=mat(bt["G"], bt["Gv"]), h_l=bt["h_l"][i], h_u=bt["h_u"][i], x_l=bt["x_l"][i],
                x_u=bt["x_u"][i])


def stored_flags(lists, n, m):
    """the finiteness flags pq_debug_bound_lists takes for an update, from the four lists held before it: 1 = in the list"""
    f = {k: np.zeros(m if k[0] == "h" else n, dtype=np.int32) for k in LISTS}
    for k in LISTS:
        f[k][np.asarray(lists[k], dtype=np.int64)] = 1
    return f


def debug_bound_lists(L, m, n, vec, fin=None):
    """pq_debug_bound_lists (the host statement of the rules): vec and fin are dicts over LISTS (a missing vector is NULL; fin None is a setup).  Returns
    ({name: list}, dead [m])"""
    ptr = lambda a: None if a is None else a.ctypes.data
    v = {k: (None if vec.get(k) is None else np.ascontiguousarray(vec[k], dtype=np.float64)) for k in LISTS}
    f = {k: (None if fin is None else np.ascontiguousarray(fin[k], dtype=np.int32)) for k in LISTS}
    counts = np.zeros(4, dtype=np.int32)
    idx = {k: np.full(max(m if k[0] == "h" else n, 1), -7, dtype=np.int32) for k in LISTS}
    dead = np.full(max(m, 1), -7, dtype=np.int32)
    rc = L.pq_debug_bound_lists(m, n, *[ptr(v[k]) for k in LISTS], *[ptr(f[k]) for k in LISTS], ptr(counts), *[ptr(idx[k]) for k in LISTS], ptr(dead), None, None, None, None)
    assert rc == 0, L.pq_last_error_string().decode()
    return {k: idx[k][:c].tolist() for k, c in zip(LISTS, counts)}, dead[:m] != 0
