"""Sparse problems whose matrix VALUES are taken from GPU memory (pq_solver_setup_sparse_mem / pq_solver_update_sparse_mem, pq_sparse_data.mem = PQ_MEM_DEVICE;
csrc/ingest_kernels.hip: mapped gather, zeroed rows of G).  The index arrays stay on the host in every mode.

Ingestion is a gather and a zero-fill, the equilibration kernels are the ones the host-fed path runs on the same values, the backends copy device-to-device instead
of host-to-device: no arithmetic differs.  Every comparison below is therefore BITWISE against the host-fed path (np.array_equal, uint64 views for the vectors that
may hold signed zeros; no tolerance anywhere)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from qp_io import load_qp

pytestmark = pytest.mark.gpu

NAMES = ("P", "c", "A", "b", "G", "h_l", "h_u", "x_l", "x_u")
SYNTHETIC = {"syn_no_eq": (37, 0, 21, 3), "syn_no_ineq": (41, 13, 0, 5), "syn_full": (130, 30, 70, 7)}  # n, p, m, seed; syn_full: every value array longer than one workgroup
FIXTURES = ("mm_HS118", "mm_QAFIRO", "mm_DUAL1", "mm_CVXQP1_S", "nl_sc50a", "qp_c0_scenario_mpc", "syn_no_eq", "syn_no_ineq", "syn_full")
FULL = "syn_full"  # has P (given in full), A and G
MPC = "qp_c0_scenario_mpc"
SOLVERS = ("SPARSE_LDLT", "SPARSE_LDLT_MULTIFRONTAL", "SPARSE_LDLT_EQ_COND", "SPARSE_LDLT_INEQ_COND", "SPARSE_LDLT_COND")
_CACHE = {}


def _synthetic(n, p, m, seed):
    """a feasible, strictly convex sparse QP; p = 0 or m = 0 leaves the matrix out (a NULL pointer at the C level).  P is given in full, with some empty columns
    off the diagonal; A and G have empty columns and rows of different lengths."""
    rng = np.random.default_rng(seed)
    R = sp.random(n, n, density=0.08, random_state=rng, format="csc")
    U = sp.triu(R, 1)
    S = U + U.T
    P = sp.csc_matrix(S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0))
    x0 = rng.standard_normal(n)
    q = dict(P=P, c=rng.standard_normal(n), A=None, b=None, G=None, h_l=None, h_u=None)
    if p:
        q["A"] = sp.random(p, n, density=0.2, random_state=rng, format="csc")
        q["b"] = q["A"] @ x0
    if m:
        q["G"] = sp.random(m, n, density=0.25, random_state=rng, format="csc")
        gx, r = q["G"] @ x0, rng.random(m)
        q["h_l"] = np.where(r < 0.4, -np.inf, gx - rng.random(m))
        q["h_u"] = np.where(r > 0.7, np.inf, gx + rng.random(m))
    r = rng.random(n)
    q["x_l"] = np.where(r < 0.3, x0 - rng.random(n), -np.inf)
    q["x_u"] = np.where(r > 0.6, x0 + rng.random(n), np.inf)
    return q


def _case(name):
    if name not in _CACHE:
        if name in SYNTHETIC:
            q = _synthetic(*SYNTHETIC[name])
        else:
            q = load_qp(name)
        for k in ("P", "A", "G"):
            if q[k] is not None:
                q[k] = sp.csc_matrix(q[k])
                q[k].sort_indices()
        _CACHE[name] = q
    return dict(_CACHE[name])  # (shallow: the tests replace entries, never write into them)


def _raise_diagonal(P, rng):
    """P with its stored diagonal entries raised: same pattern, still symmetric and convex"""
    P2 = P.copy()
    cols = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))
    diag = P.indices == cols
    P2.data = P.data + np.where(diag, rng.uniform(0.1, 1.0, P.nnz), 0.0)
    return P2


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _to_gpu(q):
    """matrices as (pattern, CUDA values in the pattern's sorted CSC order), vectors as CUDA tensors"""
    out = {}
    for k, v in q.items():
        if v is None:
            out[k] = None
        elif k in ("P", "A", "G"):
            out[k] = (v, _cuda(v.data))
        else:
            out[k] = _cuda(v)
    return out


def _values_to_gpu(kw):
    """update arguments: a matrix as a bare CUDA tensor of its values, vectors as CUDA tensors"""
    return {k: (None if v is None else _cuda(v.data if k in ("P", "A", "G") else v)) for k, v in kw.items()}


def _new_solver(hip, kkt_solver, reuse=None):
    s = hip.SparseSolver()
    s.settings.kkt_solver = kkt_solver
    if reuse is not None:
        s.settings.preconditioner_reuse_on_update = int(reuse)
    s.enable_trace()
    return s


def _ks(hip, name):
    return getattr(hip.kkt, name)


def _outcome(s, status):
    return dict(status=status, iter=s.info.iter, trace=s.trace(), result=s.result())


def _assert_same_outcome(a, b, what):
    assert a["status"] == b["status"], (what, a["status"], b["status"])
    assert a["iter"] == b["iter"], (what, a["iter"], b["iter"])
    assert _same_bits(a["trace"], b["trace"]), (what, "trace")
    assert set(a["result"]) == set(b["result"]) and len(a["result"]) == 10
    for k in a["result"]:
        assert _same_bits(a["result"][k], b["result"][k]), (what, k)


def _pair(hip, q, kkt_solver, reuse=None):
    h, d = _new_solver(hip, kkt_solver, reuse), _new_solver(hip, kkt_solver, reuse)
    assert h.setup(**q) and d.setup(**_to_gpu(q))
    return h, d


# ---------------------------------------------------------------------------------------------- 1. whole solves
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", FIXTURES)
def test_sparse_solve_from_gpu_memory_is_bitwise_the_host_fed_one(hip, name, solver):
    q = _case(name)
    h, d = _pair(hip, q, _ks(hip, solver))
    nnz = sp.triu(q["P"]).nnz + (0 if q["A"] is None else q["A"].nnz) + (0 if q["G"] is None else q["G"].nnz)
    assert h.last_ingest() == (8 * nnz, 0)
    assert d.last_ingest() == (0, 8 * nnz)
    oh, od = _outcome(h, h.solve()), _outcome(d, d.solve())
    assert oh["iter"] > 0
    _assert_same_outcome(oh, od, (name, solver))


def test_multistage_solve_from_gpu_memory_is_bitwise_the_host_fed_one(hip):
    q = _case(MPC)
    h, d = _pair(hip, q, hip.SPARSE_MULTISTAGE)
    oh, od = _outcome(h, h.solve()), _outcome(d, d.solve())
    assert oh["iter"] > 0
    _assert_same_outcome(oh, od, "sparse_multistage")
    rng = np.random.default_rng(2)
    P2 = _raise_diagonal(q["P"], rng)
    assert h.update(P=P2) and d.update(P=_cuda(P2.data))
    assert d.last_ingest()[0] == 0
    _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), "sparse_multistage, update(P)")


def test_numpy_arguments_beside_gpu_tensors_are_moved_for_the_caller(hip):
    q = _case(FULL)
    h = _new_solver(hip, hip.SPARSE_LDLT)
    assert h.setup(**q)
    mixed = dict(q)
    mixed["G"] = (q["G"], _cuda(q["G"].data))  # one CUDA array: P and A (scipy, their own values) and the numpy vectors follow it to the device
    d = _new_solver(hip, hip.SPARSE_LDLT)
    assert d.setup(**mixed)
    assert d.last_ingest()[0] == 0
    _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), "mixed scipy / CUDA arguments")


# ---------------------------------------------------------------------------------------------- 2. updates
def _perturbed(M, rng, rel):
    M2 = M.copy()
    M2.data = M.data * (1.0 + rel * rng.standard_normal(M.nnz))
    return M2


@pytest.mark.parametrize("reuse", [0, 1])
@pytest.mark.parametrize("solver", ["SPARSE_LDLT", "SPARSE_LDLT_MULTIFRONTAL", "SPARSE_LDLT_COND"])
def test_updates_from_gpu_memory_stay_bitwise_the_host_fed_ones(hip, solver, reuse):
    q = _case(FULL)
    rng = np.random.default_rng(17)
    h, d = _pair(hip, q, _ks(hip, solver), reuse)
    _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), "after setup")

    def step(what, **kw):
        assert h.update(**kw)
        assert d.update(**_values_to_gpu(kw))
        link, dev = d.last_ingest()
        moved = sum((sp.triu(v).nnz if k == "P" else v.nnz) for k, v in kw.items() if k in ("P", "A", "G"))
        assert link == 0 and dev == 8 * moved, (what, link, dev)
        _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), (what, solver, reuse))

    P2 = _raise_diagonal(q["P"], rng)
    A2, G2 = _perturbed(q["A"], rng, 0.01), _perturbed(q["G"], rng, 0.01)
    step("update(P)", P=P2)
    step("update(A)", A=A2)
    step("update(G)", G=G2)
    step("update(P, A, G)", P=q["P"], A=q["A"], G=G2)
    step("vectors only", c=q["c"] * 1.01, b=q["b"] + 1e-3)
    step("update(A, b, c)", A=A2, b=q["b"], c=q["c"])


def test_host_fed_and_device_fed_updates_mix_on_one_solver(hip):
    """Three solvers take the same sequence of calls, in lock-step (as everywhere in this file, the yardstick is a host-fed solver with the same history of updates
    and solves): `h` host-fed throughout, `d` set up from GPU memory and then updated from host arrays, `h2` set up from host arrays and then updated from GPU memory."""
    q = _case(FULL)
    rng = np.random.default_rng(3)
    h, d = _pair(hip, q, hip.SPARSE_LDLT)
    h2 = _new_solver(hip, hip.SPARSE_LDLT)
    assert h2.setup(**q)
    A2, G2 = _perturbed(q["A"], rng, 0.01), _perturbed(q["G"], rng, 0.01)
    # device-fed solver, host-fed update: the values are staged in HBM and counted as link traffic;
    # host-fed solver, device-fed update: from here on its values live on the device
    assert h.update(A=A2) and d.update(A=A2) and h2.update(A=_cuda(A2.data))
    assert d.last_ingest() == (8 * A2.nnz, 8 * A2.nnz)
    assert h2.last_ingest() == (0, 8 * A2.nnz)
    oh = _outcome(h, h.solve())
    _assert_same_outcome(oh, _outcome(d, d.solve()), "host-fed update of a device-fed solver")
    _assert_same_outcome(oh, _outcome(h2, h2.solve()), "device-fed update of a host-fed solver")
    assert h.update(G=G2) and h2.update(G=G2) and d.update(G=_cuda(G2.data))
    oh = _outcome(h, h.solve())
    _assert_same_outcome(oh, _outcome(h2, h2.solve()), "then a host-fed update again")
    _assert_same_outcome(oh, _outcome(d, d.solve()), "then a device-fed update again")


# ---------------------------------------------------------------------------------------------- 3. the unread triangle of P
@pytest.mark.parametrize("solver", ["SPARSE_LDLT", "SPARSE_LDLT_MULTIFRONTAL"])
def test_unread_triangle_of_P_never_reaches_the_solver(hip, solver):
    q = _case(FULL)
    full = sp.csc_matrix(sp.triu(q["P"]) + sp.triu(q["P"], 1).T)
    full.sort_indices()
    rows = np.repeat(np.arange(full.shape[1]), np.diff(full.indptr))
    lower = full.indices > rows
    assert lower.any()
    dirty = full.data.copy()
    dirty[lower] = np.nan
    clean = dict(q); clean["P"] = sp.triu(full, format="csc")  # the host-fed twin gets the upper triangle only
    h = _new_solver(hip, _ks(hip, solver))
    assert h.setup(**clean)
    g = _to_gpu(q)
    g["P"] = (full, _cuda(dirty))  # the NaN entries sit in the device tensor
    d = _new_solver(hip, _ks(hip, solver))
    assert d.setup(**g)
    oh, od = _outcome(h, h.solve()), _outcome(d, d.solve())
    _assert_same_outcome(oh, od, "NaN below the diagonal of P")
    assert all(np.isfinite(v).all() for v in od["result"].values()) and np.isfinite(od["trace"]).all()
    # ... and through update(P)
    dirty2 = dirty * 1.01
    clean2 = clean["P"].copy(); clean2.data = clean2.data * 1.01
    assert h.update(P=clean2) and d.update(P=_cuda(dirty2))
    oh, od = _outcome(h, h.solve()), _outcome(d, d.solve())
    _assert_same_outcome(oh, od, "NaN below the diagonal of P, update")
    assert all(np.isfinite(v).all() for v in od["result"].values())


# ---------------------------------------------------------------------------------------------- 4. rows of G without a finite bound
def _with_free_row(q, row):
    hl = np.full(q["G"].shape[0], -np.inf) if q["h_l"] is None else q["h_l"].copy()
    hu = np.full(q["G"].shape[0], np.inf) if q["h_u"] is None else q["h_u"].copy()
    hl[row] = -np.inf; hu[row] = np.inf
    return hl, hu


@pytest.mark.parametrize("solver", ["SPARSE_LDLT", "SPARSE_LDLT_MULTIFRONTAL", "SPARSE_LDLT_INEQ_COND"])
def test_doubly_infinite_row_of_G_at_setup(hip, solver):
    q = _case(FULL)
    row = int(np.argmax(np.diff(q["G"].T.tocsc().indptr)))  # the row of G with most entries
    q["h_l"], q["h_u"] = _with_free_row(q, row)
    before = q["G"].data.copy()
    g = _to_gpu(q)
    h, d = _new_solver(hip, _ks(hip, solver)), _new_solver(hip, _ks(hip, solver))
    assert h.setup(**q) and d.setup(**g)
    _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), "row disabled at setup")
    assert np.array_equal(g["G"][1].cpu().numpy(), before)  # the row is zeroed in the solver's copy, the caller's array is only read
    # a later update of G alone, and one that states the infinite bounds again (data.hpp:144-169 then zeroes the row of the new G too)
    rng = np.random.default_rng(9)
    G2 = _perturbed(q["G"], rng, 0.01)
    assert h.update(G=G2) and d.update(G=_cuda(G2.data))
    _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), "update(G) after a disabled row")
    assert h.update(G=G2, h_l=q["h_l"], h_u=q["h_u"]) and d.update(G=_cuda(G2.data), h_l=_cuda(q["h_l"]), h_u=_cuda(q["h_u"]))
    _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), "update(G, h_l, h_u) keeps the row disabled")


@pytest.mark.parametrize("solver", ["SPARSE_LDLT", "SPARSE_LDLT_MULTIFRONTAL"])
def test_doubly_infinite_row_of_G_after_an_update_of_the_bounds(hip, solver):
    q = _case(FULL)
    row = int(np.argmax(np.diff(q["G"].T.tocsc().indptr)))
    h, d = _pair(hip, q, _ks(hip, solver))
    _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), "after setup")
    hl, hu = _with_free_row(q, row)
    assert h.update(h_l=hl, h_u=hu) and d.update(h_l=_cuda(hl), h_u=_cuda(hu))  # vectors only: the stored row is zeroed by the kernel
    assert d.last_ingest() == (0, 0)
    _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), "row disabled by update(h_l, h_u)")
    rng = np.random.default_rng(11)
    G2 = _perturbed(q["G"], rng, 0.01)
    assert h.update(G=G2, h_l=hl, h_u=hu) and d.update(G=_cuda(G2.data), h_l=_cuda(hl), h_u=_cuda(hu))
    _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), "update(G, h_l, h_u) keeps the row disabled")


# ---------------------------------------------------------------------------------------------- 5. the backends on their own
def _args(q):
    return tuple(q[k] for k in NAMES)


def _scalings(n, m, rng, late):
    """the two regimes of tests/test_exact_gpu.py"""
    if not late:
        return 1e-4, np.full(n, 1e-6), np.abs(rng.standard_normal(m)) + 0.1
    return 1e-10, np.full(n, 1e-10), np.exp(rng.uniform(-18.0, 12.0, m))


def _scale_values(d, f):
    d.P_utri.data *= f; d.AT.data *= 2.0 - f; d.GT.data *= f


@pytest.mark.parametrize("solver", ["SPARSE_LDLT_EXACT", "SPARSE_LDLT_MULTIFRONTAL", "SPARSE_LDLT", "SPARSE_LDLT_EQ_COND", "SPARSE_LDLT_INEQ_COND", "SPARSE_LDLT_COND", "SPARSE_MULTISTAGE"])
def test_backend_from_a_device_mode_descriptor(hip, solver):
    name = MPC if solver == "SPARSE_MULTISTAGE" else FULL
    q = _case(name)
    ks = hip.SPARSE_MULTISTAGE if solver == "SPARSE_MULTISTAGE" else _ks(hip, solver)
    dh, dd = hip.SparseData(*_args(q)), hip.SparseData(*_args(q)).to_device()
    assert dd.descriptor().mem == hip.MEM_DEVICE and dh.descriptor().mem == hip.MEM_HOST
    kh, kd = hip.SparseKKT(dh, kkt_solver=ks), hip.SparseKKT(dd, kkt_solver=ks)
    n, p, m = dh.n, dh.p, dh.m
    rng = np.random.default_rng(17)

    def compare(handles, what):
        for late in (False, True):
            delta, x_reg, z_reg = _scalings(n, m, rng, late)
            oks = [k.update_scalings_and_factor(delta, x_reg, z_reg) for k in handles]
            assert all(o == oks[0] for o in oks), (what, late, oks)
            assert oks[0] or late, (what, "the early regime must factor: a test that skips both regimes tests nothing")
            if not oks[0]:
                continue
            if solver == "SPARSE_LDLT_EXACT":
                fs = [k.exact_factor() for k in handles]
                for f in fs[1:]:
                    assert set(f) == set(fs[0])
                    for key in f:
                        assert np.array_equal(f[key], fs[0][key]) and (f[key].dtype != np.float64 or _same_bits(f[key], fs[0][key])), (what, late, key)
            for _ in range(2):
                rx, ry, rz = rng.standard_normal(n), rng.standard_normal(p), rng.standard_normal(m)
                ls = [k.solve(rx, ry, rz) for k in handles]
                for l in ls[1:]:
                    for a, b, nm in zip(l, ls[0], "xyz"):
                        assert _same_bits(np.asarray(a), np.asarray(b)), (what, late, "solve", nm)
            x = rng.standard_normal(n)
            zs = [k.eval_P_x(1.5, x) for k in handles]
            assert all(_same_bits(z, zs[0]) for z in zs[1:]), (what, "eval_P_x")

    compare([kh, kd], "create")
    twin = kd.clone()
    compare([kh, kd, twin], "clone of a device-fed handle")
    _scale_values(dh, 1.03); _scale_values(dd, 1.03)
    dd.to_device()
    kh.update_data(dh, 7); kd.update_data(dd, 7); twin.update_data(dd, 7)
    compare([kh, kd, twin], "update_data")


@pytest.mark.parametrize("solver", ["SPARSE_LDLT", "SPARSE_LDLT_COND"])
def test_kkt_system_from_a_device_mode_descriptor(hip, solver):
    from qp_gen import random_vars
    q = _case(FULL)
    dh, dd = hip.SparseData(*_args(q)), hip.SparseData(*_args(q))
    rng = np.random.default_rng(5)
    xbs = rng.uniform(0.5, 2.0, dh.n)
    dh.x_b_scaling = xbs.copy(); dd.x_b_scaling = xbs.copy()
    dd.to_device()
    set_h, set_d = hip.default_settings(kkt_solver=_ks(hip, solver)), hip.default_settings(kkt_solver=_ks(hip, solver))
    kh, kd = hip.KKTSystem(dh, set_h), hip.KKTSystem(dd, set_d)
    state, rhs = random_vars(dh.n, dh.p, dh.m, rng, positive=True), random_vars(dh.n, dh.p, dh.m, rng)

    def compare(what):
        assert kh.update_scalings_and_factor(True, 1e-6, 1e-4, state) and kd.update_scalings_and_factor(True, 1e-6, 1e-4, state)
        (okh, lh), (okd, ld) = kh.solve(rhs), kd.solve(rhs)
        assert okh and okd
        for k in lh:
            assert _same_bits(lh[k], ld[k]), (what, k)

    compare("create")
    _scale_values(dh, 0.98); _scale_values(dd, 0.98)
    dh.x_b_scaling = xbs * 1.1; dd.x_b_scaling = xbs * 1.1
    dd.to_device()
    kh.update_data(dh, 7); kd.update_data(dd, 7)
    compare("update_data")


# ---------------------------------------------------------------------------------------------- 6. bad arguments
def test_invalid_mem_is_refused_and_leaves_the_handles_usable(hip):
    L = hip._lib.load()
    PQ_ERR_INVALID = -1
    q = _case(FULL)
    # the solver entry points
    s, ref = _new_solver(hip, hip.SPARSE_LDLT), _new_solver(hip, hip.SPARSE_LDLT)
    assert s.setup(**_to_gpu(q)) and ref.setup(**q)
    first = _outcome(ref, ref.solve())
    _assert_same_outcome(first, _outcome(s, s.solve()), "before")
    csc = lambda M: [np.ascontiguousarray(M.indptr, dtype=np.int32), np.ascontiguousarray(M.indices, dtype=np.int32), _cuda(M.data)]
    vec = lambda v: None if v is None else _cuda(v)
    keep = csc(q["P"]) + [vec(q["c"])] + csc(q["A"]) + [vec(q["b"])] + csc(q["G"]) + [vec(q[k]) for k in ("h_l", "h_u", "x_l", "x_u")]
    ptr = lambda a: None if a is None else (a.data_ptr() if torch.is_tensor(a) else a.ctypes.data)
    fifteen = [ptr(a) for a in keep]
    n, p, m = q["P"].shape[0], q["A"].shape[0], q["G"].shape[0]
    torch.cuda.synchronize()
    for mem in (7, -1, 2):
        assert L.pq_solver_setup_sparse_mem(s.h, n, p, m, *fifteen, mem) == PQ_ERR_INVALID
        assert b"PQ_MEM" in L.pq_last_error_string()
        assert L.pq_solver_update_sparse_mem(s.h, *fifteen, mem) == PQ_ERR_INVALID
    _assert_same_outcome(_outcome(ref, ref.solve()), _outcome(s, s.solve()), "after refused solver calls")
    # the same calls with a valid mem go through (the index arrays given, and not given)
    assert L.pq_solver_update_sparse_mem(s.h, *fifteen, hip.MEM_DEVICE) == 1
    assert ref.update(**q)
    _assert_same_outcome(_outcome(ref, ref.solve()), _outcome(s, s.solve()), "after a raw device-mode update")
    no_idx = list(fifteen)
    for i in (0, 1, 4, 5, 8, 9):
        no_idx[i] = None
    assert L.pq_solver_update_sparse_mem(s.h, *no_idx, hip.MEM_DEVICE) == 1
    assert ref.update(**q)
    _assert_same_outcome(_outcome(ref, ref.solve()), _outcome(s, s.solve()), "after a raw device-mode update without index arrays")

    # the backend and KKTSystem entry points
    d = hip.SparseData(*_args(q))
    k = hip.SparseKKT(d, kkt_solver=hip.SPARSE_LDLT)
    sys_ = hip.KKTSystem(d, hip.default_settings(kkt_solver=hip.SPARSE_LDLT))
    rng = np.random.default_rng(1)
    delta, x_reg, z_reg = _scalings(d.n, d.m, rng, False)
    rx, ry, rz = rng.standard_normal(d.n), rng.standard_normal(d.p), rng.standard_normal(d.m)
    assert k.update_scalings_and_factor(delta, x_reg, z_reg)
    before = k.solve(rx, ry, rz)
    bad = d.descriptor()
    bad.mem = 7
    out = C.c_void_p()
    assert L.pq_kkt_create_sparse(C.byref(out), C.byref(bad), hip.SPARSE_LDLT, 0) == PQ_ERR_INVALID and not out.value
    assert L.pq_kkt_update_data_sparse(k.h, C.byref(bad), 7) == PQ_ERR_INVALID
    assert L.pq_kktsys_create_sparse(C.byref(out), C.byref(bad), C.byref(sys_.settings), 0) == PQ_ERR_INVALID and not out.value
    assert L.pq_kktsys_update_data_sparse(sys_.h, C.byref(bad), 7) == PQ_ERR_INVALID
    assert b"PQ_MEM" in L.pq_last_error_string()
    assert k.update_scalings_and_factor(delta, x_reg, z_reg)
    after = k.solve(rx, ry, rz)
    for a, b in zip(before, after):
        assert _same_bits(np.asarray(a), np.asarray(b))


# ---------------------------------------------------------------------------------------------- 7. results on the device, clone
def test_result_on_the_gpu_and_clone_of_a_device_fed_sparse_solver(hip):
    q = _case(FULL)
    d = _new_solver(hip, hip.SPARSE_LDLT)
    assert d.setup(**_to_gpu(q))
    twin = d.clone()
    twin.enable_trace()
    out = _outcome(d, d.solve())
    on_gpu = d.result(device=True)
    assert set(on_gpu) == set(out["result"])
    for k, v in on_gpu.items():
        assert v.is_cuda and v.dtype == torch.float64
        assert _same_bits(v.cpu().numpy(), out["result"][k]), k
    _assert_same_outcome(out, _outcome(twin, twin.solve()), "clone of a device-fed sparse solver")
    G2 = q["G"].copy(); G2.data = G2.data * 1.01
    assert d.update(G=_cuda(G2.data)) and twin.update(G=_cuda(G2.data))
    _assert_same_outcome(_outcome(d, d.solve()), _outcome(twin, twin.solve()), "clone, after update(G)")


def test_inputs_are_never_modified(hip):
    q = _case(FULL)
    row = 1
    q["h_l"], q["h_u"] = _with_free_row(q, row)
    g = _to_gpu(q)
    flat = {k: (v[1] if isinstance(v, tuple) else v) for k, v in g.items() if v is not None}
    before = {k: v.clone() for k, v in flat.items()}
    s = _new_solver(hip, hip.SPARSE_LDLT)
    assert s.setup(**g)
    assert s.update(**{k: flat[k] for k in flat})
    s.solve()
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(flat[k].view(torch.int64), v.view(torch.int64)), k
