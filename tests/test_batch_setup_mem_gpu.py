"""BatchSparseSolver.setup() from problem data in GPU memory (pq_batch_setup_sparse_mem with PQ_MEM_DEVICE): every test sets up twin handles on the same data, one
host-fed and one device-fed, and asks for equality of bits -- there is no tolerance anywhere in this file.  The twins are two entries into one setup path: the
host-fed one uploads the caller's arrays into a staging buffer and checks the shared finiteness pattern on the host, the device-fed one fetches instance 0's bound
vectors and checks the pattern with a kernel; from there both run the same kernels.  The host-fed setup is the one the other test_batch_* files hold to the oracle."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from batch_sparse_mixed import mixed_sparse_batch
from qp_gen import mpc_batch
from test_batch_ldlt_gpu import _random_sparse_qp_batch, _scalings

pytestmark = pytest.mark.gpu

TIMES = ("setup_time", "update_time", "solve_time", "kkt_factor_time", "kkt_solve_time", "run_time")
VARS = ("x", "y", "z_l", "z_u", "z_bl", "z_bu", "s_l", "s_u", "s_bl", "s_bu")
STACKS = ("Pv", "c", "Av", "b", "Gv", "h_l", "h_u", "x_l", "x_u")
PQ_ERR_INVALID = -1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _mpc(B):
    mb = mpc_batch(B)
    return dict(P=mb["P_pattern"], A=mb["A_pattern"], G=None, Pv=mb["P_values"], Av=mb["A_values"], Gv=None, c=mb["c"], b=mb["b"], h_l=None, h_u=None, x_l=mb["x_l"],
                x_u=mb["x_u"], B=B)


_batches = {}


def batch(kind, *key):
    """the test data, computed once per key; nobody changes it"""
    if (kind, key) not in _batches:
        _batches[(kind, key)] = {"random": lambda d, B: _random_sparse_qp_batch(d, B, seed=d), "mixed": mixed_sparse_batch, "mpc": _mpc}[kind](*key)
    return _batches[(kind, key)]


def on_gpu(a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def args_of(bt, device):
    cv = on_gpu if device else (lambda a: a)
    return (bt["P"], cv(bt["Pv"]), cv(bt["c"]), bt["A"], cv(bt["Av"]), cv(bt["b"]), bt["G"], cv(bt["Gv"]), cv(bt["h_l"]), cv(bt["h_u"]), cv(bt["x_l"]), cv(bt["x_u"]))


def new_solver(hip, kkt, bounds):
    return hip.BatchSparseSolver(kkt_solver=getattr(hip, kkt), bounds=bounds)


def twins(hip, bt, kkt="SPARSE_MULTISTAGE", bounds="shared", **settings):
    out = []
    for device in (False, True):
        s = new_solver(hip, kkt, bounds)
        for k, v in settings.items():
            setattr(s.settings, k, v)
        assert s.setup(*args_of(bt, device))
        out.append(s)
    return out


def same_structure(a, b):
    assert a.arena_stride() == b.arena_stride() > 0
    assert (a.batch, a.n, a.p, a.m) == (b.batch, b.n, b.p, b.m)
    for i in range(a.batch):
        la, lb = a.bound_lists(i), b.bound_lists(i)
        for k in ("h_l_idx", "h_u_idx", "x_l_idx", "x_u_idx", "dropped"):
            assert np.array_equal(la[k], lb[k]), (i, k, la[k], lb[k])


def same_solve(a, b):
    """solve both; statuses, iterations, the ten result vectors and every field of pq_info but the clocks"""
    assert a.solve() == b.solve()
    assert np.array_equal(a.statuses(), b.statuses()) and np.array_equal(a.iterations(), b.iterations())
    for k in VARS:
        assert _same_bits(a.result(k), b.result(k)), k
    for i in range(a.batch):
        ia, ib = a.info(i), b.info(i)
        for name, ct in ia._fields_:
            if name in TIMES:
                continue
            va, vb = getattr(ia, name), getattr(ib, name)
            assert (va == vb) if ct is C.c_int else _same_bits(np.array([va]), np.array([vb])), (i, name, va, vb)


def same_ldlt(a, b, seed=3):
    """sparse_ldlt: the factor of the stored data under both regimes of _scalings, every item of ldlt_factor(i), and a backend solve"""
    B, n, p, m = a.batch, a.n, a.p, a.m
    rng = np.random.default_rng(seed)
    for late in (False, True):
        sc = [_scalings(n, m, rng, late) for _ in range(B)]
        f = (np.array([s[0] for s in sc]), np.array([s[1] for s in sc]).reshape(B, n), np.array([s[2] for s in sc]).reshape(B, m))
        assert np.array_equal(a.kkt_factor(*f), b.kkt_factor(*f))
        for i in range(B):
            fa, fb = a.ldlt_factor(i), b.ldlt_factor(i)
            assert fa.keys() == fb.keys()
            for k in fa:
                assert np.array_equal(fa[k].view(np.uint8), fb[k].view(np.uint8)), (late, i, k)
        r = (rng.standard_normal((B, n)), rng.standard_normal((B, p)), rng.standard_normal((B, m)))
        for x, y in zip(a.kkt_solve(*r), b.kkt_solve(*r)):
            assert _same_bits(x, y), late


def same_twins(a, b, kkt):
    same_structure(a, b)
    if kkt == "SPARSE_LDLT":
        same_ldlt(a, b)
    same_solve(a, b)


KKTS = ("SPARSE_MULTISTAGE", "SPARSE_LDLT")


# ---- 1. twins, both backends x both bound modes ---------------------------------------------------------------------------------------------------------------
# shared sets: the generator's own infinities are in (h_l[:, ::5], x_u[:, ::3]); nnz counts and lengths are below one workgroup and no multiples of 64 or 128;
# B = 1, 5, 67 is a multiple of nothing; (16, *) and (33, *) differ in the parity of their arena rows' lengths
@pytest.mark.parametrize("kkt", KKTS)
@pytest.mark.parametrize("dim,B", [(16, 1), (16, 5), (33, 5), (33, 67)])
def test_twins_with_shared_bound_sets(hip, kkt, dim, B):
    bt = batch("random", dim, B)
    assert not np.isfinite(bt["h_l"]).all() and not np.isfinite(bt["x_u"]).all()
    a, b = twins(hip, bt, kkt)
    same_twins(a, b, kkt)
    assert (b.statuses() == 1).all(), "these QPs solve (tests/test_batch_ldlt_gpu.py): equal bits of two failures would show nothing"


@pytest.mark.parametrize("kkt", KKTS)
def test_twins_on_the_mpc_batch(hip, kkt):
    a, b = twins(hip, batch("mpc", 64), kkt)
    same_twins(a, b, kkt)
    assert (b.statuses() == 1).all()


def test_one_of_the_twin_shapes_has_an_odd_arena_row(hip):
    """every slot of the arena is padded to an even length, so the row itself is even: "odd" is a row whose slots are NOT all even before the padding, which is
    where a fill that ignored the padding would go wrong: n = 33 (c, the boxes, x_b_scaling) against n = 16"""
    a = new_solver(hip, "SPARSE_LDLT", "shared")
    assert a.setup(*args_of(batch("random", 33, 5), True))
    assert a.n % 2 == 1 and a.arena_stride() % 2 == 0


@pytest.mark.parametrize("kkt", KKTS)
@pytest.mark.parametrize("dim,B", [(16, 8), (33, 9)])
def test_twins_with_per_instance_bound_sets(hip, kkt, dim, B):
    """the five forced kinds are in: every row dropped, no box at all, no finite bound at all"""
    bt = batch("mixed", dim, B)
    a, b = twins(hip, bt, kkt, bounds="per_instance")
    drop = np.array([b.bound_lists(i)["dropped"].all() for i in range(B)])
    nobox = np.array([len(b.bound_lists(i)["x_l_idx"]) + len(b.bound_lists(i)["x_u_idx"]) == 0 for i in range(B)])
    assert drop.any() and nobox.any() and (drop & nobox).any() and not drop.all()
    same_twins(a, b, kkt)


# ---- 2. absent arguments: "absent means none finite" -----------------------------------------------------------------------------------------------------------
def _without(bt, *keys, A=True, G=True):
    out = dict(bt)
    for k in keys:
        out[k] = None
    if not A:
        out.update(A=None, Av=None, b=None)
    if not G:
        out.update(G=None, Gv=None, h_l=None, h_u=None)
    return out


ABSENT = {"m=0": dict(G=False), "p=0": dict(A=False), "h_l=None": dict(keys=("h_l",)), "h_u=None": dict(keys=("h_u",)), "x_l=None": dict(keys=("x_l",)),
          "x_u=None": dict(keys=("x_u",)), "no box": dict(keys=("x_l", "x_u")), "no bound vector": dict(keys=("h_l", "h_u", "x_l", "x_u"))}


@pytest.mark.parametrize("bounds", ["shared", "per_instance"])
@pytest.mark.parametrize("kkt", KKTS)
@pytest.mark.parametrize("case", sorted(ABSENT))
def test_absent_arguments(hip, kkt, bounds, case):
    base = batch("random", 16, 5) if bounds == "shared" else batch("mixed", 16, 8)
    spec = ABSENT[case]
    bt = _without(base, *spec.get("keys", ()), A=spec.get("A", True), G=spec.get("G", True))
    a, b = twins(hip, bt, kkt, bounds=bounds)
    same_twins(a, b, kkt)


# ---- 3. P given in full: the strictly lower entries are never loaded --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kkt", KKTS)
def test_full_P_with_nan_below_the_diagonal(hip, kkt):
    bt = batch("random", 33, 5)
    U = bt["P"]
    F = sp.csc_matrix(U + sp.triu(U, 1).T)
    F.sort_indices()
    cols = np.repeat(np.arange(F.shape[1]), np.diff(F.indptr))
    lower = F.indices > cols
    assert lower.any()
    clean = np.zeros((bt["B"], F.nnz))
    for i in range(bt["B"]):
        Ui = sp.csc_matrix((bt["Pv"][i], U.indices, U.indptr), shape=U.shape)
        Fi = (Ui + sp.triu(Ui, 1).T).toarray()
        clean[i] = Fi[F.indices, cols]
    dirty = clean.copy()
    dirty[:, lower] = np.nan
    a = new_solver(hip, kkt, "shared")
    b = new_solver(hip, kkt, "shared")
    full = dict(bt, P=F)
    assert a.setup(*args_of(dict(full, Pv=clean), False))
    assert b.setup(*args_of(dict(full, Pv=dirty), True))
    same_twins(a, b, kkt)
    # and the upper triangle alone gives the same bits again
    c = new_solver(hip, kkt, "shared")
    assert c.setup(*args_of(bt, True))
    same_solve(b, c)


# ---- 4. life after a device setup -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", ["shared", "per_instance"])
@pytest.mark.parametrize("kkt", KKTS)
def test_updates_and_clones_after_a_device_setup(hip, kkt, bounds):
    bt = batch("random", 16, 5) if bounds == "shared" else batch("mixed", 16, 8)
    a, b = twins(hip, bt, kkt, bounds=bounds)
    same_solve(a, b)
    rng = np.random.default_rng(8)
    fin = lambda v, d: np.where(np.isfinite(v), v + d, v)
    nb, nxl = bt["b"] + 0.01 * rng.standard_normal(bt["b"].shape), fin(bt["x_l"], -0.125)
    for s in (a, b):
        assert s.update(b=nb, x_l=nxl)
    same_solve(a, b)
    nb2, nxl2 = bt["b"] - 0.02, fin(bt["x_l"], -0.25)
    for s in (a, b):
        assert s.update(b=on_gpu(nb2), x_l=on_gpu(nxl2))
    same_solve(a, b)
    for reuse in (0, 1):
        Pv, Gv = bt["Pv"] * (1.0 + 0.05 * (reuse + 1)), bt["Gv"] * (1.0 - 0.03 * (reuse + 1))
        hl, hu = fin(bt["h_l"], -0.5), fin(bt["h_u"], 0.25 * (reuse + 1))
        for s in (a, b):
            s.settings.preconditioner_reuse_on_update = reuse
            assert s.update_data(P_values=Pv, G_values=Gv, h_l=hl, h_u=hu)
        same_structure(a, b)
        same_solve(a, b)
    ca, cb = a.clone([2, 0, 0]), b.clone([2, 0, 0])
    same_structure(ca, cb)
    same_solve(ca, cb)


@pytest.mark.parametrize("kkt", KKTS)
def test_a_second_setup_on_the_same_handle(hip, kkt):
    """host then device and device then host, other data and another shape the second time"""
    first, second = batch("random", 16, 5), batch("random", 33, 5)
    hd, dh = new_solver(hip, kkt, "shared"), new_solver(hip, kkt, "shared")
    assert hd.setup(*args_of(first, False)) and dh.setup(*args_of(first, True))
    same_solve(hd, dh)
    assert hd.setup(*args_of(second, True)) and dh.setup(*args_of(second, False))
    same_twins(dh, hd, kkt)


@pytest.mark.parametrize("bounds", ["shared", "per_instance"])
@pytest.mark.parametrize("kkt", KKTS)
def test_a_host_setup_over_another_problem_is_a_fresh_one(hip, kkt, bounds):
    """the re-setup path of the host mode: the handle holds another problem -- other data, another shape, more instances, the list buffer of a solve by list -- when
    it is set up from host arrays.  Nothing of the old table of lists, list buffer or finiteness copies may show: every arena row and every bound list is bitwise a
    fresh handle's, and so is what an update (checked against the finiteness copies) and a solve by list (through the list buffer) make of them"""
    old, bt = (batch("random", 33, 67), batch("random", 16, 5)) if bounds == "shared" else (batch("mixed", 33, 9), batch("mixed", 16, 5))
    s, fresh = new_solver(hip, kkt, bounds), new_solver(hip, kkt, bounds)
    assert s.setup(*args_of(old, False))
    s.solve(instances=[1, 0])
    assert s.setup(*args_of(bt, False)) and fresh.setup(*args_of(bt, False))
    same_structure(s, fresh)
    for i in range(bt["B"]):
        assert np.array_equal(_bits(s.arena_row(i)), _bits(fresh.arena_row(i))), i
    for h in (s, fresh):
        assert h.update(x_l=bt["x_l"], h_u=bt["h_u"])
        h.solve(instances=[4, 2])
    for i in range(bt["B"]):
        assert np.array_equal(_bits(s.arena_row(i)), _bits(fresh.arena_row(i))), i


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,value", [("h_l", -np.inf), ("h_u", np.inf), ("x_l", -np.inf), ("x_u", 1.0)])
def test_shared_mode_refuses_an_instance_with_another_finiteness(hip, key, value):
    bt = dict(batch("random", 16, 5))
    v = bt[key].copy()
    j = 2 if key != "x_u" else 0  # x_u[:, 0] is infinite in the generator's batch: one instance gets a finite one
    assert np.isfinite(v[3, j]) != np.isfinite(value)
    v[3, j] = value
    bt[key] = v
    texts = []
    for device in (False, True):
        s = new_solver(hip, "SPARSE_MULTISTAGE", "shared")
        with pytest.raises(RuntimeError) as e:
            s.setup(*args_of(bt, device))
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "batch setup: instances differ in which bounds are finite" in texts[0]


def _raw_setup(s, bt, mem, ptr):
    Pp, Pi, Pm = s._pattern(bt["P"])
    Ap, Ai, Am = s._pattern(bt["A"])
    Gp, Gi, Gm = s._pattern(bt["G"])
    n, p, m = Pm.shape[0], Am.shape[0], Gm.shape[0]
    keep = [np.ascontiguousarray(bt[k]) for k in STACKS]
    d = dict(zip(STACKS, keep))
    a = [Pp.ctypes.data, Pi.ctypes.data, ptr(d["Pv"]), ptr(d["c"]), Ap.ctypes.data, Ai.ctypes.data, ptr(d["Av"]), ptr(d["b"]), Gp.ctypes.data, Gi.ctypes.data, ptr(d["Gv"]),
         ptr(d["h_l"]), ptr(d["h_u"]), ptr(d["x_l"]), ptr(d["x_u"])]
    return s.L.pq_batch_setup_sparse_mem(s.h, bt["B"], n, p, m, *a, mem)


def test_an_unknown_mem_is_refused_and_the_handle_stays_as_it_was(hip):
    bt, other = batch("random", 16, 5), batch("random", 33, 5)
    a, b = twins(hip, bt)
    assert _raw_setup(b, other, 7, lambda v: v.ctypes.data) == PQ_ERR_INVALID
    assert "mem" in b.L.pq_last_error_string().decode()
    same_structure(a, b)
    same_solve(a, b)


def _wide_batch(n):
    """B = 2 diagonal QPs with n variables, box bounds: n + p + m = n"""
    P = sp.identity(n, format="csc")
    return dict(P=P, A=None, G=None, Pv=np.ones((2, n)), Av=None, Gv=None, c=np.ones((2, n)), b=None, h_l=None, h_u=None, x_l=-np.ones((2, n)), x_u=np.ones((2, n)), B=2)


def test_the_backend_refusals_are_the_host_modes(hip):
    wide = _wide_batch(8200)
    texts = []
    for device in (False, True):
        s = new_solver(hip, "SPARSE_LDLT", "shared")
        with pytest.raises(RuntimeError) as e:
            s.setup(*args_of(wide, device))
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "n + p + m <= 8192" in texts[0] and "8200" in texts[0]
    texts = []
    for device in (False, True):
        s = hip.BatchSparseSolver(kkt_solver=4)  # sparse_ldlt_cond: a condensed backend
        with pytest.raises(RuntimeError) as e:
            s.setup(*args_of(batch("random", 16, 5), device))
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "kkt_solver must be sparse_multistage, sparse_ldlt or sparse_ldlt_exact" in texts[0]


def test_the_wrapper_refuses_bad_tensors(hip):
    import torch
    bt = batch("random", 16, 5)
    s = new_solver(hip, "SPARSE_MULTISTAGE", "shared")
    good = list(args_of(bt, True))
    c = 2  # the position of c in the argument list
    for bad, err in ((good[c].float(), TypeError), (good[c][:, :-1], ValueError), (good[c][:-1], ValueError), (torch.as_tensor(bt["c"]), TypeError)):
        a = list(good)
        a[c] = bad
        with pytest.raises(err):
            s.setup(*a)
    # numpy beside tensors is moved for the caller, a strided view is made contiguous
    a = list(args_of(bt, False))
    wide = on_gpu(np.repeat(bt["Pv"], 2, axis=1))
    a[1] = wide[:, ::2]
    assert not a[1].is_contiguous() and s.setup(*a)
    t = new_solver(hip, "SPARSE_MULTISTAGE", "shared")
    assert t.setup(*args_of(bt, False))
    same_twins(t, s, "SPARSE_MULTISTAGE")


# ---- 6. no link traffic, no staging ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", ["shared", "per_instance"])
def test_last_ingest_and_the_allocation_count(hip, bounds):
    bt = batch("random", 16, 5) if bounds == "shared" else batch("mixed", 16, 8)
    B = bt["B"]
    count = hip._lib.load().pq_debug_alloc_count
    moved = []
    for device in (False, True):
        s = new_solver(hip, "SPARSE_LDLT", bounds)
        args = args_of(bt, device)
        c0 = count()
        assert s.setup(*args)
        moved.append(count() - c0)
        n, m = s.n, s.m
        got = s.last_ingest()
        # header: what the ingest kernels write, 8 x B x (the stored nonzeros of upper(P), A', G' + the lengths of the given c, b, x_l, x_u + 2 m + n)
        K = 8 * B * (sp.triu(bt["P"]).nnz + bt["A"].nnz + bt["G"].nnz + sum(bt[k].shape[1] for k in ("c", "b", "x_l", "x_u")) + 2 * m + n)
        if device:
            # header: the fetch of instance 0's h_l, h_u, x_l, x_u, and not a byte of the matrices
            assert got == dict(link_bytes=8 * (2 * m + 2 * n), kernel_bytes=K)
        else:
            given = sum(bt[k].shape[1] for k in STACKS)
            assert got == dict(link_bytes=8 * B * given, kernel_bytes=K)
        ms = s.setup_ms()
        assert ms["wall_ms"] > 0 and 0 < ms["analysis_ms"] < ms["wall_ms"] and 0 < ms["device_ms"] < ms["wall_ms"]
    # the host mode uploads the caller's arrays into one staging buffer; every other device buffer of a setup is made by both modes
    assert moved[0] == moved[1] + 1 > 1
    # only the vectors that are given are fetched; an update in device mode moves nothing
    s = new_solver(hip, "SPARSE_LDLT", bounds)
    assert s.setup(*args_of(_without(bt, "h_l", "x_u"), True))
    assert s.last_ingest()["link_bytes"] == 8 * (s.m + s.n)
    assert s.update(b=on_gpu(bt["b"]))
    assert s.last_ingest() == dict(link_bytes=0, kernel_bytes=8 * B * s.p)
    assert s.update(b=bt["b"])
    assert s.last_ingest() == dict(link_bytes=8 * B * s.p, kernel_bytes=8 * B * s.p)


def test_the_read_outs_of_a_fresh_handle_and_of_a_clone_are_zero(hip):
    s = new_solver(hip, "SPARSE_MULTISTAGE", "shared")
    assert s.last_ingest() == dict(link_bytes=0, kernel_bytes=0) and s.setup_ms() == dict(wall_ms=0.0, analysis_ms=0.0, device_ms=0.0)
    assert s.setup(*args_of(batch("random", 16, 5), True))
    c = s.clone()
    assert c.last_ingest() == dict(link_bytes=0, kernel_bytes=0) and c.setup_ms() == dict(wall_ms=0.0, analysis_ms=0.0, device_ms=0.0)
