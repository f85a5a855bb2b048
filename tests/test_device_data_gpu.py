"""Problem data taken from GPU memory and results returned there (pq_solver_*_mem, pq_batch_*_mem; csrc/ingest_kernels.hip).

Ingestion is copies, a transpose and a triangle mask: no arithmetic.  Every comparison below is therefore BITWISE against the host-fed path (uint64 views,
no tolerance anywhere), after the host-fed path has been shown to repeat itself bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from qp_gen import dense_strongly_convex_qp, mpc_batch
from qp_io import dense_args, load_qp

pytestmark = pytest.mark.gpu

NAMES = ("P", "c", "A", "b", "G", "h_l", "h_u", "x_l", "x_u")
LAYOUTS = ("row", "col")
FIXTURES = ("mm_QAFIRO", "mm_HS118", "mm_DUAL1", "mm_CVXQP1_S")
GENERATED = {"c1_200_50_100": (200, 50, 100, 7), "offtile_257_33_129": (257, 33, 129, 11), "no_eq_96_0_40": (96, 0, 40, 3), "one_tile_64_64_64": (64, 64, 64, 5)}


def _case(name):
    if name in GENERATED:
        n, p, m, seed = GENERATED[name]
        return dense_strongly_convex_qp(n, p, m, seed=seed)
    return dict(zip(NAMES, dense_args(load_qp(name))))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _matrix_to_gpu(M, layout):
    """a CUDA tensor holding M, stored row by row ("row") or column by column ("col": a transposed view, which is what a column-major matrix is in torch)"""
    if layout == "row":
        return torch.from_numpy(np.ascontiguousarray(M, dtype=np.float64)).cuda()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(M, dtype=np.float64).T)).cuda().t()


def _to_gpu(q, layout):
    out = {}
    for k, v in q.items():
        if v is None:
            out[k] = None
        elif k in ("P", "A", "G"):
            out[k] = _matrix_to_gpu(v, layout)
        else:
            out[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()
    return out


def _new_solver(hip, kkt_solver=None, reuse=None):
    s = hip.DenseSolver()
    if kkt_solver is not None:
        s.settings.kkt_solver = kkt_solver
    if reuse is not None:
        s.settings.preconditioner_reuse_on_update = int(reuse)
    s.enable_trace()
    return s


def _outcome(s, status):
    return dict(status=status, iter=s.info.iter, trace=s.trace(), result=s.result())


def _solve(hip, q, kkt_solver=None):
    s = _new_solver(hip, kkt_solver)
    assert s.setup(**q)
    return s, _outcome(s, s.solve())


def _assert_same_outcome(a, b, what):
    assert a["status"] == b["status"], (what, a["status"], b["status"])
    assert a["iter"] == b["iter"], (what, a["iter"], b["iter"])
    assert _same_bits(a["trace"], b["trace"]), (what, "trace")
    assert set(a["result"]) == set(b["result"]) and len(a["result"]) == 10
    for k in a["result"]:
        assert _same_bits(a["result"][k], b["result"][k]), (what, k)


# ---------------------------------------------------------------------------------------------- 1. dense solves bitwise
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(GENERATED) + list(FIXTURES))
def test_dense_solve_from_gpu_memory_is_bitwise_the_host_fed_one(hip, name, layout):
    q = _case(name)
    _, h1 = _solve(hip, q)
    _, h2 = _solve(hip, q)
    _assert_same_outcome(h1, h2, "host path repeated")
    assert h1["iter"] > 0
    _, d = _solve(hip, _to_gpu(q, layout))
    _assert_same_outcome(h1, d, f"{name} fed from the GPU ({layout}-major)")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_dense_solve_from_gpu_memory_reference_order_backend(hip, layout):
    q = _case("c1_200_50_100")
    _, h1 = _solve(hip, q, hip.DENSE_CHOLESKY_EXACT)
    _, h2 = _solve(hip, q, hip.DENSE_CHOLESKY_EXACT)
    _assert_same_outcome(h1, h2, "host path repeated")
    _, d = _solve(hip, _to_gpu(q, layout), hip.DENSE_CHOLESKY_EXACT)
    _assert_same_outcome(h1, d, "dense_cholesky_exact fed from the GPU")


def test_numpy_arguments_beside_gpu_tensors_are_moved_for_the_caller(hip):
    q = _case("offtile_257_33_129")
    _, h = _solve(hip, q)
    mixed = dict(q)
    mixed["G"] = _matrix_to_gpu(q["G"], "col")  # one CUDA matrix: P and A (numpy) follow it to the device
    s, d = _solve(hip, mixed)
    _assert_same_outcome(h, d, "mixed numpy / CUDA arguments")
    assert s.last_ingest()[0] == 0


# ---------------------------------------------------------------------------------------------- 2. the unread triangle of P
@pytest.mark.parametrize("layout", LAYOUTS)
def test_unread_triangle_of_P_never_reaches_the_solver(hip, layout):
    q = _case("offtile_257_33_129")
    n = q["P"].shape[0]
    clean = dict(q); clean["P"] = np.triu(q["P"])
    _, h = _solve(hip, clean)
    dirty = dict(q); dirty["P"] = np.triu(q["P"]) + np.tril(np.full((n, n), np.nan), -1)
    assert np.isnan(dirty["P"][n - 1, 0]) and not np.isnan(np.triu(dirty["P"])).any()
    _, d = _solve(hip, _to_gpu(dirty, layout))
    _assert_same_outcome(h, d, "NaN below the diagonal of P")
    # ... and through update(P) as well (an update unscales and rescales the stored data, so the yardstick is a host-fed solver taking the same two calls)
    r = _new_solver(hip)
    assert r.setup(**clean) and r.update(P=clean["P"])
    s = _new_solver(hip)
    g = _to_gpu(dirty, layout)
    assert s.setup(**g) and s.update(P=g["P"])
    _assert_same_outcome(_outcome(r, r.solve()), _outcome(s, s.solve()), "NaN below the diagonal of P, update")


# ---------------------------------------------------------------------------------------------- 3. inputs intact
@pytest.mark.parametrize("layout", LAYOUTS)
def test_inputs_are_never_modified(hip, layout):
    q = _case("c1_200_50_100")
    q["h_l"] = q["h_l"].copy(); q["h_u"] = q["h_u"].copy()
    q["h_l"][4] = -np.inf; q["h_u"][4] = np.inf  # a row of G the solver zeroes in ITS copy
    g = _to_gpu(q, layout)
    before = {k: v.clone() for k, v in g.items() if v is not None}
    s = _new_solver(hip)
    assert s.setup(**g)
    assert s.update(P=g["P"], A=g["A"], b=g["b"], G=g["G"], h_l=g["h_l"], h_u=g["h_u"], c=g["c"], x_l=g["x_l"], x_u=g["x_u"])
    s.solve()
    s.result(device=True)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(g[k].contiguous().view(torch.int64), v.contiguous().view(torch.int64)), k


# ---------------------------------------------------------------------------------------------- 4. updates
@pytest.mark.parametrize("reuse", [0, 1])
def test_updates_from_gpu_memory_stay_bitwise_the_host_fed_ones(hip, reuse):
    q = _case("offtile_257_33_129")
    rng = np.random.default_rng(17)
    n, p, m = q["P"].shape[0], q["A"].shape[0], q["G"].shape[0]
    h = _new_solver(hip, reuse=reuse)
    d = _new_solver(hip, reuse=reuse)
    assert h.setup(**q) and d.setup(**_to_gpu(q, "row"))
    _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), "after setup")

    def step(what, layout, **kw):
        assert h.update(**kw)
        assert d.update(**_to_gpu(kw, layout))
        assert d.last_ingest()[0] == 0
        _assert_same_outcome(_outcome(h, h.solve()), _outcome(d, d.solve()), (what, reuse))

    x0 = rng.standard_normal(n)
    P2 = q["P"] + np.diag(rng.uniform(0.1, 1.0, n))
    step("update(P)", "col", P=P2)
    A2 = q["A"] * (1.0 + 0.01 * rng.standard_normal((p, n)))
    step("update(A, b)", "col", A=A2, b=A2 @ x0)
    G2 = q["G"] * (1.0 + 0.01 * rng.standard_normal((m, n)))
    hu2 = np.where(np.isfinite(q["h_u"]), G2 @ x0 + 0.5, q["h_u"])
    step("update(G, h_u)", "row", G=G2, h_u=hu2)
    step("update(c, b)", "row", c=rng.standard_normal(n), b=A2 @ x0 + 1e-3)
    # a row of G loses both finite bounds: vectors only first (the stored row is zeroed), then together with a new G
    hl3, hu3 = q["h_l"].copy(), hu2.copy()
    hl3[2] = -np.inf; hu3[2] = np.inf
    step("update(h_l, h_u) disabling a row", "row", h_l=hl3, h_u=hu3)
    hl4, hu4 = hl3.copy(), hu3.copy()
    hl4[7] = -np.inf; hu4[7] = np.inf
    step("update(G, h_l, h_u) disabling a row", "col", G=q["G"], h_l=hl4, h_u=hu4)
    step("update(P, A, G) together", "row", P=q["P"], A=q["A"], G=G2, b=q["b"])


# ---------------------------------------------------------------------------------------------- 5. the ingest counter
def test_ingest_counter(hip):
    q = _case("c1_200_50_100")
    n, p, m = 200, 50, 100
    s = _new_solver(hip)
    assert s.setup(**q)
    assert s.last_ingest() == (8 * n * (n + p + m), 0)
    for layout in LAYOUTS:
        g = _to_gpu(q, layout)
        s = _new_solver(hip)
        assert s.setup(**g)
        link, dev = s.last_ingest()
        assert link == 0 and dev == 8 * n * (n + p + m)
        assert s.update(P=g["P"], G=g["G"])
        link, dev = s.last_ingest()
        assert link == 0 and dev == 8 * n * (n + m) > 0
        assert s.update(A=q["A"])  # a host-fed update of a device-fed solver
        assert s.last_ingest() == (8 * n * p, 0)


# ---------------------------------------------------------------------------------------------- 6. results on the GPU, clone
def test_result_on_the_gpu_and_clone_of_a_device_fed_solver(hip):
    q = _case("offtile_257_33_129")
    d = _new_solver(hip)
    assert d.setup(**_to_gpu(q, "col"))
    twin = d.clone()
    twin.enable_trace()
    out = _outcome(d, d.solve())
    on_gpu = d.result(device=True)
    assert set(on_gpu) == set(out["result"])
    for k, v in on_gpu.items():
        assert v.is_cuda and v.dtype == torch.float64
        assert _same_bits(v.cpu().numpy(), out["result"][k]), k
    _assert_same_outcome(out, _outcome(twin, twin.solve()), "clone of a device-fed solver")
    # the clone takes device-fed updates like the original
    g = _to_gpu(dict(G=q["G"] * 1.01), "row")
    assert d.update(**g) and twin.update(**g)
    _assert_same_outcome(_outcome(d, d.solve()), _outcome(twin, twin.solve()), "clone, after update(G)")


# ---------------------------------------------------------------------------------------------- 7. a tensor written on a side stream
def test_tensor_written_on_a_side_stream_is_ingested_whole(hip):
    q = _case("c1_200_50_100")
    _, h = _solve(hip, q)
    g = _to_gpu(q, "row")
    src = g["P"].clone()
    busy = torch.randn(4096, 4096, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = _new_solver(hip)
    with torch.cuda.stream(side):
        g["P"].zero_()
        for _ in range(8):
            busy = busy @ busy * 1e-3  # keeps the side stream busy ahead of the write below
        g["P"].copy_(src)
        assert s.setup(**g)  # the binding drains torch's current stream: the side stream
    _assert_same_outcome(h, _outcome(s, s.solve()), "P written on a side stream right before setup")


# ---------------------------------------------------------------------------------------------- 8. the batched solver
def _batch_pair(hip, mb, backend):
    pair = []
    for _ in range(2):
        bs = hip.BatchSparseSolver(kkt_solver=backend)
        assert bs.setup(mb["P_pattern"], mb["P_values"], mb["c"], mb["A_pattern"], mb["A_values"], mb["b"], x_l=mb["x_l"], x_u=mb["x_u"])
        pair.append(bs)
    return pair


def _assert_same_batch(a, b, what):
    assert np.array_equal(a.statuses(), b.statuses()), what
    assert np.array_equal(a.iterations(), b.iterations()), what
    for name in ("x", "y", "z_l", "z_u", "z_bl", "z_bu", "s_l", "s_u", "s_bl", "s_bu"):
        ra, rb = a.result(name), b.result(name)
        assert _same_bits(ra, rb), (what, name)
        on_gpu = b.result(name, device=True)
        assert on_gpu.is_cuda and tuple(on_gpu.shape) == ra.shape
        assert _same_bits(on_gpu.cpu().numpy(), rb), (what, name, "device=True")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@pytest.mark.parametrize("backend", ["SPARSE_MULTISTAGE", "SPARSE_LDLT"])
def test_batch_updates_and_results_in_gpu_memory(hip, backend):
    B = 256
    mb = mpc_batch(B, seed=1000)
    host, dev = _batch_pair(hip, mb, getattr(hip, backend))
    assert host.solve() == B and dev.solve() == B
    _assert_same_batch(host, dev, "after setup")
    rng = np.random.default_rng(5)
    b2 = mb["b"].copy()
    b2[:, :2] = rng.uniform(-0.8, 0.8, (B, 2))  # new initial states
    assert host.update(b=b2) and dev.update(b=_cuda(b2))
    host.solve(); dev.solve()
    _assert_same_batch(host, dev, "update(b)")
    assert (host.statuses() == 1).all()
    P2 = mb["P_values"] * rng.uniform(0.8, 1.25, mb["P_values"].shape)
    A2 = mb["A_values"] * (1.0 + 0.01 * rng.standard_normal(mb["A_values"].shape))
    c2 = 0.1 * rng.standard_normal(mb["c"].shape)
    xu2 = mb["x_u"] * 1.1
    assert host.update_data(P_values=P2, A_values=A2, c=c2, x_u=xu2)
    assert dev.update_data(P_values=_cuda(P2), A_values=_cuda(A2), c=_cuda(c2), x_u=xu2)  # (x_u: numpy beside CUDA tensors)
    host.solve(); dev.solve()
    _assert_same_batch(host, dev, "update_data(P, A, c, x_u)")
    assert host.update_data(P_values=mb["P_values"]) and dev.update_data(P_values=_cuda(mb["P_values"]))
    host.solve(); dev.solve()
    _assert_same_batch(host, dev, "update_data(P)")
    # a strided view is handed over as a contiguous copy
    wide = _cuda(np.concatenate([b2, b2], axis=1))
    assert host.update(b=b2) and dev.update(b=wide[:, : b2.shape[1]])
    host.solve(); dev.solve()
    _assert_same_batch(host, dev, "update(b) from a strided view")


@pytest.mark.parametrize("backend", ["SPARSE_MULTISTAGE", "SPARSE_LDLT"])
def test_batch_device_update_refuses_a_changed_set_of_finite_bounds(hip, backend):
    B = 256
    mb = mpc_batch(B, seed=1000)
    host, dev = _batch_pair(hip, mb, getattr(hip, backend))
    bad = mb["x_l"].copy()
    bad[B - 3, 5] = -np.inf
    with pytest.raises(RuntimeError) as eh:
        host.update(x_l=bad)
    with pytest.raises(RuntimeError) as ed:
        dev.update(x_l=_cuda(bad))
    msg = "the set of finite bounds differs from the one given at setup"
    assert msg in str(eh.value) and msg in str(ed.value)
    assert str(eh.value).split(":", 1)[1] == str(ed.value).split(":", 1)[1]
    with pytest.raises(RuntimeError, match=msg):
        dev.update_data(P_values=_cuda(mb["P_values"]), x_u=_cuda(np.where(np.arange(mb["n"]) == 1, np.inf, mb["x_u"])))
    # the refused calls changed nothing; an unchanged pattern passes the same check
    assert dev.update(x_l=_cuda(mb["x_l"]), x_u=_cuda(mb["x_u"])) and host.update(x_l=mb["x_l"], x_u=mb["x_u"])
    assert host.solve() == B and dev.solve() == B
    _assert_same_batch(host, dev, "after refused updates")


@pytest.mark.parametrize("backend", ["SPARSE_MULTISTAGE", "SPARSE_LDLT"])
def test_batch_device_round_trip_allocates_nothing(hip, backend):
    B = 256
    mb = mpc_batch(B, seed=1000)
    dev = _batch_pair(hip, mb, getattr(hip, backend))[1]
    assert dev.solve() == B
    L = hip._lib.load()
    b2, c2, P2, xl = _cuda(mb["b"] * 0.9), _cuda(mb["c"] * 1.1), _cuda(mb["P_values"] * 1.05), _cuda(mb["x_l"])
    torch.cuda.synchronize()
    before = L.pq_debug_alloc_count()
    assert dev.update(b=b2, x_l=xl)
    assert dev.solve() == B
    x = dev.result("x", device=True)
    assert dev.update_data(P_values=P2, c=c2, x_l=xl)
    assert dev.solve() == B
    y = dev.result("y", device=True)
    assert L.pq_debug_alloc_count() == before
    assert torch.isfinite(x).all() and torch.isfinite(y).all()


# ---------------------------------------------------------------------------------------------- 9. invalid arguments through the raw C-ABI
def test_invalid_mem_and_layout_are_refused_and_leave_the_handle_usable(hip):
    L = hip._lib.load()
    PQ_ERR_INVALID = -1
    q = _case("c1_200_50_100")
    s, h = _solve(hip, q)
    ref, _ = _solve(hip, q)  # goes through the same sequence of solves and updates, host-fed, without the refused calls
    g = _to_gpu(q, "row")
    ptr = lambda k: None if g[k] is None else g[k].data_ptr()
    nine = [ptr(k) for k in NAMES]
    torch.cuda.synchronize()
    for mem, layout in ((7, 0), (0, 7), (1, 7), (-1, 1), (2, 0)):
        assert L.pq_solver_setup_dense_mem(s.h, 200, 50, 100, *nine, mem, layout) == PQ_ERR_INVALID
        assert L.pq_solver_update_dense_mem(s.h, *nine, mem, layout) == PQ_ERR_INVALID
    out = hip.Variables.zeros(200, 50, 100)
    vs = hip.Variables.to_struct(out)
    assert L.pq_solver_get_result_mem(s.h, C.byref(vs), 7) == PQ_ERR_INVALID
    assert b"PQ_MEM" in L.pq_last_error_string()
    _assert_same_outcome(_outcome(ref, ref.solve()), _outcome(s, s.solve()), "after refused calls")
    # the same calls with valid arguments go through
    assert L.pq_solver_update_dense_mem(s.h, *nine, 1, 1) == 1
    assert ref.update(**q)
    _assert_same_outcome(_outcome(ref, ref.solve()), _outcome(s, s.solve()), "after a raw device-mode update")

    mb = mpc_batch(16, seed=1000)
    bs = _batch_pair(hip, mb, hip.SPARSE_MULTISTAGE)[0]
    b = _cuda(mb["b"])
    torch.cuda.synchronize()
    assert L.pq_batch_update_mem(bs.h, None, b.data_ptr(), None, None, None, None, 7) == PQ_ERR_INVALID
    assert L.pq_batch_update_data_mem(bs.h, None, None, None, None, b.data_ptr(), None, None, None, None, 7) == PQ_ERR_INVALID
    x = torch.zeros((16, mb["n"]), dtype=torch.float64, device="cuda")
    assert L.pq_batch_get_result_mem(bs.h, 0, x.data_ptr(), 7) == PQ_ERR_INVALID
    assert bs.solve() == 16
    assert L.pq_batch_get_result_mem(bs.h, 0, x.data_ptr(), 1) == 0
    assert _same_bits(x.cpu().numpy(), bs.result("x"))


# ---------------------------------------------------------------------------------------------- 10. host memory, row-major (raw C-ABI)
def test_host_row_major_matrices_are_bitwise_the_column_major_host_call(hip):
    """PQ_MEM_HOST with PQ_ROW_MAJOR: the host loops read C-ordered numpy arrays as they are (NaN below the diagonal of P included); the binding never
    sends this combination, so it goes through the raw entry points"""
    L = hip._lib.load()
    q = _case("offtile_257_33_129")
    n, p, m = 257, 33, 129
    ref, h = _solve(hip, q)
    rowq = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in q.items()}
    rowq["P"] = np.ascontiguousarray(np.triu(q["P"]) + np.tril(np.full((n, n), np.nan), -1))
    nine = [rowq[k].ctypes.data for k in NAMES]
    s = _new_solver(hip)
    assert L.pq_solver_setup_dense_mem(s.h, n, p, m, *nine, hip.MEM_HOST, hip.ROW_MAJOR) == 1
    assert s.last_ingest() == (8 * n * (n + p + m), 0)
    _assert_same_outcome(h, _outcome(s, s.solve()), "host row-major setup")
    G2 = np.ascontiguousarray(q["G"] * 1.01)
    assert ref.update(P=q["P"], A=q["A"], G=G2)
    upd = [rowq["P"].ctypes.data, None, rowq["A"].ctypes.data, None, G2.ctypes.data, None, None, None, None]
    assert L.pq_solver_update_dense_mem(s.h, *upd, hip.MEM_HOST, hip.ROW_MAJOR) == 1
    _assert_same_outcome(_outcome(ref, ref.solve()), _outcome(s, s.solve()), "host row-major update(P, A, G)")


def test_nested_list_beside_a_gpu_tensor_is_moved_like_a_numpy_array(hip):
    q = _case("one_tile_64_64_64")
    _, h = _solve(hip, q)
    mixed = dict(q)
    mixed["P"] = q["P"].tolist()
    mixed["A"] = _matrix_to_gpu(q["A"], "row")
    _, d = _solve(hip, mixed)
    _assert_same_outcome(h, d, "P as a nested list beside a CUDA tensor")
