"""The device Ruiz equilibration (piqp_amd/csrc/ruiz_kernels.hip: k_ruiz_sparse<GRID>, the six k_rzd_* kernels, launch_ruiz_sparse, DeviceRuiz::run) against
ruiz_reference of tests/ruiz_shapes.py, BIT FOR BIT -- the norms are maxima, every product has a fixed order, the one sum is sequential, so no tolerance is needed and
none is used.  tests/test_ruiz_shapes.py holds that reference to the oracle's ruiz_scale_data / ruiz_unscale_data on the same shapes.  One equilibration at a time
through pq_debug_ruiz -- no solver, no KKT backend, no symbolic analysis -- on the two paths production takes: the solver path (a DeviceRuiz as Solver::setup / update
drive it: the dense tiled kernels, or the sparse kernel on the grid or on one workgroup) and the kernel path (launch_ruiz_sparse on a strided arena of several instances
with the tail, as the batched solver launches it).  Every case compares every array the kernels may write, checks the guard doubles around the hook's buffers and the
sentinel below the diagonal of a dense P_utri, and compares the launch that was made with the plan of tests/ruiz_shapes.py."""
import ctypes as C

import numpy as np
import pytest

import ruiz_shapes as rs

pytestmark = pytest.mark.gpu

SOLVER = [s.name for s in rs.all_shapes() if s.kind in ("dense", "sparse")]
KERNEL = [s.name for s in rs.all_shapes() if s.kind == "batch" or s.also_kernel]
BOTH = [s.name for s in rs.all_shapes() if s.also_kernel]


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def same(got, want, what):
    gb, wb = rs.bits(got), rs.bits(want)
    assert gb.shape == wb.shape, (what, gb.shape, wb.shape)
    bad = np.nonzero(gb != wb)[0]
    assert bad.size == 0, (what, f"{bad.size} of {gb.size} entries differ in bits; first at {int(bad[0])}: "
                           f"{float(gb[bad[0]:bad[0] + 1].view(np.float64)[0])!r} != {float(wb[bad[0]:bad[0] + 1].view(np.float64)[0])!r}")


def check(got, want, what, tail=True):
    """every array of a (Problem, Scalings) pair of the device against the reference's"""
    (gq, gs), (wq, ws) = got, want
    for k in rs.FIELDS:
        if tail or k in ("P", "AT", "GT", "c", "xbs"):
            same(gq.values(k) if k in rs.MATS else getattr(gq, k), wq.values(k) if k in rs.MATS else getattr(wq, k), f"{what}: {k}")
    for k in rs.SCAL_FIELDS:
        same(getattr(gs, k), getattr(ws, k), f"{what}: {k}")
    same(np.array([gs.c]), np.array([ws.c]), f"{what}: cost scaling")


def run(hip, path, mode, insts, scale_cost=False, max_iter=10, scals=None, threads=1024, pad=0, tail="absent"):
    """one pq_debug_ruiz call on copies of the instances (one unless path == 'kernel') -> ([(Problem, Scalings)], guards or None, launch)"""
    L = hip._lib.load()
    lib = hip._lib
    q0 = insts[0]
    n, p, m, batch = q0.n, q0.p, q0.m, len(insts)
    N = n + p + m
    io = lib.RuizIO()
    io.path, io.mode = lib.RUIZ_PATHS.index(path), lib.RUIZ_MODES.index(mode)
    io.n, io.p, io.m, io.scale_cost, io.max_iter, io.batch, io.threads = n, p, m, int(scale_cost), max_iter, batch, threads
    keep = {}

    def stack(name, rows, dtype=np.float64):
        a = np.ascontiguousarray(np.stack([np.asarray(r, dtype=dtype).flatten(order="F") for r in rows]))
        keep[name] = a
        setattr(io, name, _ptr(a))
        return a

    if q0.sparse:
        for nm, M in (("P", q0.P), ("AT", q0.AT), ("GT", q0.GT)):
            for suffix, a in (("_colptr", M[0]), ("_rowind", M[1])):
                keep[nm + suffix] = np.ascontiguousarray(a, dtype=np.int32)
                setattr(io, nm + suffix, _ptr(keep[nm + suffix]))
    for nm in rs.MATS:
        stack(nm, [q.values(nm) for q in insts])
    stack("c", [q.c for q in insts]); stack("x_b_scaling", [q.xbs for q in insts])
    scals = scals or [None] * batch
    fill = lambda k: np.full(k, rs.SENTINEL)  # compute reads none of them
    stack("delta", [s.delta if s else fill(N) for s in scals]); stack("delta_inv", [s.delta_inv if s else fill(N) for s in scals])
    stack("delta_b", [s.delta_b if s else fill(n) for s in scals]); stack("delta_b_inv", [s.delta_b_inv if s else fill(n) for s in scals])
    stack("c_scale", [[s.c if s else rs.SENTINEL] for s in scals])
    lens = [keep[nm].shape[1] for nm in rs.MATS] + [n, n, N, N, n, n, n]
    if path == "kernel":
        lens += [p, m, m, q0.x_l_idx.size, q0.x_u_idx.size]
        present = sum(lens[:10])
        if tail != "absent":
            for k in ("b", "h_l", "h_u", "x_l", "x_u"):
                stack(k, [getattr(q, k) for q in insts])
            stack("x_l_idx", [q0.x_l_idx], np.int32); stack("x_u_idx", [q0.x_u_idx], np.int32)
            io.n_x_l, io.n_x_u = q0.x_l_idx.size, q0.x_u_idx.size
            present += sum(lens[10:])
        else:
            lens[13:] = [0, 0]  # (without x_l / x_u the hook is told of no index lists)
        io.stride = rs.GUARD + sum(k + rs.GUARD for k in lens) + pad
        total = batch * io.stride + rs.GUARD
        guards = np.zeros(total + 2 * rs.GUARD)
        io.guards, io.guards_cap = guards.ctypes.data, guards.size
    lib.check(L.pq_debug_ruiz(0, C.byref(io)), f"pq_debug_ruiz {path} {mode}")
    out = []
    for i, q in enumerate(insts):
        r = q.copy()
        for nm in rs.MATS:
            v, M = keep[nm][i].copy(), getattr(q, nm)
            setattr(r, nm, (M[0], M[1], v) if q.sparse else v.reshape(M.shape, order="F"))
        r.c, r.xbs = keep["c"][i].copy(), keep["x_b_scaling"][i].copy()
        if path == "kernel" and tail != "absent":
            for k in ("b", "h_l", "h_u", "x_l", "x_u"):
                setattr(r, k, keep[k][i].copy())
        out.append((r, rs.Scalings(*(keep[k][i].copy() for k in rs.SCAL_FIELDS), keep["c_scale"][i][0])))
    launch = (lib.RUIZ_LAUNCHES[io.launch[0]], io.launch[1], io.launch[2], io.launch[3])
    if path != "kernel":
        assert io.guards_len == 0
        return out, None, launch
    assert io.guards_len == total - batch * present + 2 * rs.GUARD, ("guard count", io.guards_len, total, present)
    return out, guards[:io.guards_len], launch


def intact(guards, what):
    bad = np.nonzero(rs.bits(guards) != rs.SENTINEL_BITS)[0]
    assert bad.size == 0, (what, f"{bad.size} of {guards.size} guard doubles overwritten; first at {int(bad[0])}: {float(guards[bad[0]])!r}")


def triangle_intact(q, what):
    if not q.sparse:
        lower = q.P[np.tril_indices(q.n, -1)]
        assert (rs.bits(lower) == rs.SENTINEL_BITS).all(), (what, "the strictly lower triangle of P_utri was written")


def solver_path(s):
    return "solver_dense" if s.kind == "dense" else "solver_sparse"


def plan(s):
    q = s.instances()[0]
    return rs.dense_plan(q.n, q.p, q.m)[0] if s.kind == "dense" else rs.sparse_plan(s.N, s.max_iter)


# ------------------------------------------------------------------------------------------------------------------- the solver path
@pytest.mark.parametrize("name", SOLVER)
def test_solver_path_compute_bitwise_the_reference(hip, name):
    s = rs.shape(name)
    ref = rs.chain(name, 0, True)
    (got,), _, launch = run(hip, solver_path(s), "compute", [ref["start"]], s.scale_cost, s.max_iter)
    print(f"{name}: {launch}, {ref['passes']} passes")
    assert launch == plan(s), (name, launch, plan(s))
    check(got, ref["compute"], name + " compute", tail=False)
    triangle_intact(got[0], name)


@pytest.mark.parametrize("name", SOLVER)
def test_solver_path_round_trip_bitwise_the_reference(hip, name):
    """compute -> unscale -> the second matrices assigned -> reuse, and -> compute again (what update() does with and without preconditioner_reuse_on_update), every
    step fed with what the device returned from the one before and compared with the reference (tests/test_ruiz_shapes.py: the cost scaling they multiply with is not 1)"""
    s = rs.shape(name)
    ref = rs.chain(name, 0, True)
    path = solver_path(s)
    ((q0, s0),), _, _ = run(hip, path, "compute", [ref["start"]], s.scale_cost, s.max_iter)
    check((q0, s0), ref["compute"], name + " compute", tail=False)
    (got,), _, launch = run(hip, path, "unscale", [q0], scals=[s0])
    check(got, ref["unscale"], name + " unscale", tail=False)
    assert launch == (plan(s) if s.kind == "dense" else rs.sparse_plan(s.N, 0)), launch  # (unscale passes max_iter = 0: s_N600_iter65 is on the grid here)
    triangle_intact(got[0], name + " unscale")
    assigned = got[0].with_matrices(s.seconds()[0].with_sentinel_triangle())
    (re,), _, _ = run(hip, path, "reuse", [assigned], scals=[got[1]])
    check(re, ref["reuse"], name + " reuse", tail=False)
    triangle_intact(re[0], name + " reuse")
    (rc,), _, _ = run(hip, path, "compute", [assigned], s.scale_cost, s.max_iter)
    check(rc, ref["recompute"], name + " compute after the update", tail=False)
    triangle_intact(rc[0], name + " compute after the update")


# ------------------------------------------------------------------------------------------------------------------- the kernel path
def kernel_args(s):
    """(threads, tail, pad) of a kernel-path run: a batch shape's own; a solver-path shape runs as PIQP_AMD_DEBUG=ruiz_one_wg would run it, with its full tail"""
    return (s.threads, s.tail, s.pad) if s.kind == "batch" else (1024, "full", 3)


@pytest.mark.parametrize("mode", rs.MODES)
@pytest.mark.parametrize("name", KERNEL)
def test_kernel_path_bitwise_the_reference(hip, name, mode):
    s = rs.shape(name)
    B = len(s.instances())
    threads, tail, pad = kernel_args(s)
    refs = [rs.chain(name, i) for i in range(B)]
    if mode == "compute":
        insts, scals = [r["start"] for r in refs], None
    elif mode == "unscale":
        insts, scals = [r["compute"][0] for r in refs], [r["compute"][1] for r in refs]
    else:
        insts, scals = [r["assigned"] for r in refs], [r["compute"][1] for r in refs]
    got, guards, launch = run(hip, "kernel", mode, insts, s.scale_cost, s.max_iter, scals, threads, pad, tail)
    assert launch == ("one_wg", B, 1, threads), launch
    intact(guards, f"{name} {mode}")
    for i in range(B):
        check(got[i], refs[i][mode], f"{name} {mode} instance {i} ({refs[i]['passes']} passes)", tail=tail != "absent")
        if tail == "absent":  # nothing of the tail is in the arena: the instances' own come back as they went
            for k in ("b", "h_l", "h_u", "x_l", "x_u"):
                same(getattr(got[i][0], k), getattr(insts[i], k), f"{name} {mode}: {k} without a tail")


@pytest.mark.parametrize("name", BOTH)
def test_the_paths_agree(hip, name):
    """one sparse problem through the solver path (the grid kernel from N = 513 on), through the one-workgroup kernel with 1024 threads and as both instances of a
    batch of two with the batched solver's thread count: the same bits, and the reference's"""
    s = rs.shape(name)
    ref = rs.chain(name, 0)
    q = ref["start"]
    (a,), _, la = run(hip, "solver_sparse", "compute", [q], s.scale_cost, s.max_iter)
    (b,), gb, lb = run(hip, "kernel", "compute", [q], s.scale_cost, s.max_iter, threads=1024, pad=2, tail="full")
    t2 = 64 if s.N <= 512 else 256
    (c0, c1), gc, lc = run(hip, "kernel", "compute", [q, q], s.scale_cost, s.max_iter, threads=t2, pad=7, tail="full")
    assert la == rs.sparse_plan(s.N, s.max_iter) and lb == ("one_wg", 1, 1, 1024) and lc == ("one_wg", 2, 1, t2), (la, lb, lc)
    intact(gb, name); intact(gc, name)
    check(a, ref["compute"], name + " solver path", tail=False)
    for other, what in ((b, "one workgroup"), (c0, "batch of two, instance 0"), (c1, "batch of two, instance 1")):
        check(other, a, f"{name}: {what} against the solver path", tail=False)
        check(other, ref["compute"], f"{name}: {what}")


def test_launches_cover_every_branch(hip):
    """what the hook reports for the shapes of this file: k_ruiz_sparse<true> on 2, 3, 47 and 48 workgroups, k_ruiz_sparse<false> with 64, 256 and 1024 threads on
    batches of 1 and 3, the dense tile grids of every n listed"""
    seen = set()
    for s in rs.all_shapes():
        q = s.instances()[0]
        if s.kind == "batch":
            threads, tail, pad = kernel_args(s)
            _, _, launch = run(hip, "kernel", "unscale", list(s.instances()), scals=[rs.unit_scalings(q.n, q.p, q.m)] * len(s.instances()), threads=threads, pad=pad, tail=tail)
        else:
            _, _, launch = run(hip, solver_path(s), "compute", [q], s.scale_cost, min(s.max_iter, 1) if s.max_iter <= 64 else s.max_iter)
        seen.add(launch)
    assert {("grid", g, 1, 256) for g in (2, 3, 47, 48)} <= seen
    assert {("one_wg", 3, 1, 64), ("one_wg", 3, 1, 256), ("one_wg", 3, 1, 1024), ("one_wg", 1, 1, 1024)} <= seen
    assert {("dense", 1, 1, 256), ("dense", 1, 2, 256), ("dense", 1, 8, 256), ("dense", 2, 9, 256), ("dense", 3, 17, 256)} <= seen


def test_hook_refuses_what_a_kernel_would_index_with(hip):
    """a pattern, an index list, a thread count or a stride that would send a kernel out of bounds is an error before anything is launched"""
    q = rs.shape("k_b3_t64").instances()[0]
    bad = q.copy()
    ri = q.GT[1].copy(); ri[-1] = q.n
    bad.GT = (q.GT[0], ri, q.GT[2].copy())
    with pytest.raises(RuntimeError, match="GT: row index out of range"):
        run(hip, "kernel", "compute", [bad], threads=64)
    bad = q.copy()
    ri = q.P[1].copy(); ri[0] = q.n - 1
    bad.P = (q.P[0], ri, q.P[2].copy())
    with pytest.raises(RuntimeError, match="P: not upper triangular"):
        run(hip, "solver_sparse", "compute", [bad])
    bad = q.copy(x_l_idx=np.where(np.arange(q.x_l_idx.size) == 0, q.n, q.x_l_idx).astype(np.int32))
    with pytest.raises(RuntimeError, match="x_l_idx out of range"):
        run(hip, "kernel", "compute", [bad], threads=64, tail="full")
    with pytest.raises(RuntimeError, match="threads must be a multiple of 64"):
        run(hip, "kernel", "compute", [q], threads=100)
    with pytest.raises(RuntimeError, match="does not hold the layout"):
        run(hip, "kernel", "compute", [q], threads=64, pad=-1)
